"""CPU: the order in which the vote grid takes the reference points of a batch (oslam_vote_ref_order): a permutation
whatever the demands are, heavy classes first, index order inside a class."""
import ctypes as C

import numpy as np
import pytest


def _is_permutation(order, n):
    return np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))


def test_params_carry_the_switch(ppf, built_lib):
    p = ppf.default_params()
    assert p.vote_order == 0 and C.sizeof(ppf.Params) == 64
    assert ppf.default_params(vote_order=1).vote_order == 1


@pytest.mark.parametrize("n", [0, 1, 2, 8, 13, 4097])
def test_equal_demands_keep_the_index_order(ppf, built_lib, n):
    for value in (0, 1, 299, 0xffffffff):
        order = ppf.vote_ref_order(np.full(n, value, np.uint32))
        assert np.array_equal(order, np.arange(n, dtype=np.uint32))


def test_one_heavy_reference_point_last_goes_first(ppf, built_lib):
    for n in (2, 9, 13, 1000):
        keep = np.zeros(n, np.uint32)
        keep[-1] = 299
        order = ppf.vote_ref_order(keep)
        assert np.array_equal(order, np.concatenate([[n - 1], np.arange(n - 1)]).astype(np.uint32))


def test_random_demands(ppf, built_lib):
    rng = np.random.default_rng(11)
    for n, top in ((13, 50), (1000, 3), (12500, 99999), (5000, 0xffffffff)):
        keep = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
        order = ppf.vote_ref_order(keep)
        assert _is_permutation(order, n)
        # classes of demand: 1024 of equal width up to the largest; descending, index order inside one
        cls = keep[order].astype(np.uint64) * np.uint64(1023) // np.uint64(max(int(keep.max()), 1))
        assert np.all(cls[1:] <= cls[:-1])
        same = cls[1:] == cls[:-1]
        assert np.all(order[1:][same] > order[:-1][same])
        # no reference point stands behind one of less than 1/1023 of the largest demand below its own
        assert np.all(keep[order][1:].astype(np.int64) - keep[order][:-1].astype(np.int64) <= int(keep.max()) // 1023 + 1)
