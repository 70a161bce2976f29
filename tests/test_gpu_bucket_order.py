"""GPU: k_bucket_spread and k_bucket_psort alone, through oslam_bucket_order_tap, on every case of tests/bucket_inputs.py.

The six arrays the tap copies back -- the entry words, their uv and mi in the spread's order, the second order pw / puv
and its directories pdir -- equal the restatement (tests/bucket_ref.py) word for word, the places the kernels do not own
included: padding words come back as they went up, and the tap fills pw, puv and pdir with 0xA5 bytes before the
launches.  Integers and floats' bit patterns only: no tolerance.  tests/test_bucket_host.py proves on the CPU that every
case reaches the edge it is named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bucket_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("e4", "uv", "mi", "pw", "puv", "pdir")


def _first_difference(got, want):
    at = np.argwhere(got != want)
    return None if len(at) == 0 else (tuple(at[0].tolist()), hex(int(got[tuple(at[0])])), hex(int(want[tuple(at[0])])))


def _run(ppf, L):
    got = ppf.bucket_order(L.lens, L.e4, L.uv.view(np.float32), L.mi, keys=L.keys, **{k: L.flags[k] for k in ("with_uv", "spread")})
    return tuple(g.view(np.uint32) if g.dtype == np.float32 else g for g in got)


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_orders_equal_the_restatement(ppf, name):
    L, _ = I.reference(name)
    for what, g, w in zip(NAMES, _run(ppf, L), L.want):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert np.array_equal(g, w), (name, what, "first difference (place, got, want)", _first_difference(g, w),
                                      "bucket starts", L.starts.tolist(), "lengths", L.lens.tolist())


def test_keys_default_to_the_bucket_number(ppf):
    """keys = None: every slot is keyed, the key's value is nothing to the two kernels"""
    L, _ = I.reference("one_bucket")
    got = ppf.bucket_order(L.lens, L.e4, L.uv.view(np.float32), L.mi)
    assert all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w) for g, w in zip(got, L.want))


def test_orders_are_the_same_twice(ppf):
    """the same launch again: ties go by arrival index and by position, not by which wave got there first"""
    L, _ = I.reference("lengths_around_one_segment")
    first, again = _run(ppf, L), _run(ppf, L)
    assert all(np.array_equal(a, b) and np.array_equal(a, w) for a, b, w in zip(first, again, L.want))
