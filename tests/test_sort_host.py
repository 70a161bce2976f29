"""CPU: the hit sort's restatement (tests/sort_ref.py) on lists small enough to write the answer down, the cases of
tests/sort_inputs.py -- every one proves from the restatement alone that it reaches the edge it is named for, and the
table as a whole covers the lengths and id_bits it promises -- the clouds of tests/test_gpu_wide_keys.py on the CPU oracle
(more than 2^18 keys, more than a segment of hits, a key with more than one run, the mixed run's shared key), and the
argument checks of oslam_sort_hits_tap, which refuse before a device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_inputs as I  # noqa: E402
import sort_ref as R  # noqa: E402

A5 = R.SENTINEL
M = R.MARKER
FLAG = R.FLAG


def u32(*v):
    return np.array(v, np.uint32)


# ---------------------------------------------------------------- the restatement
def test_restatement_on_a_list_written_down():
    #            arrival: 0  1  2  3  4  5   (two slots past the count)
    num = u32(7, 3, 7, 0, 3, 7, 9, 1)
    th = u32(10, 11, M, 13, 14, 15, M, 17)
    idx = u32(100, 101, 102, 103, 104, 105, 106, 107)
    r = R.sort_list(num, th, idx, 6, 4)
    assert r["numbers"].tolist() == [0, 3, 3, 7 | FLAG, 7 | FLAG, 7 | FLAG, 9, 1]      # past the count: the input
    assert r["theta"].tolist() == [13, 11, 14, 10, M, 15, A5, A5]
    assert r["idx"].tolist() == [103, 101, 104, 100, 102, 105, A5, A5]                 # equal keys in arrival order
    assert r["run_count"] == 3
    assert r["runs"].tolist() == [[0, 0], [3 | 1 << 26, 1], [7 | 2 << 26, 3 | FLAG]] + [[A5, A5]] * 5
    assert r["detail"] == [(0, 0, 1, 0, False), (0, 1, 2, 3, False), (0, 3, 3, 7, True)]


def test_restatement_cuts_runs_at_64_and_at_segments():
    n = 16384 + 70
    num = np.full(n, 5, np.uint32)
    th = np.zeros(n, np.uint32)
    th[16384 + 65] = M
    r = R.sort_list(num, th, np.arange(n, dtype=np.uint32), n, 18)
    assert r["run_count"] == 256 + 2
    assert r["runs"][255].tolist() == [5 | 63 << 26, 16320] and r["runs"][256].tolist() == [5 | 63 << 26, 16384]
    assert r["runs"][257].tolist() == [5 | 5 << 26, (16384 + 64) | FLAG]
    assert np.array_equal(np.nonzero(r["numbers"] & FLAG)[0], np.arange(16384 + 64, n))
    wide = R.sort_list(num, th, np.arange(n, dtype=np.uint32), n, 19)                  # half the segment: 8192
    assert wide["run_count"] == 128 + 128 + 2 and wide["runs"][128].tolist() == [5 | 63 << 26, 8192]
    assert R.seg_of(18) == 16384 and R.seg_of(19) == 8192 and R.seg_of(26) == 8192 and R.seg_of(1) == 16384


def test_restatement_of_several_lists_leaves_each_its_slots():
    num = u32(2, 1, 9, 9, 4, 3)
    th = u32(0, 1, 2, 3, 4, 5)
    idx = u32(0, 1, 2, 3, 4, 5)
    n, t, i, runs, rc, _ = R.sort_lists(num, th, idx, u32(0, 2, 4, 6), u32(7, 0, 1), 4)
    assert n.tolist() == [1, 2, 9, 9, 4, 3] and t.tolist() == [1, 0, A5, A5, 4, A5] and i.tolist() == [1, 0, A5, A5, 4, A5]
    assert rc.tolist() == [2, 0, 1]
    assert runs.tolist() == [[1, 0], [2, 1], [A5, A5], [A5, A5], [4, 0], [A5, A5]]     # `first` counts from the list's start


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", sorted(I.CASES))
def test_case_reaches_its_edge(name):
    bits, (num, th, idx, off, cnt), want, lists, prove = I.reference(name)
    assert 1 <= bits <= 26 and len(off) == len(cnt) + 1 == len(lists) + 1
    assert all(len(l[0]) <= I.MAX_HITS for l in lists)
    assert len(num) == 0 or int(num.max()) < 1 << bits
    for l, (k, t, i, c) in enumerate(lists):                                # idx = arrival position + the list's salt
        assert len(i) == 0 or np.array_equal(i - i[0], np.arange(len(i), dtype=np.uint32))
    prove(want[5], lists)
    # what any answer must satisfy: a permutation of the payloads per segment, keys ascending, stable
    for l in range(len(cnt)):
        a, b = int(off[l]), int(off[l + 1])
        n = min(int(cnt[l]), b - a)
        seg = R.seg_of(bits)
        for s in range(a, a + n, seg):
            e = min(s + seg, a + n)
            ks = (want[0][s:e] & ~np.uint32(FLAG)).astype(np.int64)
            assert np.all(ks[1:] >= ks[:-1])
            assert np.array_equal(np.sort(want[2][s:e]), idx[s:e])
            same = ks[1:] == ks[:-1]
            assert np.all(want[2][s + 1:e][same] > want[2][s:e - 1][same])


def test_table_covers_the_lengths_and_id_bits():
    narrow, wide, bits_seen, n_lists = set(), set(), set(), 0
    for name in I.CASES:
        bits, arrays, want, lists, _ = I.reference(name)
        bits_seen.add(bits)
        n_lists += len(lists)
        for l in lists:
            (narrow if bits <= 18 else wide).add(min(int(l[3]), len(l[0])))
    assert set(I.NARROW_LENGTHS) <= narrow and set(I.WIDE_LENGTHS) <= wide
    assert set(I.NARROW_BITS + I.WIDE_BITS) <= bits_seen
    assert n_lists <= 72                                                     # a few dozen lists, no full product


# ---------------------------------------------------------------- the clouds of test_gpu_wide_keys, on the oracle
def test_wide_key_clouds_are_what_they_are_named_for(oracle):
    import test_gpu_wide_keys as W
    for bins in (1500, 3000):
        mp, mn, d = W.wide_model(bins)
        keys = W.oracle_key_set(oracle, mp, mn, d)
        assert len(keys) > W.WIDE, (bins, len(keys))                         # 19 bits of key numbers: the 64-bit sort
        sp, sn = W.wide_scene(mp, mn)
        for r in W.WIDE_REFS:
            row = oracle.ppf_row_keys(sp, sn, r, d)
            hit = (row != 0) & np.isin(row, keys)
            hit[r] = False
            assert hit.sum() > 8192 and np.unique(row[hit], return_counts=True)[1].max() > 64, (bins, r)
    ca, cb, d = W.group_models()
    ka, kb = (W.oracle_key_set(oracle, c[0], c[1], d) for c in (ca, cb))
    assert len(ka) < W.WIDE and len(kb) < W.WIDE and len(np.union1d(ka, kb)) > W.WIDE
    mp, mn, sp, sn, d = W.mixed_run_case()
    row = oracle.ppf_row_keys(sp, sn, 0, d)
    assert row[W.MIXED_ON_AXIS] == row[W.MIXED_OFF_AXIS] == oracle.ppf_row_keys(mp, mn, 0, d)[W.MIXED_ON_AXIS] != 0
    assert np.count_nonzero(row == row[W.MIXED_ON_AXIS]) == 2 and np.isin(row, W.oracle_key_set(oracle, mp, mn, d)).sum() <= 64


# ---------------------------------------------------------------- the tap's argument checks
def test_sort_tap_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    L, INV = ppf.lib(), ppf.OSLAM_E_INVALID
    num, th, idx = u32(1, 0, 3, 2), u32(0, 0, 0, 0), u32(0, 1, 2, 3)
    off, cnt = u32(0, 2, 4), u32(2, 2)
    outs = [np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros((4, 2), np.uint32), np.zeros(2, np.uint32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731

    def call(ins=(num, th, idx, off, cnt), n=2, bits=2, outs=outs, null=None):
        args = [p(a) for a in ins] + [n, bits, 0] + [p(a) for a in outs]
        if null is not None:
            args[null if null < 5 else null + 3] = None
        return L.oslam_sort_hits_tap(*args)

    for k in range(10):                                                      # every array, in and out
        assert call(null=k) == INV, k
    assert b"NULL" in L.oslam_last_error()
    assert call(ins=(num, th, idx, u32(0, 3, 2), cnt)) == INV                # offsets that descend
    assert b"descend" in L.oslam_last_error()
    assert call(ins=(num, th, idx, u32(2, 1, 4), cnt)) == INV
    for bits in (0, 27, 32, 0xFFFFFFFF):
        assert call(bits=bits) == INV, bits
    assert call(bits=1) == INV                                               # 3 and 2 do not fit one bit
    assert b"id_bits" in L.oslam_last_error()
    assert call(ins=(u32(1, 0, 1 << 26, 2), th, idx, off, cnt), bits=26) == INV
    assert call(ins=(u32(1, 0, 0xFFFFFFFF, 2), th, idx, off, cnt), bits=26) == INV
    assert call(n=0) == ppf.OSLAM_OK                                         # no list: nothing to launch, no device
    with pytest.raises(ValueError):
        ppf.sort_hits(num, th, idx, u32(0, 2), cnt, 2)
    with pytest.raises(ValueError):
        ppf.sort_hits(num, th[:3], idx, off, cnt, 2)
