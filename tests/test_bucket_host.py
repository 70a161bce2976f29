"""CPU: the restatement of the two orders inside a model's buckets (tests/bucket_ref.py) on buckets small enough to
write the answer down, the cases of tests/bucket_inputs.py -- every one proves from the restatement alone that it reaches
the edge it is named for, and the table as a whole covers the lengths it promises -- the directory's size rule, and the
argument checks of oslam_bucket_order_tap, which refuse before a device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bucket_inputs as I  # noqa: E402
import bucket_ref as R  # noqa: E402

A5, A5H = R.A5_32, R.A5_16
SINK = R.ROW_SINK


def u32(*v):
    return np.array(v, np.uint32)


def one_bucket(words, with_uv=True, spread=True, key=1):
    """a launch of one bucket: uv = (arrival index, 100 + arrival index), mi = arrival index, sink padding"""
    n = len(words)
    total = (n + 3) & ~3
    e4 = np.full(total, SINK, np.uint32)
    e4[:n] = words
    uv = np.stack([np.arange(total), 100 + np.arange(total)], 1).astype(np.uint32)
    mi = np.arange(total).astype(np.uint16)
    return R.order_buckets([n], [key], e4, uv, mi, with_uv, spread)


# ---------------------------------------------------------------- the restatement
def test_spread_key_written_down():
    # angle field 0: the key is minus 31 rows, that is (row mod 32) banks, in units of 2^-16 bank
    assert R.spread_key(u32(0, 1, 3, 31, 32, 35, 1023)).tolist() == [0, 1 << 16, 3 << 16, 31 << 16, 0, 3 << 16, 31 << 16]
    # the half bit is no part of it; the angle field counts 30 / 32 of 2^-5 bank per unit
    assert R.spread_key(u32(1 << 10, 32 << 11, 33 << 11, (1 << 21) - 1 << 11)).tolist() == [0, 30, 30, ((1 << 21) - 1) * 30 >> 5]
    assert R.spread_key(u32(32 << 11 | 1)).tolist() == [(30 + (1 << 16)) % (1 << 21)]
    assert R.spread_key(u32(5)).tolist() == [(0 - (5 * 31 << 16)) % (1 << 21)]


def test_spread_of_five_written_down():
    #   arrival:     0  1  2   3  4        keys (row mod 32): 5 3 3 0 31
    e4, uv, mi, pw, puv, pdir = one_bucket(u32(5, 3, 35, 0, 31), with_uv=False)
    # sorted by (key, arrival): 3 1 2 0 4; five positions are lanes 0 and 1: dealt in place order
    assert e4.tolist() == [0, 3, 35, 5, 31, SINK, SINK, SINK]
    assert mi.tolist() == [3, 1, 2, 0, 4, 5, 6, 7]
    assert uv[:, 0].tolist() == list(range(8))                               # the fast-mode build: no uv to move
    assert one_bucket(u32(5, 3, 35, 0, 31))[1].tolist() == [[3, 103], [1, 101], [2, 102], [0, 100], [4, 104], [5, 105], [6, 106], [7, 107]]
    assert np.all(pw == A5) and np.all(puv == A5) and np.all(pdir == A5H) and len(pdir) == 8 + 256


def test_second_order_of_five_written_down():
    # P = word * 30:   0, 2^30 + 26 (cell 1), 2^30 - 4 (cell 0), 3 * 2^30 + 18 (cell 3), and its twin under bit 31
    words = u32(107374183 ^ 0x80000000, 35791395, 0, 107374183, 35791394)
    assert R.p_of(words).tolist() == [3 * 2**30 + 18, 2**30 + 26, 0, 3 * 2**30 + 18, 2**30 - 4]
    e4, uv, mi, pw, puv, pdir = one_bucket(words, spread=False)
    assert e4[:5].tolist() == words.tolist()
    assert pw.tolist() == [0, 35791394, 35791395, 107374183 ^ 0x80000000, 107374183, A5, A5, A5]   # the tie: by position
    assert puv[:5, 0].tolist() == [2, 4, 1, 0, 3] and puv[:5, 1].tolist() == [102, 104, 101, 100, 103] and np.all(puv[5:] == A5)
    assert R.cells(5) == 4
    assert pdir[:8].tolist() == [0, 2, 3, 3, 5, A5H, A5H, A5H]              # cells 0 | 1 | - | 3, then n


def test_orders_of_nine_written_down():
    # nine entries, angle field 0 but for two: keys (row mod 32) << 16, + 30 per 32 units of the angle field
    words = u32(8, 7, 6, 5, 4, 3, 2, 1, 33)
    e4, uv, mi, pw, puv, pdir = one_bucket(words)
    # sorted by (key, arrival): rows 1 33 2 3 4 5 6 7 8 -> arrivals 7 8 6 5 4 3 2 1 0; lanes 0, 1, 2 in place order
    assert mi[:9].tolist() == [7, 8, 6, 5, 4, 3, 2, 1, 0] and e4[:9].tolist() == [1, 33, 2, 3, 4, 5, 6, 7, 8]
    # P = 30 * word, all in cell 0 of K = 8: ascending words
    assert R.cells(9) == 8
    assert pw[:9].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 33] and puv[:9, 0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0, 8]
    assert pdir[:12].tolist() == [0] + [9] * 8 + [A5H] * 3
    assert np.all(pw[9:] == A5) and e4[9:].tolist() == [SINK] * 3


def test_dealing_order_written_down():
    # 130 positions: lanes 0..31 full and two registers of lane 32, which shares h = 0 with lane 0 (g = 1)
    assert R.deal_positions(130)[:8].tolist() == [0, 128, 1, 129, 2, 3, 4, 5]
    # 258: a second chunk of two registers of lane 0; h = 0 takes its 8 places of chunk 0, then chunk 1, then h = 1
    assert R.deal_positions(258)[:12].tolist() == [0, 128, 1, 129, 2, 130, 3, 131, 256, 257, 4, 132]
    # a full segment: h = 0 over all 16 chunks first, (j, g) inside a chunk
    d = R.deal_positions(4096)
    assert d[:9].tolist() == [0, 128, 1, 129, 2, 130, 3, 131, 256] and d[128:130].tolist() == [4, 132] and d[-1] == 4095
    for n in (1, 2, 5, 129, 4095):
        assert np.array_equal(np.sort(R.deal_positions(n)), np.arange(n))
    # all keys equal, 130 entries: place 128 takes the entry that arrived second
    src = R.spread_segment(np.zeros(130, np.uint32))
    assert src[[0, 128, 1, 129, 2, 3, 4]].tolist() == [0, 1, 2, 3, 4, 5, 6]


def test_buckets_side_by_side_and_what_is_skipped():
    lens, keys = [1, 0, 2, 3], [9, 9, 0, 9]
    e4 = u32(50, 1, 2, 3, 7, 6, 4, 5, 35, 5, 3, 9)                           # padding words 1 2 3 / 4 5 / 9
    uv = np.arange(24, dtype=np.uint32).reshape(12, 2)
    mi = np.arange(12).astype(np.uint16)
    o = R.order_buckets(lens, keys, e4, uv, mi)
    assert o[0].tolist() == [50, 1, 2, 3, 7, 6, 4, 5, 35, 3, 5, 9]          # 35 and 3 tie in the key: arrival; 5 after them
    assert o[2].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 9, 11] and o[1][:, 0].tolist() == [0, 2, 4, 6, 8, 10, 12, 14, 16, 20, 18, 22]
    assert o[3].tolist() == [50, A5, A5, A5, A5, A5, A5, A5, 3, 5, 35, A5]
    assert o[5][:12].tolist() == [0, 1, A5H, A5H, A5H, A5H, A5H, A5H, 0, 3, 3, A5H]   # K = 1 | skipped | K = 2: cell 0, 3 entries
    assert R.starts_of(lens)[0].tolist() == [0, 4, 4, 8] and R.starts_of(lens)[1] == 12


def test_directory_never_leaves_its_segment():
    for n in range(1, 4097):
        K = R.cells(n)
        assert K & (K - 1) == 0 and 1 <= K <= 2048 and K + 1 <= max(n, 2), n
        assert n <= 2 or K < n <= 2 * K, n
    assert [R.cells(n) for n in (1, 2, 3, 4, 5, 8, 9, 4096)] == [1, 1, 2, 2, 4, 4, 8, 2048]


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", sorted(I.CASES))
def test_case_reaches_its_edge(name):
    L, prove = I.reference(name)
    assert 1 <= len(L.lens) <= 40 and int(L.lens.max()) <= I.MAX_LEN
    prove(L)
    e4, uv, mi, pw, puv, pdir = L.want
    assert len(pdir) == L.total + R.PDIR_TAIL
    # what any answer must satisfy: per segment a permutation that moves word, uv and mi together; pw ascending in P
    for b in range(len(L.lens)):
        for a, n in L.segments(b):
            src = mi[a:a + n].astype(np.int64) + int(L.starts[b])
            assert np.array_equal(np.sort(mi[a:a + n]), L.mi[a:a + n]) and np.array_equal(e4[a:a + n], L.e4[src])
            assert np.array_equal(uv[a:a + n], L.uv[src] if L.flags["with_uv"] else L.uv[a:a + n])
            if L.flags["with_uv"] and L.live(b):
                p = R.p_of(pw[a:a + n])
                assert np.all(p[1:] >= p[:-1]) and np.array_equal(np.sort(puv[a:a + n, 0]), L.uv[a:a + n, 0])


def test_table_covers_the_lengths_and_the_cells():
    seen, Ks, n_buckets = set(), set(), 0
    for name in I.CASES:
        L, _ = I.reference(name)
        n_buckets += len(L.lens)
        if L.flags["with_uv"] and L.flags["spread"]:
            seen |= {int(n) for b, n in enumerate(L.lens) if L.keys[b] != 0}
            Ks |= L.Ks()
    assert set(I.LENGTHS) <= seen
    assert {1, 2, 4, 2048} <= Ks
    assert n_buckets <= 120                                                  # a few dozen a launch, no full product
    kinds = [{L.flags["with_uv"], L.flags["spread"]} for L, _ in map(I.reference, I.CASES)]
    assert {False} in kinds and any(not I.reference(n)[0].flags["spread"] and I.reference(n)[0].flags["with_uv"] for n in I.CASES)


# ---------------------------------------------------------------- the tap's argument checks
def test_bucket_tap_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    L, INV = ppf.lib(), ppf.OSLAM_E_INVALID
    lens, keys = u32(2, 1), u32(1, 2)
    e4, uv, mi = np.zeros(8, np.uint32), np.zeros((8, 2), np.float32), np.zeros(8, np.uint16)
    outs = [np.zeros(8, np.uint32), np.zeros((8, 2), np.float32), np.zeros(8, np.uint16), np.zeros(8, np.uint32),
            np.zeros((8, 2), np.float32), np.zeros(8 + 256, np.uint16)]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731

    def call(lens=lens, keys=keys, n=2, ins=(e4, uv, mi), outs=outs):
        return L.oslam_bucket_order_tap(p(lens), p(keys), n, *[p(a) for a in ins], 1, 1, 0, *[p(a) for a in outs])

    assert call(lens=None) == INV
    assert b"NULL" in L.oslam_last_error()
    for k in range(3):
        assert call(ins=[None if j == k else a for j, a in enumerate((e4, uv, mi))]) == INV, k
    for k in range(6):
        assert call(outs=[None if j == k else a for j, a in enumerate(outs)]) == INV, k
    assert call(lens=u32(2, (1 << 20) + 1)) == INV
    assert b"2^20" in L.oslam_last_error()
    assert call(lens=u32(0xFFFFFFFF, 1)) == INV
    many = np.full(17, 1 << 20, np.uint32)                                   # 17 * 2^20 > 2^24
    assert call(lens=many, keys=None, n=17) == INV
    assert b"2^24" in L.oslam_last_error()
    assert call(n=0) == ppf.OSLAM_OK                                         # no bucket: nothing to launch, no device
    with pytest.raises(ValueError):
        ppf.bucket_order(lens, e4[:4], uv, mi)
    with pytest.raises(ValueError):
        ppf.bucket_order(lens, e4, uv, mi, keys=u32(1))
