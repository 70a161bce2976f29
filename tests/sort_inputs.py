"""Deterministic inputs at the edges of the hit sort (k_sort_hits): list lengths around the wave shares, the block and
the segments, every pass count of both element widths, key patterns that stress one digit or the run cutting, markers
that must stay in their own run, and several lists in one launch.

Every case is a named builder that returns (id_bits, lists, prove): `lists` holds one (numbers, theta, idx, count) per
list of the launch, in arrival order, and prove(details, lists) asserts FROM THE RESTATEMENT ALONE (sort_ref's per-run
detail) that the case reaches the edge it is named for.  tests/test_sort_host.py runs every prove on a machine without a
GPU; tests/test_gpu_sort_hits.py compares the device with the restatement on the same inputs.  numpy only, seeded."""
import numpy as np

import sort_ref as R

MARKER = R.MARKER
NARROW_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 1023, 1024, 1025, 2048, 16383, 16384, 16385, 32768, 32769]
WIDE_LENGTHS = [1, 8191, 8192, 8193, 16385, 24577]
NARROW_BITS = [1, 7, 8, 9, 16, 17, 18]
WIDE_BITS = [19, 24, 25, 26]
MAX_HITS = 33000

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def mk(keys, salt, rng, theta=None, count=None):
    """a list from its key numbers: idx = arrival position + salt (stability shows), theta random and no marker"""
    keys = np.asarray(keys, np.int64).astype(np.uint32)
    n = len(keys)
    th = rng.integers(0, 1 << 22, n, dtype=np.int64).astype(np.uint32) if theta is None else np.asarray(theta, np.uint32)
    return keys, th, (np.arange(n, dtype=np.int64) + salt).astype(np.uint32), n if count is None else count


def heavy(rng, n, bits):
    """heavy-tailed key numbers: most hits under a few small numbers (long runs), a tenth spread over the whole range"""
    top = (1 << bits) - 1
    k = np.minimum((rng.pareto(0.7, n) * 3.0).astype(np.int64), top)
    wide = rng.random(n) < 0.1
    k[wide] = rng.integers(0, top + 1, int(wide.sum()))
    if n >= 4:
        k[n // 3], k[n // 2] = top, 0
    return k


def n_segments(detail):
    return len({d[0] for d in detail})


def runs_of(detail, key):
    return [d for d in detail if d[3] == key]


def passes(bits):
    return (bits + 7) // 8


# ---------------------------------------------------------------- lengths
@case
def lengths_up_to_two_blocks():
    rng = np.random.default_rng(101)
    lens = [n for n in NARROW_LENGTHS if n <= 2048]
    lists = [mk(heavy(rng, n, 16), 1000 * i, rng) for i, n in enumerate(lens)]

    def prove(details, lists):
        assert [sum(d[2] for d in det) for det in details] == lens
        assert details[0] == [] and len(details[1]) == 1
        assert all(n_segments(det) <= 1 for det in details)
        assert any(d[2] == 64 for d in details[lens.index(2048)])          # a full group under one key
    return 16, lists, prove


@case
def lengths_around_one_segment():
    rng = np.random.default_rng(102)
    lens = [16383, 16384, 16385]
    lists = [mk(heavy(rng, n, 9), 7 * i, rng) for i, n in enumerate(lens)]

    def prove(details, lists):
        assert [n_segments(det) for det in details] == [1, 1, 2]
        assert [d[:3] for d in details[2] if d[0] == 16384] == [(16384, 0, 1)]   # the second segment: one hit, one run
    return 9, lists, prove


@case
def lengths_around_two_segments():
    rng = np.random.default_rng(103)
    lens = [32768, 32769]
    lists = [mk(heavy(rng, n, 18), 50000 * i, rng) for i, n in enumerate(lens)]

    def prove(details, lists):
        assert [n_segments(det) for det in details] == [2, 3]
        assert details[1][-1][:3] == (32768, 0, 1)
        assert R.seg_of(18) == 16384
    return 18, lists, prove


@case
def lengths_wide():
    rng = np.random.default_rng(104)
    lists = [mk(heavy(rng, n, 19), 30000 * i, rng) for i, n in enumerate(WIDE_LENGTHS)]

    def prove(details, lists):
        assert R.seg_of(19) == 8192
        assert [n_segments(det) for det in details] == [1, 1, 1, 2, 3, 4]
        assert all(max(int(l[0].max()), 0) >= 1 << 18 for l in lists[1:])   # numbers the narrow word cannot hold
    return 19, lists, prove


# ---------------------------------------------------------------- id_bits: pass counts and the buffer the result ends in
def _bits_case(bits, n, seed):
    def build():
        rng = np.random.default_rng(seed)
        k = rng.integers(0, 1 << bits, n)
        k[0], k[n - 1] = (1 << bits) - 1, 0
        lists = [mk(k, bits, rng)]

        def prove(details, lists):
            assert R.seg_of(bits) == (16384 if bits <= 18 else 8192)
            keys = [d[3] for d in details[0]]
            assert keys[0] == 0 and keys[-1] == (1 << bits) - 1 and keys == sorted(keys)
            assert passes(bits) == {1: 1, 7: 1, 8: 1, 9: 2, 16: 2, 17: 3, 18: 3, 19: 3, 24: 3, 25: 4, 26: 4}[bits]
            if bits > 8:                                                     # every pass has work: the top digit varies
                assert len({k >> (8 * (passes(bits) - 1)) for k in keys}) > 1
        return bits, lists, prove
    build.__name__ = "id_bits_%d" % bits
    return case(build)


for _b in NARROW_BITS:
    _bits_case(_b, 1500, 200 + _b)            # 1500: shares of 128, the last waves empty, the last share ragged
for _b in WIDE_BITS:
    _bits_case(_b, 2100, 200 + _b)


# ---------------------------------------------------------------- key patterns
@case
def all_equal_key_zero():
    rng = np.random.default_rng(301)
    lists = [mk(np.zeros(200), 5, rng)]

    def prove(details, lists):
        assert [d[1:] for d in details[0]] == [(0, 64, 0, False), (64, 64, 0, False), (128, 64, 0, False), (192, 8, 0, False)]
    return 8, lists, prove


@case
def all_equal_top_key_full_segment():
    """18 bits and a full segment: the element of the last hit, key << 14 | place, is all ones"""
    rng = np.random.default_rng(302)
    top = (1 << 18) - 1
    lists = [mk(np.full(16384, top), 9, rng)]

    def prove(details, lists):
        assert ((top << 14) | 16383) == 0xFFFFFFFF
        assert len(details[0]) == 256 and all(d[2] == 64 and d[3] == top for d in details[0])
    return 18, lists, prove


@case
def all_equal_top_key_wide():
    rng = np.random.default_rng(303)
    top = (1 << 26) - 1
    lists = [mk(np.full(8192, top), 11, rng)]

    def prove(details, lists):
        assert len(details[0]) == 128 and all(d[2] == 64 and d[3] == top for d in details[0])
        assert (top | (63 << R.RUN_SHIFT)) == 0xFFFFFFFF                    # slot_r of every run is all ones
    return 26, lists, prove


@case
def distinct_descending():
    rng = np.random.default_rng(304)
    lists = [mk(np.arange(16383, -1, -1), 3, rng)]

    def prove(details, lists):
        assert len(details[0]) == 16384 and all(d[2] == 1 for d in details[0])
        assert [d[3] for d in details[0][:3]] == [0, 1, 2]
    return 14, lists, prove


@case
def distinct_descending_wide():
    rng = np.random.default_rng(305)
    top = (1 << 19) - 1
    lists = [mk(top - np.arange(8192) * 64, 3, rng)]

    def prove(details, lists):
        assert len(details[0]) == 8192 and all(d[2] == 1 for d in details[0])
        assert details[0][-1][3] == top
    return 19, lists, prove


@case
def two_alternating_keys():
    rng = np.random.default_rng(306)
    k = np.where(np.arange(1025) % 2 == 0, 0x1FFFF, 5)
    lists = [mk(k, 77, rng)]

    def prove(details, lists):
        assert {d[3] for d in details[0]} == {5, 0x1FFFF}
        assert sum(d[2] for d in runs_of(details[0], 5)) == 512 and sum(d[2] for d in runs_of(details[0], 0x1FFFF)) == 513
        assert (512, 1, 5, False) not in [d[1:] for d in details[0]] and (512, 64, 0x1FFFF, False) in [d[1:] for d in details[0]]
    return 17, lists, prove


def _digit_case(name, bits, which, n, seed):
    def build():
        rng = np.random.default_rng(seed)
        shift = 8 * (passes(bits) - 1) if which == "top" else 0
        width = min(8, bits - shift)
        fixed = (0x2B3C4D5 & ((1 << bits) - 1)) & ~(((1 << width) - 1) << shift)
        k = fixed | (rng.integers(0, 1 << width, n) << shift)
        lists = [mk(k, 13, rng)]

        def prove(details, lists):
            keys = {d[3] for d in details[0]}
            assert len(keys) == 1 << width                                   # every value of the digit
            assert {k ^ fixed for k in keys} == {v << shift for v in range(1 << width)}   # and nothing but the digit
        return bits, lists, prove
    build.__name__ = name
    return case(build)


_digit_case("top_digit_only", 18, "top", 3000, 311)
_digit_case("bottom_digit_only", 18, "bottom", 3000, 312)
_digit_case("top_digit_only_wide", 26, "top", 3000, 313)
_digit_case("bottom_digit_only_wide", 26, "bottom", 3000, 314)


@case
def already_sorted():
    rng = np.random.default_rng(320)
    lists = [mk(np.sort(heavy(rng, 4097, 16)), 21, rng)]

    def prove(details, lists):
        k = lists[0][0].astype(np.int64)
        assert np.all(k[1:] >= k[:-1]) and len(np.unique(k)) > 100
    return 16, lists, prove


def _stretches(bits, base, seed):
    """equal-key stretches of 64, 128, 65 and 129, then 63 single keys and a second stretch of 129 that starts on a
    multiple of 64; the arrival order is a seeded shuffle"""
    rng = np.random.default_rng(seed)
    k = np.concatenate([np.full(64, base + 1), np.full(128, base + 2), np.full(65, base + 3), np.full(129, base + 4),
                        base + 10 + np.arange(62), np.full(129, base + 100)])
    lists = [mk(rng.permutation(k), 31, rng)]

    def prove(details, lists):
        shape = lambda key: [(d[1], d[2]) for d in runs_of(details[0], key)]      # noqa: E731
        assert shape(base + 1) == [(0, 64)]                                   # exactly 64, from a multiple of 64
        assert shape(base + 2) == [(64, 64), (128, 64)]
        assert shape(base + 3) == [(192, 64), (256, 1)]
        assert shape(base + 4) == [(257, 63), (320, 64), (384, 2)]
        assert shape(base + 100) == [(448, 64), (512, 64), (576, 1)]
    return bits, lists, prove


@case
def equal_key_stretches():
    return _stretches(12, 0, 330)


@case
def equal_key_stretches_wide():
    return _stretches(20, 1 << 19, 331)


def _boundary(bits, key, seed):
    rng = np.random.default_rng(seed)
    seg = R.seg_of(bits)
    k = rng.integers(0, 1 << bits, seg + 100)
    k[k == key] = key + 1
    k[seg - 3:seg + 4] = key                                                  # three hits before the boundary, four after
    lists = [mk(k, 41, rng)]

    def prove(details, lists):
        rs = runs_of(details[0], key)
        assert [(d[0], d[2]) for d in rs] == [(0, 3), (seg, 4)]               # one run per segment
        assert rs[1][0] + rs[1][1] >= seg                                     # `first` goes on past the boundary
    return bits, lists, prove


@case
def key_on_both_sides_of_a_segment_boundary():
    return _boundary(16, 40000, 340)


@case
def key_on_both_sides_of_a_segment_boundary_wide():
    return _boundary(20, 700000, 341)


# ---------------------------------------------------------------- markers
@case
def marker_in_the_first_and_in_the_last_hit_of_a_run():
    rng = np.random.default_rng(401)
    k = rng.permutation(np.concatenate([np.full(5, 20), np.full(5, 30), np.arange(100, 130)]))
    keys, th, idx, n = mk(k, 51, rng)
    th[np.nonzero(k == 20)[0][0]] = MARKER                                    # stable: the first to arrive is the first of the run
    th[np.nonzero(k == 30)[0][-1]] = MARKER
    lists = [(keys, th, idx, n)]

    def prove(details, lists):
        assert [d[3] for d in details[0] if d[4]] == [20, 30]
        ref = R.sort_list(*lists[0], 8)
        a, b = runs_of(details[0], 20)[0], runs_of(details[0], 30)[0]
        assert ref["theta"][a[1]] == MARKER and ref["theta"][b[1] + b[2] - 1] == MARKER
        assert (ref["theta"] == MARKER).sum() == 2
    return 8, lists, prove


def _marker_130(bits, key, seed):
    rng = np.random.default_rng(seed)
    keys, th, idx, n = mk(np.full(130, key), 61, rng)
    th[129] = MARKER
    lists = [(keys, th, idx, n)]

    def prove(details, lists):
        assert [d[1:] for d in details[0]] == [(0, 64, key, False), (64, 64, key, False), (128, 2, key, True)]
        ref = R.sort_list(*lists[0], bits)
        assert np.array_equal(np.nonzero(ref["numbers"] & R.FLAG)[0], [128, 129])   # only the third run's two key words
    return bits, lists, prove


@case
def marker_in_the_last_of_130_equal_keys():
    return _marker_130(10, 777, 402)


@case
def marker_in_the_last_of_130_equal_keys_wide():
    return _marker_130(24, (1 << 24) - 2, 403)


@case
def marked_key_between_two_clean_ones_in_one_group():
    rng = np.random.default_rng(404)
    k = rng.permutation(np.concatenate([np.full(10, 300), np.full(7, 301), np.full(12, 302)]))
    keys, th, idx, n = mk(k, 71, rng)
    th[np.nonzero(k == 301)[0][3]] = MARKER
    lists = [(keys, th, idx, n)]

    def prove(details, lists):
        assert [d[1:] for d in details[0]] == [(0, 10, 300, False), (10, 7, 301, True), (17, 12, 302, False)]
    return 9, lists, prove


@case
def every_hit_marked():
    rng = np.random.default_rng(405)
    lists = [mk(heavy(rng, 300, 16), 81, rng, theta=np.full(300, MARKER))]

    def prove(details, lists):
        assert details[0] and all(d[4] for d in details[0])
    return 16, lists, prove


@case
def theta_one_below_the_marker_marks_nothing():
    rng = np.random.default_rng(406)
    lists = [mk(heavy(rng, 300, 16), 91, rng, theta=np.full(300, MARKER - 1))]

    def prove(details, lists):
        assert details[0] and not any(d[4] for d in details[0])
        assert not np.any(R.sort_list(*lists[0], 16)["numbers"] & R.FLAG)
    return 16, lists, prove


# ---------------------------------------------------------------- several lists in one launch
@case
def lists_side_by_side_wide():
    rng = np.random.default_rng(502)
    lens = [0, 1, 64, 16385, 0, 8193]
    lists = [mk(heavy(rng, n, 19), 20000 * i, rng) for i, n in enumerate(lens)]

    def prove(details, lists):
        assert [n_segments(det) for det in details] == [0, 1, 1, 3, 0, 2]
        assert [sum(d[2] for d in det) for det in details] == lens
    return 19, lists, prove


@case
def counts_beyond_the_slots_and_below():
    """count = slots + 5 and count = all ones sort the slots and no more; an empty list between them and a list that is
    filled to a third keep what they held"""
    rng = np.random.default_rng(503)
    slots = [100, 70, 300, 90]
    counts = [105, 0, 0xFFFFFFFF, 30]
    lists = [mk(heavy(rng, s, 16), 1000 * i, rng, count=c) for i, (s, c) in enumerate(zip(slots, counts))]

    def prove(details, lists):
        assert [sum(d[2] for d in det) for det in details] == [100, 0, 300, 30]
        ref = R.sort_list(*lists[3], 16)
        assert np.array_equal(ref["numbers"][30:], lists[3][0][30:]) and np.all(ref["theta"][30:] == R.SENTINEL)
        assert np.all(ref["runs"][ref["run_count"]:] == R.SENTINEL)
        ref1 = R.sort_list(*lists[1], 16)
        assert np.array_equal(ref1["numbers"], lists[1][0]) and np.all(ref1["idx"] == R.SENTINEL) and ref1["run_count"] == 0
    return 16, lists, prove


# ---------------------------------------------------------------- a launch's arrays
def build(name):
    """-> (id_bits, numbers, theta, idx, offsets, counts, lists, prove): the case's lists laid side by side"""
    bits, lists, prove = CASES[name]()
    offsets = np.concatenate([[0], np.cumsum([len(l[0]) for l in lists])]).astype(np.uint32)
    cat = lambda j: np.concatenate([l[j] for l in lists]).astype(np.uint32)      # noqa: E731
    counts = np.array([l[3] for l in lists], np.uint32)
    return bits, cat(0), cat(1), cat(2), offsets, counts, lists, prove


_REFS = {}


def reference(name):
    """the case's arrays and the restatement's answer, computed once per process and never changed"""
    if name not in _REFS:
        bits, num, th, idx, off, cnt, lists, prove = build(name)
        want = R.sort_lists(num, th, idx, off, cnt, bits)
        for a in (num, th, idx, off, cnt) + want[:5]:
            a.setflags(write=False)
        _REFS[name] = (bits, (num, th, idx, off, cnt), want, lists, prove)
    return _REFS[name]
