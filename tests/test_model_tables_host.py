"""CPU: the clouds of tests/model_inputs.py prove, from the oracle and the restatement (tests/model_ref.py) alone, that
each reaches the edge it is named for; a build simulated in numpy with a seeded arrival order passes hold(), and tables
that are wrong in one place do not; the tables tap refuses bad arguments.

CPU time of the restatement per cloud (oracle keys, host words, reach and key map; process time over the helper's
OpenMP threads, wall time in brackets, measured on the development machine): points_2, points_3, markers, far_*, small,
small_other 2.1 .. 2.7 s (0.3 s) each, nearly all of it the 80 million hashes of the reach bitset; points_1023 3.1 s
(0.8 s), points_1024 3.6 s (0.9 s), points_2046 5.4 s (2.7 s), points_2047 5.3 s (2.8 s), growth 3.1 s (0.4 s),
points_4093 10 .. 16 s (8 .. 12 s: 16.7 million pairs, 3 s of it the oracle's keys; it appears once)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_inputs as I  # noqa: E402
import model_ref as R  # noqa: E402

SMALL = ("points_2", "points_3", "markers", "far_beyond_the_key_map", "far_beyond_reach", "small", "small_other")


def ref(name, oracle, ppf):
    return I.reference(name, oracle, ppf)


def bins_of_pairs(p, d):
    """distance of every ordered pair in units of d_dist, in double precision: far from any bin edge where it is used"""
    diff = p[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)
    return np.sqrt((diff ** 2).sum(-1)) / d


# ---------------------------------------------------------------- every cloud reaches its edge
@pytest.mark.parametrize("n", I.COUNTS)
def test_point_counts_reach_the_slice_and_half_boundaries(built_lib, oracle, ppf, n):
    p, nr, d, m, u = ref("points_%d" % n, oracle, ppf)
    assert m.M == n and m.n_slices == {2: 1, 3: 1, 1023: 1, 1024: 1, 2046: 1, 2047: 2, 4093: 3}[n]
    per_slice = [len(np.unique(m.r[m.slice == s])) for s in range(m.n_slices)]
    assert per_slice == {2: [2], 3: [3], 1023: [1023], 1024: [1024], 2046: [2046], 2047: [2046, 1], 4093: [2046, 2046, 1]}[n]
    local = m.r % R.SLICE
    row11 = m.word & 0x7FF
    assert np.array_equal(row11, (local // R.HALF) << 10 | local % R.HALF)      # pc_row11, restated
    halves = [sorted(set((row11[m.slice == s] >> 10).tolist())) for s in range(m.n_slices)]
    assert halves == {2: [[0]], 3: [[0]], 1023: [[0]], 1024: [[0, 1]], 2046: [[0, 1]], 2047: [[0, 1], [0]],
                      4093: [[0, 1], [0, 1], [0]]}[n]
    assert int((row11 & 0x3FF).max()) == min(n, R.HALF) - 1 and not np.any((row11 & 0x3FF) == R.SINK)
    if n == 1024:                                                              # exactly one point in the second half: row 0
        assert set(row11[row11 >> 10 == 1].tolist()) == {1 << 10}
    if n in (2047, 4093):                                                      # a last slice of one point: n - 1 entries, row 0
        last = m.slice == m.n_slices - 1
        assert last.sum() == n - 1 and set(row11[last].tolist()) == {0}
    assert len(m.key) == n * (n - 1) - int((m.key == 0).sum()) and not np.any(m.key == 0)
    assert m.cap == 1 << 16 and m.n_entries >= len(m.key)
    if n == 4093:
        assert int(m.b_len.max()) > 4096                                       # a bucket of more than one segment
        assert u.ucap == 1 << 17 and u.n_ids * 4 < 1 << 16                     # sized by the slices' counts, which share most keys
    if n >= 1023:
        assert int(m.b_len.max()) > 256 and np.count_nonzero(m.b_len == 1) > 0


def test_markers_cloud_has_a_marker_in_a_bucket_with_clean_pairs(built_lib, oracle, ppf):
    p, nr, d, m, u = ref("markers", oracle, ppf)
    assert m.force.sum() >= 1 + 6 and np.any(m.b_force & m.b_clean) and np.any(m.b_force & ~m.b_clean)
    on_axis = (m.r == 0) & (m.mi == 1)
    off_axis = (m.r == 0) & (m.mi == 60)
    assert m.force[on_axis].all() and not m.force[off_axis].any() and m.key[on_axis][0] == m.key[off_axis][0]
    assert np.all(m.word[m.force] >> 11 == 0)                                  # a marker entry carries angle field 0
    assert np.all(m.uv[on_axis] & 0x7FFFFFFF == 0)                             # uy = uz = 0
    twins = np.isin(m.r, (5, 61, 62)) & np.isin(m.mi, (5, 61, 62))
    assert twins.sum() == 6 and m.force[twins].all()


def test_growth_cloud_outgrows_the_first_table(built_lib, oracle, ppf):
    p, nr, d, m, u = ref("growth", oracle, ppf)
    assert m.n_slices == 1 and m.n_unique[0] > 32768 and m.cap > 1 << 16
    assert m.cap // 2 >= m.n_unique[0] > m.cap // 4
    assert u.ucap >= 4 * u.n_ids > u.ucap // 2


def test_far_clouds_pass_the_key_map_and_the_reach_bitset(built_lib, oracle, ppf):
    p, nr, d, m, u = ref("far_beyond_the_key_map", oracle, ppf)
    k = bins_of_pairs(p, d)
    assert 2048 + 100 < k[0, 2] < 16384 - 100 and k[0, 1] < 10
    assert u.top > 2048 and u.kmap_bins == 2048 and u.reach_words == (u.top + 31) // 32 > 64
    assert abs(u.top - 1 - k[0, 2]) < 2 or abs(u.top - 1 - k[1, 2]) < 2        # the top bit is the far pair's own bin
    p, nr, d, m, u = ref("far_beyond_reach", oracle, ppf)
    k = bins_of_pairs(p, d)
    assert k[0, 2] > 16384 + 100 and k[1, 2] > 16384 + 100 and k[0, 1] < 10
    assert len(m.key) == 6 and u.n_ids == 6                                    # the far pairs are in the tables all the same
    assert u.top < 10 and u.kmap_bins == u.top and u.reach.shape == (512,) and u.reach_words == 1


def test_group_union_exceeds_either_member(built_lib, oracle, ppf):
    _, _, d, ma, ua = ref("small", oracle, ppf)
    _, _, d2, mb, ub = ref("small_other", oracle, ppf)
    g = R.Union([ma, mb], d)
    assert d == d2 and g.n_ids > max(ua.n_ids, ub.n_ids) and g.n_ids < ua.n_ids + ub.n_ids   # partly shared keys
    shared = np.intersect1d(ma.ukeys, mb.ukeys)
    k = shared[0]
    assert g.weights[np.searchsorted(g.keys, k)] == (ma.key == k).sum() + (mb.key == k).sum()
    assert g.ucap == R.union_cap(ma.num_model_keys + mb.num_model_keys)
    assert not np.array_equal(g.rank[np.searchsorted(g.keys, ma.ukeys)], ua.rank)   # the group numbers its keys anew


# ---------------------------------------------------------------- hold() on a build made in numpy
VARIANTS = {"exact": {}, "fast": dict(fast=True), "no_spread": dict(spread=False), "slot_order": dict(vote_order=1)}


@pytest.mark.parametrize("name,variant", [(n, v) for n in SMALL for v in sorted(VARIANTS)] + [("points_1024", "exact")])
def test_simulated_build_holds(built_lib, oracle, ppf, name, variant):
    p, nr, d, m, u = ref(name, oracle, ppf)
    R.hold(R.simulate(m, u, seed=5, **VARIANTS[variant]), m, u, **VARIANTS[variant])


def test_simulated_group_holds(built_lib, oracle, ppf):
    _, _, d, ma, _ = ref("small", oracle, ppf)
    _, _, _, mb, _ = ref("small_other", oracle, ppf)
    g = R.Union([ma, mb], d)
    R.hold(R.simulate(ma, g, seed=6), ma, g)
    R.hold(R.simulate(mb, g, seed=7), mb, g)


def _bucket(T, min_len):
    flat = T["slots"].reshape(-1, 4)
    j = np.nonzero((flat[:, 0] != 0) & (flat[:, 2] >= min_len))[0][0]
    return j, int(flat[j, 1]), int(flat[j, 2])


def _swap(a, i, j):
    a[i], a[j] = a[j].copy(), a[i].copy()


def _mutations():
    def dealt_wrong(T):
        j, a, n = _bucket(T, 8)
        k = R.B.spread_key(T["e4"][a:a + n])
        i = int(np.nonzero(k != k[0])[0][0])
        for x in ("e4", "mi"):
            _swap(T[x], a, a + i)

    def entry_twice(T):
        j, a, n = _bucket(T, 2)
        T["e4"][a + 1], T["mi"][a + 1] = T["e4"][a], T["mi"][a]

    def directory_off_by_one(T):
        j, a, n = _bucket(T, 8)
        T["pdir"][a + 1] += 1

    def second_order_unstable(T):
        j, a, n = _bucket(T, 8)
        _swap(T["pw"], a, a + n - 1)

    def puv_of_another_entry(T):
        j, a, n = _bucket(T, 2)
        _swap(T["puv"], a, a + 1)

    def marker_flag_lost(T):
        flat = T["slots"].reshape(-1, 4)
        flat[np.nonzero(flat[:, 3] & R.MARK)[0][0], 3] &= 0x7FFFFFFF

    def marker_flag_lost_in_uinfo(T):
        ui = T["uinfo"].reshape(-1, 2)
        ui[np.nonzero(ui[:, 1] & R.MARK)[0][0], 1] &= 0x7FFFFFFF

    def padding_word_written(T):
        j, a, n = _bucket(T, 1)
        assert n % 4
        T["e4"][a + n] = 0

    def word_behind_the_arrays(T):
        T["e4"][-1] = 0

    def uinfo_stride_padding_written(T):
        assert T["n_ids"] % 64
        T["uinfo"][0, -1, 1] = 1

    def key_behind_an_empty_slot(T):
        s = T["slots"][0]
        j = int(np.nonzero(s[:, 0])[0][0])
        e = np.nonzero(s[:, 0] == 0)[0]
        to = int(e[e > j + 1][1])                                              # two empty slots further on: one stays between
        s[to, [0, 2, 3]], s[j, [0, 2, 3]] = s[j, [0, 2, 3]].copy(), 0

    def weight_short(T):
        T["weights"][np.nonzero(T["ukeys"])[0][0]] -= 1

    def numbers_swapped(T):
        o = np.nonzero(T["ukeys"])[0]
        _swap(T["uids"], o[0], o[1])

    def reach_bit_extra(T):
        T["reach"][511] |= 1 << 31

    def kmap_none_for_a_key(T):
        at = np.argwhere(T["kmap"] != R.KMAP_NONE)[0]
        T["kmap"][at[0], at[1]] = R.KMAP_NONE

    def cap_not_grown(T):
        T["cap"] //= 2

    return [v for k, v in sorted(locals().items()) if callable(v)]


@pytest.mark.parametrize("mutate", _mutations(), ids=lambda f: f.__name__)
def test_hold_refuses_tables_wrong_in_one_place(built_lib, oracle, ppf, mutate):
    p, nr, d, m, u = ref("markers", oracle, ppf)
    if mutate.__name__ in ("dealt_wrong", "directory_off_by_one", "second_order_unstable"):
        p, nr, d, m, u = ref("small", oracle, ppf)                             # buckets of eight entries and more
    T = R.simulate(m, u, seed=9)
    R.hold(T, m, u)
    mutate(T)
    with pytest.raises(AssertionError):
        R.hold(T, m, u)


# ---------------------------------------------------------------- the tap's argument checks
def test_tables_tap_rejects_null_before_touching_a_device(built_lib, ppf):
    L = ppf.lib()
    info = ppf.ModelTables()
    import ctypes as C
    assert L.oslam_model_tables_tap(None, C.byref(info), *([None] * 12)) == ppf.OSLAM_E_INVALID
    assert b"NULL" in L.oslam_last_error()
