"""CPU: the instance selection rule of include/oslam.h (oslam_select_instances) against its numpy restatement
(tests/instances_ref.py) on seeded candidate sets, its argument checks, and on the golden fixtures' cells: the host
pose stage (default clustering) followed by the selection gives the registration's pose as instance 0.  The greedy
clustering's candidates are only reachable through oslam_align_instances: tests/test_gpu_instances.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import instances_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def random_set(rng, n, n_centres=4, spread=0.3, score_levels=6):
    """poses around a few centres (several per object, some far), scores from few levels (many ties)"""
    centres = rng.uniform(-3, 3, size=(n_centres, 3))
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        T[i, :3, :3] = rotation(rng)
        T[i, :3, 3] = centres[rng.integers(n_centres)] + rng.normal(scale=spread, size=3)
        T[i, 3, 3] = 1
    scores = (1 + rng.integers(score_levels, size=n) * 3).astype(np.float32)
    return T, scores


def both(ppf, T, scores, c, ext, **kw):
    got = ppf.select_instances(T, scores, c, ext, params=ppf.default_instance_params(**kw))
    want = R.select(T, scores, c, ext, **kw)
    assert np.array_equal(got, want), (kw, got, want)
    return got


def test_defaults(ppf, built_lib):
    p = ppf.default_instance_params()
    assert (p.max_instances, p.min_separation, p.min_score_ratio, p.keep_not_found) == (8, F(0.5), F(0.5), 0)
    assert p.max_angle == F(math.pi)


@pytest.mark.parametrize("seed", range(6))
def test_random_sets_equal_the_restatement(ppf, built_lib, seed):
    rng = np.random.default_rng(100 + seed)
    c = rng.normal(size=3).astype(np.float32)
    ext = F(rng.uniform(0.5, 2.0))
    T, scores = random_set(rng, int(rng.integers(20, 400)))
    seen = set()
    for kw in (dict(), dict(max_instances=64, min_score_ratio=0.0), dict(max_instances=3),
               dict(min_separation=0.05, max_instances=64, min_score_ratio=0.2),
               dict(max_angle=0.5, max_instances=64, min_score_ratio=0.0),
               dict(max_angle=2.0, min_separation=1.5, max_instances=20), dict(min_separation=0.0, max_instances=64),
               dict(min_score_ratio=1.0, max_instances=64)):
        got = both(ppf, T, scores, c, ext, **kw)
        seen.add(len(got))
    assert len(seen) >= 3                 # the parameters matter on these sets


def test_equal_scores_lower_index_wins(ppf, built_lib):
    T = np.tile(np.eye(4, dtype=np.float32), (5, 1, 1))
    T[:, 0, 3] = [0, 10, 0, 10, 20]      # 0 and 2 coincide, 1 and 3 coincide
    scores = np.full(5, 7, np.float32)
    got = both(ppf, T, scores, np.zeros(3, np.float32), F(1), max_instances=8, min_score_ratio=0.0)
    assert list(got) == [0, 1, 4]
    scores[3] = 8
    got = both(ppf, T, scores, np.zeros(3, np.float32), F(1), max_instances=8, min_score_ratio=0.0)
    assert list(got) == [3, 0, 4]


def test_centroid_distance_on_either_side_of_the_threshold(ppf, built_lib):
    ext = F(1)
    sep2, _, _ = R.thresholds(0.5, math.pi, ext)
    assert sep2 == F(0.25)
    c = np.array([0.0, -0.5, 1.0], np.float32)
    for dx, same in ((F(0.5), False), (np.nextafter(F(0.5), F(0)), True), (F(0.75), False)):
        T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
        T[1, 0, 3] = dx
        p0, p1 = R.transformed_centroid(T[0], c), R.transformed_centroid(T[1], c)
        d2 = F(F(F((p1[0] - p0[0]) ** 2) + F((p1[1] - p0[1]) ** 2)) + F((p1[2] - p0[2]) ** 2))
        assert (d2 < sep2) == same
        got = both(ppf, T, np.array([5, 4], np.float32), c, ext, min_score_ratio=0.0)
        assert len(got) == (1 if same else 2)


def test_rotation_sum_on_either_side_of_the_threshold(ppf, built_lib):
    for max_angle in (0.2, 1.0, 2.5):
        _, cos_thr, rot_on = R.thresholds(0.5, max_angle, F(1))
        assert rot_on
        sums = []
        for v in (np.nextafter(cos_thr, F(-4)), cos_thr, np.nextafter(cos_thr, F(4))):
            T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
            T[1, :3, :3] = np.diag([v, 0, 0])       # not a rotation: the rule only reads the sum, v here
            sums.append(R.rotation_sum(T[0], T[1]))
            got = both(ppf, T, np.array([5, 4], np.float32), np.zeros(3, np.float32), F(1), max_angle=max_angle,
                       min_score_ratio=0.0)
            assert len(got) == (1 if sums[-1] >= cos_thr else 2)
        assert sums[0] < cos_thr == sums[1] < sums[2], (max_angle, sums, cos_thr)


def test_max_angle_pi_is_translation_only(ppf, built_lib):
    T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    T[1, :3, :3] = np.diag([-1, -1, 1]).astype(np.float32)      # 180 degrees apart, same place
    got = both(ppf, T, np.array([5, 4], np.float32), np.zeros(3, np.float32), F(1), min_score_ratio=0.0)
    assert list(got) == [0]
    got = both(ppf, T, np.array([5, 4], np.float32), np.zeros(3, np.float32), F(1), min_score_ratio=0.0,
               max_angle=3.1)
    assert list(got) == [0, 1]


def test_score_floor_and_cap(ppf, built_lib):
    T = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    T[:, 0, 3] = np.arange(6) * 10
    scores = np.array([10, 9, 5, 4.9999995, 8, 7], np.float32)
    assert list(both(ppf, T, scores, np.zeros(3, np.float32), F(1))) == [0, 1, 4, 5, 2]
    assert list(both(ppf, T, scores, np.zeros(3, np.float32), F(1), min_score_ratio=0.8)) == [0, 1, 4]
    assert list(both(ppf, T, scores, np.zeros(3, np.float32), F(1), max_instances=2)) == [0, 1]
    assert list(both(ppf, T, scores, np.zeros(3, np.float32), F(1), max_instances=1, min_score_ratio=0.0)) == [0]


def test_empty_and_single(ppf, built_lib):
    c = np.zeros(3, np.float32)
    assert len(ppf.select_instances(np.zeros((0, 4, 4), np.float32), np.zeros(0, np.float32), c, F(1))) == 0
    assert list(both(ppf, np.eye(4, dtype=np.float32)[None], np.array([3], np.float32), c, F(1))) == [0]


def test_invalid_arguments(ppf, built_lib):
    T = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    s = np.ones(3, np.float32)
    c = np.zeros(3, np.float32)
    bad = [dict(max_instances=0), dict(max_instances=65), dict(min_separation=float("nan")),
           dict(min_separation=float("inf")), dict(min_separation=-0.1), dict(max_angle=-0.01),
           dict(max_angle=3.2), dict(max_angle=float("nan")), dict(min_score_ratio=-0.01),
           dict(min_score_ratio=1.01), dict(min_score_ratio=float("nan"))]
    for kw in bad:
        with pytest.raises(ppf.OslamError) as e:
            ppf.select_instances(T, s, c, F(1), params=ppf.default_instance_params(**kw))
        assert e.value.code == ppf.OSLAM_E_INVALID, kw
    for ext in (F("nan"), F(-1), F("inf")):
        with pytest.raises(ppf.OslamError):
            ppf.select_instances(T, s, c, ext)
    with pytest.raises(ppf.OslamError):
        ppf.select_instances(T, s, c, F(1), params=ppf.default_instance_params(max_instances=4), cap=3)
    ppf.select_instances(T, s, c, F(1), params=ppf.default_instance_params(max_angle=math.pi, max_instances=64))
    L, ip = ppf.lib(), ppf.default_instance_params()
    idx = np.zeros(8, np.uint32)
    n = C.c_size_t(0)
    args = [ppf._p(T), ppf._p(s), 3, ppf._p(c), 1.0, C.byref(ip), ppf._p(idx), 8, C.byref(n)]
    for k in (0, 1, 3, 5, 6, 8):
        a = list(args)
        a[k] = None
        assert L.oslam_select_instances(*a) == ppf.OSLAM_E_INVALID, k
    assert L.oslam_select_instances(*args) == ppf.OSLAM_OK and n.value == 1
    # the entry points check their instance parameters before any handle is read
    out = (ppf.Instance * 8)()
    for kw in bad:
        p = ppf.default_instance_params(**kw)
        assert L.oslam_align_instances(C.c_void_p(1), C.c_void_p(1), C.byref(p), None, out, 8, C.byref(n), None) == ppf.OSLAM_E_INVALID
        assert L.oslam_db_align_instances(C.c_void_p(1), C.c_void_p(1), C.byref(p), None, out, 8, ppf._p(idx), None) == ppf.OSLAM_E_INVALID
    p = ppf.default_instance_params()
    assert L.oslam_align_instances(C.c_void_p(1), C.c_void_p(1), C.byref(p), None, out, 7, C.byref(n), None) == ppf.OSLAM_E_INVALID
    assert L.oslam_align_instances(None, C.c_void_p(1), C.byref(p), None, out, 8, C.byref(n), None) == ppf.OSLAM_E_INVALID
    rp = ppf.default_refine_params(inlier_dist=3.0)
    assert L.oslam_align_instances(C.c_void_p(1), C.c_void_p(1), C.byref(p), C.byref(rp), out, 8, C.byref(n), None) == ppf.OSLAM_E_INVALID


@pytest.mark.parametrize("name", ["case_m64_s128.npz", "case_m200_s400_df3.npz"])
def test_golden_cells_give_the_registration_pose_as_instance_0(ppf, built_lib, name):
    g = np.load(os.path.join(GOLDEN, name))
    cells = np.zeros(len(g["cell_code"]), ppf.CELL_DTYPE)
    cells["code"], cells["count"] = g["cell_code"], g["cell_count"]
    n = len(cells)
    mp, mn, sp, sn = (np.ascontiguousarray(g[k], np.float32) for k in ("mp", "mn", "sp", "sn"))
    T = np.zeros(16, np.float32)
    poses = np.zeros((n, 16), np.float32)
    tr, ro, sc = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    best = C.c_uint32(0)
    assert ppf.lib().oslam_pose_stage_ex(ppf._p(cells), n, ppf._p(mp), ppf._p(mn), len(mp), ppf._p(sp), ppf._p(sn),
                                         len(sp), float(g["d_dist"]), 0, 0, 0, None, ppf._p(T), ppf._p(poses), ppf._p(tr),
                                         ppf._p(ro), ppf._p(sc), C.byref(best)) == 0
    cand = R.default_candidates(poses, tr)
    c, ext = R.centroid(mp), R.extent(mp)
    for kw in (dict(), dict(max_instances=64, min_score_ratio=0.0, min_separation=0.1)):
        got = both(ppf, cand, sc, c, ext, **kw)
        assert got[0] == best.value
        assert np.array_equal(cand[got[0]].reshape(16), T)
        # the fixture's default-clustering pose was written on another host (libm sinf/cosf: last-bit tolerance, as
        # tests/test_gpu_parity.py compares it)
        np.testing.assert_allclose(cand[got[0]], g["T_gpu"], rtol=0, atol=2e-5)
