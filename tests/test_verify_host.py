"""CPU: the verification stage's yardstick, its calibration and its arguments (include/oslam.h at oslam_verify).

Calibration (verify_calib.table): a 10-model database (synthetic models 0..9, 1500 points voxel-gridded at d_dist),
seeded 640x480 depth frames of model 0 at random rotations in front of a wall at 9 m, every other frame partly covered
by a non-member object; every member's voting pose from the oracle (df 4), refined by tests/refine_ref.py, scored by
tests/view_ref.py.  Measured on the CPU when the defaults were set (absent: the largest value over the nine absent
members, each column on its own):

    frame  occluder   present: supported  view_fitness  coverage  (refine fitness)   absent: supported  vf     coverage
    0      no                  164        0.994         0.732     (0.262)                    144        0.762  0.495
    1      yes                 177        0.983         0.766     (0.266)                    141        0.753  0.478
    2      no                  156        1.000         0.817     (0.221)                    142        0.743  0.454
    3      yes                 116        0.935         0.509     (0.152)                    143        0.899  0.474
    4      no                  144        0.954         0.682     (0.193)                    143        0.753  0.493
    5      yes                 128        1.000         0.520     (0.195)                    143        0.762  0.481

view_fitness separates (present >= 0.935, absent <= 0.899): min_view_fitness 0.92.  Coverage separates narrowly
(present >= 0.509, absent <= 0.495): min_coverage 0.5.  The supported count does not separate (present 116-177, absent
up to 144): min_supported 50 is a floor against a few chance agreements, not a separator.  The refine fitness of the
present model (0.152-0.266) stays below refine's own threshold of 0.3 on every frame.  The test runs frames 0-3 (one
to two minutes); frames 4 and 5 come from the same seeded sequence, run with 6 frames.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_calib  # noqa: E402
import view_ref as V  # noqa: E402

# the known-answer frame: a wall farther away than the calibration's, so that a model moved two extents toward the
# camera stays in front of it
KCAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=30.0)
WALL = 20.0


@pytest.fixture(scope="module")
def known(synth):
    """(model points, normals, d_dist, extent, ground-truth pose, uint16 image): model 0 at 10.5 m before a wall."""
    mp, mn = synth.make_model(0, 1500)
    d = synth.d_dist_for(mp, 0.05)
    ext = synth.bbox_extent(mp)
    dense, _ = synth.make_model(0, 200000)
    rng = synth.SplitMix64(77)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth.random_rotation(rng)
    T[:3, 3] = [0.3, -0.2, 10.5]
    img = synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=WALL, splat=1)
    return mp, mn, d, ext, T, img


def moved(T, dx=0.0, dy=0.0, dz=0.0):
    T = T.copy()
    T[:3, 3] += np.float32([dx, dy, dz])
    return T


def check_invariants(mp, mn, T, cls):
    assert len(cls) == len(mp) and cls.max() <= V.UNKNOWN
    q, m = V.refine_ref.transform_f32(T, mp, mn)
    dot = (m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2]
    assert np.array_equal(cls == V.BACK, dot >= 0)
    r = V.scores(cls)
    assert sum(r[k] for k in V.NAMES) == len(mp)


def test_calibration_separates_present_from_absent(oracle, synth):
    rows = verify_calib.table(synth, oracle, n_frames=4)
    p = V.default_params()
    present = [r["present"] for r in rows]
    assert all(x["rot_err"] < 5.0 for x in present), [x["rot_err"] for x in present]
    assert min(x["view_fitness"] for x in present) >= p["min_view_fitness"] > max(r["absent"]["view_fitness"] for r in rows)
    assert min(x["coverage"] for x in present) >= p["min_coverage"] > max(r["absent"]["coverage"] for r in rows)
    assert min(x["supported"] for x in present) >= p["min_supported"]
    assert all(x["found"] for x in present)
    assert not any(r["absent"]["view_fitness"] >= p["min_view_fitness"] and r["absent"]["coverage"] >= p["min_coverage"]
                   for r in rows)


def test_ground_truth_pose_is_found(known):
    mp, mn, d, ext, T, img = known
    r, cls = V.verify(mp, mn, T, img, KCAM, d)
    check_invariants(mp, mn, T, cls)
    assert r["view_fitness"] >= 0.9 and r["coverage"] >= 0.6 and r["found"], r
    assert r["out"] == 0 and r["unknown"] == 0, r


def test_model_moved_toward_the_camera_conflicts(known):
    mp, mn, d, ext, T, img = known
    Tm = moved(T, dz=-2.0 * ext)
    assert Tm[2, 3] > 2.0
    r, cls = V.verify(mp, mn, Tm, img, KCAM, d)
    check_invariants(mp, mn, Tm, cls)
    facing = len(mp) - r["back"]
    # the projection grows past the image: what stays in it lies in front of everything the camera saw
    assert r["conflict"] == facing - r["out"] and r["conflict"] > r["out"] and not r["found"], r


def test_model_behind_the_wall_is_occluded(known):
    mp, mn, d, ext, T, img = known
    Tm = moved(T, dz=WALL + ext - T[2, 3])
    r, cls = V.verify(mp, mn, Tm, img, KCAM, d)
    check_invariants(mp, mn, Tm, cls)
    assert r["occluded"] == len(mp) - r["back"] and r["coverage"] == 0.0 and not r["found"], r


def test_model_outside_the_frustum_is_out(known):
    mp, mn, d, ext, T, img = known
    for Tm in (moved(T, dx=50.0), moved(T, dy=-40.0), moved(T, dz=40.0), moved(T, dz=-20.0)):
        r, cls = V.verify(mp, mn, Tm, img, KCAM, d)
        check_invariants(mp, mn, Tm, cls)
        assert r["out"] == len(mp) - r["back"] and r["out"] > 0 and not r["found"], r


def test_counts_and_back_rule_at_any_pose(known, synth):
    mp, mn, d, ext, T, img = known
    rng = synth.SplitMix64(5)
    z = V.view_z(img, KCAM["depth_scale"], KCAM["z_min"], KCAM["z_max"])
    for k in range(12):
        Tm = np.eye(4, dtype=np.float32)
        Tm[:3, :3] = synth.random_rotation(rng)
        Tm[:3, 3] = (rng.uniform(3) - 0.5) * np.array([6.0, 5.0, 20.0]) + np.array([0, 0, 9.0])
        for window in range(4):
            cls = V.classify(mp, mn, Tm, z, KCAM["fx"], KCAM["fy"], KCAM["cx"], KCAM["cy"], KCAM["z_min"], KCAM["z_max"],
                             V.tolerance(1.0, d), window)
            check_invariants(mp, mn, Tm, cls)


def test_window_rule_by_hand():
    """One point on a 5x5 image: the window decides between supported, occluded, conflict and unknown."""
    z = np.zeros((5, 5), np.float32)
    mp = np.float32([[0.0, 0.0, 4.0]])
    mn = np.float32([[0.0, 0.0, -1.0]])
    T = np.eye(4, dtype=np.float32)
    cam = (1.0, 1.0, 2.0, 2.0, 0.5, 10.0)           # fx fy cx cy z_min z_max: the point lands on pixel (2, 2)

    def cls(window=1, tol=0.1):
        return int(V.classify(mp, mn, T, z, *cam, tol, window)[0])
    assert cls() == V.UNKNOWN
    z[0, 0] = 9.0                                    # farther, outside the 3x3 window
    assert cls() == V.UNKNOWN and cls(window=2) == V.CONFLICT
    z[1, 3] = 9.0
    assert cls() == V.CONFLICT
    z[3, 1] = 2.0                                    # nearer
    assert cls() == V.OCCLUDED
    z[2, 3] = 4.1                                    # within tol: |4.1f - 4.0f| <= 0.11f
    assert cls(tol=0.11) == V.SUPPORTED and cls(window=0) == V.UNKNOWN
    assert int(V.classify(mp, -mn, T, z, *cam, 0.1, 1)[0]) == V.BACK
    assert int(V.classify(mp + np.float32([0, 0, 20]), mn, T, z, *cam, 0.1, 1)[0]) == V.OUT


def test_verify_params_default(built_lib, ppf):
    p = ppf.default_verify_params()
    want = V.default_params()
    assert p.depth_tol == np.float32(want["depth_tol"]) and p.window == want["window"]
    assert p.min_view_fitness == np.float32(want["min_view_fitness"]) and p.min_coverage == np.float32(want["min_coverage"])
    assert p.min_supported == want["min_supported"] and list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_verify_params(window=3).window == 3
    with pytest.raises(TypeError):
        ppf.default_verify_params(no_such_field=1)


def test_verify_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: stand-in handles (zeroed host
    memory) are never looked at, on a machine with or without a GPU."""
    L = ppf.lib()
    fake_m, fake_v, fake_db = C.create_string_buffer(4096), C.create_string_buffer(4096), C.create_string_buffer(4096)
    m, v, db = C.cast(fake_m, C.c_void_p), C.cast(fake_v, C.c_void_p), C.cast(fake_db, C.c_void_p)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    res = ppf.VerifyResult()
    cls = np.zeros(8, np.uint8)

    def call(T=eye, params=None, mm=m, vv=v, r=True):
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        p = params if params is not None else ppf.default_verify_params()
        return L.oslam_verify(mm, vv, ppf._p(T), C.byref(p), C.byref(res) if r else None)

    assert call(mm=None) == ppf.OSLAM_E_INVALID
    assert call(vv=None) == ppf.OSLAM_E_INVALID
    assert call(r=False) == ppf.OSLAM_E_INVALID
    assert L.oslam_verify(m, v, None, None, C.byref(res)) == ppf.OSLAM_E_INVALID
    bad_T = []
    T = eye.copy(); T[3] = np.nan; bad_T.append(T)
    T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad_T.append(T)
    T = eye.copy(); T[0] = -1; bad_T.append(T)
    T = eye.copy(); T[13] = 0.5; bad_T.append(T)
    bad_T.append(np.zeros(16, np.float32))           # a single call has no "skipped"
    for T in bad_T:
        assert call(T) == ppf.OSLAM_E_INVALID, T
    bad_p = [dict(depth_tol=0.0), dict(depth_tol=-1.0), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
             dict(window=4), dict(min_view_fitness=1.5), dict(min_view_fitness=-0.1), dict(min_coverage=1.01),
             dict(min_coverage=float("nan"))]
    for kw in bad_p:
        p = ppf.default_verify_params(**kw)
        assert call(params=p) == ppf.OSLAM_E_INVALID, kw
        assert L.oslam_verify_classes(m, v, ppf._p(eye), C.byref(p), ppf._p(cls)) == ppf.OSLAM_E_INVALID, kw
        Tn = np.zeros((2, 16), np.float32)
        res2 = (ppf.VerifyResult * 2)()
        assert L.oslam_db_verify(db, v, ppf._p(Tn), C.byref(p), res2) == ppf.OSLAM_E_INVALID, kw
    assert L.oslam_verify_classes(m, v, ppf._p(eye), None, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_verify_classes(None, v, ppf._p(eye), None, ppf._p(cls)) == ppf.OSLAM_E_INVALID
    assert L.oslam_verify_classes(m, v, ppf._p(bad_T[1]), None, ppf._p(cls)) == ppf.OSLAM_E_INVALID
    Tn = np.zeros((2, 16), np.float32)
    res2 = (ppf.VerifyResult * 2)()
    assert L.oslam_db_verify(None, v, ppf._p(Tn), None, res2) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_verify(db, None, ppf._p(Tn), None, res2) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_verify(db, v, None, None, res2) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_verify(db, v, ppf._p(Tn), None, None) == ppf.OSLAM_E_INVALID
    # the view: bad image or camera arguments are refused before any device call
    img = np.zeros((4, 4), np.uint16)
    h = C.c_void_p(0)
    good = ppf.Camera(525.0, 525.0, 2.0, 2.0, 0.001, 0.5, 10.0, 0.05)
    assert L.oslam_view_create(None, 1, 4, 4, C.byref(good), 0, C.byref(h)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_create(ppf._p(img), 1, 0, 4, C.byref(good), 0, C.byref(h)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_create(ppf._p(img), 1, 4, 4, None, 0, C.byref(h)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_create(ppf._p(img), 1, 4, 4, C.byref(good), 0, None) == ppf.OSLAM_E_INVALID
    for cam in (ppf.Camera(0.0, 525.0, 2.0, 2.0, 0.001, 0.5, 10.0, 0.05), ppf.Camera(525.0, 525.0, 2.0, 2.0, 0.0, 0.5, 10.0, 0.05),
                ppf.Camera(525.0, 525.0, 2.0, 2.0, 0.001, 0.0, 10.0, 0.05), ppf.Camera(525.0, 525.0, 2.0, 2.0, 0.001, 5.0, 1.0, 0.05),
                ppf.Camera(525.0, 525.0, float("nan"), 2.0, 0.001, 0.5, 10.0, 0.05)):
        assert L.oslam_view_create(ppf._p(img), 1, 4, 4, C.byref(cam), 0, C.byref(h)) == ppf.OSLAM_E_INVALID
    assert not h.value
    assert L.oslam_view_destroy(None) == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(call(params=ppf.default_verify_params(window=7)))
    assert e.value.code == ppf.OSLAM_E_INVALID and "window" in str(e.value)
