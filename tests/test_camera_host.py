"""CPU: the camera motion stage's yardstick, its calibration, the tracker's camera arithmetic on the host and the
arguments (include/oslam.h at oslam_view_egomotion and oslam_tracker_step_cam).

The world (tests/camera_ref.py make_world): a floor, a back wall at 6.0 m (+ 0.4 m per seed), a side wall and three synth
objects of about 1.2 m, rendered at 640x480 from a camera that turns 3 degrees per frame about a tilted axis near the
vertical and moves 3 cm per frame along a seeded direction, 10 frames, seeds 0, 1, 2.  Measured with the restatement
(float64 sums) on the CPU when the defaults were set, src = frame f - 1 and dst = frame f from the identity; "chained" is
the product of the frame-to-frame results against the true pose of frame f in frame 0:

    seed  frame  rot err (deg)  trans err (m)  chained (deg, m)  correspondences  overlap  iterations  rmse (m)
    0     1      0.0089         0.0008         0.0089  0.0008    279591           0.928    4 2 2       0.0010
    0     5      0.0102         0.0007         0.0482  0.0036    281339           0.932    4 5 3       0.0010
    0     9      0.0123         0.0004         0.0902  0.0057    230992           0.916    4 5 6       0.0014
    1     1      0.0105         0.0007         0.0105  0.0007    280345           0.932    4 2 2       0.0011
    1     5      0.0108         0.0007         0.0538  0.0032    281800           0.935    4 5 2       0.0011
    1     9      0.0117         0.0004         0.0970  0.0051    229331           0.921    4 5 2       0.0015
    2     1      0.0070         0.0008         0.0070  0.0008    277821           0.923    4 5 2       0.0012
    2     5      0.0068         0.0007         0.0325  0.0038    273521           0.908    4 2 1       0.0015
    2     9      0.0107         0.0007         0.0620  0.0064    251860           0.832    4 2 2       0.0018

Over all 27 pairs: rotation <= 0.0123 degrees, translation <= 0.0008 m, chained <= 0.0970 degrees and 0.0064 m, every
level ended by its convergence test but the first (4 iterations), condition number of J^T J 1.2e2 .. 3.8e3.  Started
from the truth, the first step of every level moves the pose by 0.007 .. 0.011 degrees and 0.8 mm: the rule's own
fixed point lies that far from the truth (depth in millimetres, one-pixel splats).

Bounds asserted here and by tests/test_gpu_camera.py on the same frames (camera_ref.ROT_BOUND and so on): the largest
measured value over the three seeds times 3.  The seeds differ by up to a factor of 1.6 among themselves (largest
frame-to-frame errors per seed: rotation 0.0123 / 0.0120 / 0.0107 degrees, chained 0.090 / 0.097 / 0.062 degrees), so a factor of 3 is twice the spread between seeds.

KinFu's gates.  With max_corr_dist = 0.10 m (KinFu's distance gate) the same frames are NOT followed: at 3 degrees per
frame and a mean depth of 5.4 m a point moves 0.28 m between frames, the objects and the side wall, which alone tell a
turn about the vertical from a step sideways, fall outside the gate, and the result slides by 0.22 .. 0.29 m along x
with the rotation right to 0.01 degrees (seed 0, every frame; at 1 degree per frame the same gate gives 0.3 mm).  0.20,
0.30 and 0.50 m all give the table's values, so the default is 0.30 m: the motion of the stream at its mean depth.  The
normal gate is KinFu's cos(20 degrees).  Strides buy time, not reach: the gates are the same at every level.

min_overlap.  Overlap of consecutive frames and of unrelated pairs (a jump of 7 .. 9 frames, 21 .. 27 degrees; frame f of
another world):

    consecutive frames, 27 pairs                      0.832 .. 0.935
    a jump of 7 .. 9 frames, 9 pairs                  0.000 .. 0.672   (translation wrong by 1.1 .. 2.9 m)
    frame f of the next seed's world, 4 pairs         0.274 .. 0.875

The default 0.75 lies in the gap between consecutive frames (asserted >= 0.80) and far jumps (asserted <= 0.70).  It
does NOT tell a similar room apart: the next seed's world has the same floor and side wall and a back wall 0.4 m
further, and the alignment slides onto them (0.875 on one pair).  The overlap measures shared surface, not identity;
those four pairs are printed, not asserted.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402

SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def streams(synth):
    out = {}
    for seed in SEEDS:
        world = E.make_world(synth, seed)
        traj = E.trajectory(synth, seed)
        maps = [K.view_maps(E.render(synth, world, T), E.CAM, E.MAX_JUMP) for T in traj]
        out[seed] = dict(traj=traj, maps=maps)
    return out


def test_world_constrains_all_six_degrees_of_freedom(synth, streams):
    """J^T J of the first step (undamped, pivot at the camera) is well conditioned on the world; the back wall alone, the
    named degenerate case, is several times worse.  The bound: the float32 terms carry a relative error of about 6e-8 and the condition number multiplies
    it, so below 1e5 the step is right to better than 1 %; rotations and translations differ by the square of the scene's
    depth (about 30), which a well constrained world cannot avoid."""
    worst = 0.0
    for seed in SEEDS:
        s = streams[seed]
        _, r = E.egomotion(s["maps"][0], s["maps"][1], E.CAM, levels=[(4, 1)])
        print("seed %d: condition number of J^T J at the first step %.3e" % (seed, r["cond"]))
        assert r["cond"] < 1e5, (seed, r["cond"])
        worst = max(worst, r["cond"])
    wall = E.make_world(synth, 0, one_plane=True)
    traj = streams[0]["traj"]
    maps = [K.view_maps(E.render(synth, wall, T), E.CAM, E.MAX_JUMP) for T in traj[:2]]
    T, r = E.egomotion(maps[0], maps[1], E.CAM, levels=[(4, 1)])
    print("one plane: condition number %.3e" % r["cond"])
    # measured 1.9e4 against 2.1e3 .. 3.8e3: the normals of a wall in millimetre depth steps scatter by degrees, which
    # fills the three sliding directions with noise; the one plane is still the worst conditioned of all
    assert r["cond"] > 4.0 * worst, (r["cond"], worst)


def test_restatement_follows_the_moving_camera(streams):
    worst = {}
    for seed in SEEDS:
        s = streams[seed]
        chain = np.eye(4)
        w = [0.0, 0.0, 0.0, 0.0]
        for f in range(1, len(s["traj"])):
            G = E.truth(s["traj"][f - 1], s["traj"][f])
            T, r = E.egomotion(s["maps"][f - 1], s["maps"][f], E.CAM)
            rot, tr = refine_ref.pose_error(T, G)
            chain = T.astype(np.float64) @ chain
            crot, ctr = refine_ref.pose_error(chain, E.truth(s["traj"][0], s["traj"][f]))
            print("seed %d frame %d  rot %.4f deg  trans %.4f m  chained %.4f deg %.4f m  corr %d  overlap %.3f  it %s  "
                  "rmse %.4f  conv %d" % (seed, f, rot, tr, crot, ctr, r["correspondences"], r["overlap"], r["iterations"],
                                          r["rmse"], r["converged"]))
            assert rot < E.ROT_BOUND and tr < E.TRANS_BOUND, (seed, f, rot, tr)
            assert crot < E.CHAIN_ROT_BOUND and ctr < E.CHAIN_TRANS_BOUND, (seed, f, crot, ctr)
            assert r["ok"] and r["overlap"] >= E.OVERLAP_CONSECUTIVE_MIN
            w = [max(a, b) for a, b in zip(w, (rot, tr, crot, ctr))]
        worst[seed] = w
    print("largest per seed (rot, trans, chained rot, chained trans):", worst)


def test_overlap_separates_consecutive_from_unrelated(streams):
    lo = []
    for seed in SEEDS:
        s = streams[seed]
        for a, b in ((0, 9), (9, 0), (1, 8)):
            _, r = E.egomotion(s["maps"][a], s["maps"][b], E.CAM)
            print("seed %d jump %d -> %d: overlap %.3f" % (seed, a, b, r["overlap"]))
            lo.append(r["overlap"])
        other = streams[SEEDS[(SEEDS.index(seed) + 1) % len(SEEDS)]]
        for f in (0, 4):
            _, r = E.egomotion(s["maps"][f], other["maps"][f], E.CAM)
            print("seed %d frame %d against another world: overlap %.3f (not asserted)" % (seed, f, r["overlap"]))
    assert max(lo) <= E.OVERLAP_UNRELATED_MAX, max(lo)
    assert E.OVERLAP_UNRELATED_MAX < E.default_params()["min_overlap"] < E.OVERLAP_CONSECUTIVE_MIN


def test_pinned_sums_are_sums():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 255, 256, 257, 300 * 256 + 17):
        t = rng.standard_normal((n, 3)).astype(np.float32)
        s = E.pinned_sums(t)
        assert np.allclose(s, t.astype(np.float64).sum(axis=0), rtol=0, atol=1e-4 * max(1.0, np.sqrt(n)))
    assert np.array_equal(E.pinned_sums(np.ones((70000, 1), np.float32)), [70000.0])


# ---------------------------------------------------------------- ABI
def test_egomotion_defaults(built_lib, ppf):
    p = ppf.default_egomotion_params()
    want = E.default_params()
    assert p.n_levels == 3 and [(l.stride, l.max_iterations) for l in p.level] == want["levels"] == [(4, 4), (2, 5), (1, 10)]
    assert p.max_corr_dist == np.float32(want["max_corr_dist"]) == np.float32(0.30)
    assert p.min_normal_dot == np.float32(want["min_normal_dot"]) == np.float32(np.cos(np.radians(20.0)))
    assert p.stop_rot == np.float32(1e-5) and p.stop_trans == np.float32(1e-5)
    assert p.min_overlap == np.float32(want["min_overlap"]) and list(p.reserved) == [0, 0, 0, 0]
    q = ppf.default_egomotion_params(levels=[(1, 7)], max_corr_dist=0.1)
    assert q.n_levels == 1 and q.level[0].stride == 1 and q.level[0].max_iterations == 7 and q.max_corr_dist == np.float32(0.1)
    with pytest.raises(TypeError):
        ppf.default_egomotion_params(no_such_field=1)
    assert C.sizeof(ppf.TrackerParams) == TRACKER_PARAMS_SIZE      # oslam_tracker_params keeps its size


TRACKER_PARAMS_SIZE = 316


def test_egomotion_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Every OSLAM_E_INVALID case of oslam_view_egomotion, its tap and oslam_tracker_step_cam, with stand-in handles
    (zeroed host memory: device 0) on a machine with or without a GPU."""
    L = ppf.lib()
    fa, fb = C.create_string_buffer(4096), C.create_string_buffer(4096)
    a, b = C.cast(fa, C.c_void_p), C.cast(fb, C.c_void_p)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    To = np.zeros(16, np.float32)
    pix = np.zeros(4, np.int32)
    res = ppf.EgomotionResult()

    def call(src=a, dst=b, T=eye, params=None, out=To):
        p = params if params is not None else ppf.default_egomotion_params()
        return L.oslam_view_egomotion(src, dst, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None,
                                      C.byref(p), ppf._p(out) if out is not None else None, C.byref(res))

    def tap(src=a, dst=b, T=eye, params=None, out=pix):
        p = params if params is not None else ppf.default_egomotion_params()
        return L.oslam_view_egomotion_correspondences(src, dst, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None
                                                      else None, C.byref(p), ppf._p(out) if out is not None else None)

    assert call(src=None) == call(dst=None) == call(out=None) == ppf.OSLAM_E_INVALID
    assert tap(src=None) == tap(dst=None) == tap(out=None) == tap(T=None) == ppf.OSLAM_E_INVALID
    assert L.oslam_egomotion_params_default(None) == ppf.OSLAM_E_INVALID
    bad_T = []
    T = eye.copy(); T[3] = np.nan; bad_T.append(T)
    T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad_T.append(T)
    T = eye.copy(); T[0] = -1; bad_T.append(T)
    T = eye.copy(); T[13] = 0.5; bad_T.append(T)
    for T in bad_T:
        assert call(T=T) == ppf.OSLAM_E_INVALID and tap(T=T) == ppf.OSLAM_E_INVALID, T
    bad_p = [dict(max_corr_dist=0.0), dict(max_corr_dist=-1.0), dict(max_corr_dist=float("nan")), dict(max_corr_dist=float("inf")),
             dict(min_normal_dot=float("nan")), dict(stop_rot=float("inf")), dict(stop_trans=float("nan")), dict(stop_rot=-1.0),
             dict(min_overlap=float("nan")), dict(min_overlap=1.5), dict(levels=[(0, 1)]), dict(levels=[(17, 1)]),
             dict(levels=[(4, 4), (2, 1001)]), dict(levels=[]), dict(n_levels=4)]
    for kw in bad_p:
        p = ppf.default_egomotion_params(**kw)
        assert call(params=p) == ppf.OSLAM_E_INVALID, kw
        assert tap(params=p) == ppf.OSLAM_E_INVALID, kw
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(call(params=ppf.default_egomotion_params(levels=[(32, 1)])))
    assert e.value.code == ppf.OSLAM_E_INVALID and "stride" in str(e.value)
    # views on different devices: the stand-in destination says device 1
    C.cast(fb, C.POINTER(C.c_int))[0] = 1
    assert call() == ppf.OSLAM_E_INVALID and "different devices" in L.oslam_last_error().decode()
    assert tap() == ppf.OSLAM_E_INVALID
    C.cast(fb, C.POINTER(C.c_int))[0] = 0
    # src == dst: the identity at once, without a device, whatever T_init is
    To[:] = 7
    Ti = np.eye(4, dtype=np.float32)
    Ti[:3, 3] = [1, 2, 3]
    assert call(dst=a, T=Ti.reshape(16)) == ppf.OSLAM_OK
    assert np.array_equal(To, eye) and list(res.iterations) == [0, 0, 0] and res.launches == 0 and res.ok == 1
    assert res.converged == 1 and res.overlap == 1.0
    # oslam_tracker_step_cam
    t = ppf.Tracker.from_shapes(np.float32([[0, 0, 0]]), np.float32([1.0]))
    out = (ppf.TrackState * 4)()
    n = C.c_size_t(0)

    def step(tr=t._h, v=a, T=eye, nn=C.byref(n), o=out):
        return L.oslam_tracker_step_cam(tr, None, v, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None,
                                        o, 4, nn, None)
    assert step(tr=None) == step(v=None) == step(nn=None) == step(o=None) == ppf.OSLAM_E_INVALID
    for T in bad_T:
        assert step(T=T) == ppf.OSLAM_E_INVALID, T
        assert L.oslam_tracker_predict(t._h, ppf._p(T)) == ppf.OSLAM_E_INVALID
    assert step() == ppf.OSLAM_E_INVALID and "shapes" in L.oslam_last_error().decode()   # made from shapes: cannot step
    assert L.oslam_tracker_predict(None, ppf._p(eye)) == L.oslam_tracker_predict(t._h, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_tracker_camera(None, ppf._p(To)) == L.oslam_tracker_camera(t._h, None) == ppf.OSLAM_E_INVALID
    assert np.array_equal(t.camera(), np.eye(4, dtype=np.float32))                      # nothing changed
    t.close()


def test_tracker_camera_arithmetic(built_lib, ppf, synth):
    """Step 0 on the host: every live pose becomes float32(double(T_cam) * double(T)), the camera accumulates
    T_world_cam * T_cam^-1 in double, and the identity changes no bit."""
    t = ppf.Tracker.from_shapes(np.float32([[0.1, 0, 0], [0, 0.2, 0]]), np.float32([2.0, 1.0]))
    rng = synth.SplitMix64(77)
    poses = []
    for k in range(3):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [4.0 * k, -1.0, 5.0 + k]
        poses.append(T)
    poses[2][:3, :3] = np.float32([[1, 0, 0], [0, -0.0, -1], [0, 1, -0.0]])             # negative zeros must survive
    t.update([dict(model=k % 2, T=T) for k, T in enumerate(poses)])
    before = [x["T"].copy() for x in t.tracks()]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, poses))
    after = t.predict(np.eye(4, dtype=np.float32))
    assert all(x["T"].tobytes() == b.tobytes() for x, b in zip(after, before))
    assert np.array_equal(t.camera(), np.eye(4, dtype=np.float32))
    W = np.eye(4)
    cur = [b.copy() for b in before]
    for k in range(12):
        Tc = np.eye(4)
        Tc[:3, :3] = K.axis_rotation((0.2, 1.0, -0.1 * k), 3.0 + k)
        Tc[:3, 3] = [0.03 * k, -0.01, 0.02]
        Tc = Tc.astype(np.float32)
        got = t.predict(Tc)
        D = Tc.astype(np.float64)
        cur = [(D @ c.astype(np.float64)).astype(np.float32) for c in cur]
        for x, c in zip(got, cur):
            assert np.abs(x["T"].astype(np.float64) - c).max() <= 2.0 ** -22 * max(1.0, np.abs(c).max()), k
            assert np.array_equal(x["T"][3], [0, 0, 0, 1])
        Di = np.eye(4)
        Di[:3, :3] = D[:3, :3].T
        Di[:3, 3] = -(D[:3, :3].T @ D[:3, 3])
        W = W @ Di
        cam = t.camera()
        assert np.abs(cam.astype(np.float64) - W).max() <= 2.0 ** -22 * max(1.0, np.abs(W).max()), k
    # a track's world pose stays where it was: T_world_cam * T is the pose of frame 0, to float32 rounding
    for x, b in zip(t.tracks(), before):
        assert np.abs(W @ x["T"].astype(np.float64) - b).max() < 1e-4
    t.close()
