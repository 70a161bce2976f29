"""GPU: the camera motion stage (oslam_view_egomotion, its tap) against the numpy restatement of tests/camera_ref.py and
the ground truth of the moving-camera stream, and the tracker with the camera's motion (oslam_tracker_step_cam)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

DYN = ("launches", "ms_total")
ROT_FLOOR = 0.01                                  # degrees: tests/test_gpu_view_edges.py


def view_of(ppf, img, cam=E.CAM):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=E.MAX_JUMP)


def plain(d):
    """a result dict without the fields that depend on the call"""
    return {k: (plain(v) if isinstance(v, dict) else v) for k, v in d.items() if k not in DYN}


@pytest.fixture(scope="module")
def stream(ppf, synth):
    """Seed 0 of tests/test_camera_host.py: the world, the 10 camera poses, the frames, their restated maps."""
    world = E.make_world(synth, 0)
    traj = E.trajectory(synth, 0)
    imgs = [E.render(synth, world, T) for T in traj]
    maps = [K.view_maps(im, E.CAM, E.MAX_JUMP) for im in imgs]
    return dict(world=world, traj=traj, imgs=imgs, maps=maps)


def test_correspondences_equal_restatement(built_lib, ppf, synth, stream):
    c = stream
    p = E.default_params()
    rag = edge_inputs.RAGGED
    rcam = edge_inputs.ragged_cam()
    rimgs = [E.render(synth, c["world"], T, **rag) for T in c["traj"][:2]]
    fimgs = [im.astype(np.float32) * np.float32(0.001) for im in c["imgs"][3:5]]
    for im in fimgs:
        im[::7, ::5] = np.nan
        im[3::11, ::3] = -1.0
        im[5::13, 1::4] = np.inf
    fcam = dict(E.CAM, depth_scale=1.0)
    G01 = E.truth(c["traj"][0], c["traj"][1]).astype(np.float32)
    cases = [("640x480 identity", c["imgs"][0], c["imgs"][1], E.CAM, np.eye(4, dtype=np.float32)),
             ("640x480 truth", c["imgs"][0], c["imgs"][1], E.CAM, G01),
             ("333x251 identity", rimgs[0], rimgs[1], rcam, np.eye(4, dtype=np.float32)),
             ("333x251 truth", rimgs[0], rimgs[1], rcam, G01),
             ("float with holes", fimgs[0], fimgs[1], fcam, E.truth(c["traj"][3], c["traj"][4]).astype(np.float32))]
    for name, a, b, cam, T in cases:
        va, vb = view_of(ppf, a, cam), view_of(ppf, b, cam)
        got = ppf.egomotion_correspondences(va, vb, T)
        ma, mb = K.view_maps(a, cam, E.MAX_JUMP), K.view_maps(b, cam, E.MAX_JUMP)
        want, _, _ = E.correspondences(ma, mb, T, cam, p["max_corr_dist"], p["min_normal_dot"])
        n = int((want >= 0).sum())
        print("%s: %d of %d source pixels correspond" % (name, n, want.size))
        assert np.array_equal(got.reshape(-1), want), (name, np.flatnonzero(got.reshape(-1) != want)[:8])
        assert n > want.size // 10, (name, n)
        q = ppf.default_egomotion_params(max_corr_dist=0.05, min_normal_dot=0.99)
        got = ppf.egomotion_correspondences(va, vb, T, q)
        want, _, _ = E.correspondences(ma, mb, T, cam, 0.05, 0.99)
        assert np.array_equal(got.reshape(-1), want), name
        va.close()
        vb.close()


def test_pose_equals_restatement_and_reaches_the_truth(built_lib, ppf, stream):
    c = stream
    views = [view_of(ppf, im) for im in c["imgs"]]
    chain = np.eye(4)
    for f in range(1, len(views)):
        T, res = ppf.egomotion(views[f - 1], views[f])
        G = E.truth(c["traj"][f - 1], c["traj"][f])
        rot, tr = refine_ref.pose_error(T, G)
        chain = T.astype(np.float64) @ chain
        crot, ctr = refine_ref.pose_error(chain, E.truth(c["traj"][0], c["traj"][f]))
        assert rot < E.ROT_BOUND and tr < E.TRANS_BOUND, (f, rot, tr)
        assert crot < E.CHAIN_ROT_BOUND and ctr < E.CHAIN_TRANS_BOUND, (f, crot, ctr)
        assert res["ok"] and res["overlap"] >= E.OVERLAP_CONSECUTIVE_MIN
        line = "frame %d: truth %.4f deg %.4f m, chained %.4f deg %.4f m, overlap %.3f, iterations %s" % (
            f, rot, tr, crot, ctr, res["overlap"], res["iterations"])
        if f in (1, 5, 9):
            W64, w64 = E.egomotion(c["maps"][f - 1], c["maps"][f], E.CAM)
            W32, w32 = E.egomotion(c["maps"][f - 1], c["maps"][f], E.CAM, sums="f32")
            s_ang, s_dt = refine_ref.pose_error(W32, W64)
            ang, dt = refine_ref.pose_error(T, W64)
            depth = E.mean_depth(c["maps"][f - 1])
            b_ang, b_dt = max(ROT_FLOOR, 8.0 * s_ang), max(np.radians(ROT_FLOOR) * depth, 8.0 * s_dt)
            a32, d32 = refine_ref.pose_error(T, W32)
            line += "; device vs float64 sums %.3e deg %.3e m (vs the pinned float32 order %.3e deg %.3e m); spread of " \
                    "the restatement %.3e deg %.3e m; bound %.3e deg %.3e m; correspondences %d / %d" % (
                        ang, dt, a32, d32, s_ang, s_dt, b_ang, b_dt, res["correspondences"], w64["correspondences"])
            assert ang <= b_ang and dt <= b_dt, (f, ang, dt, b_ang, b_dt)
            assert res["iterations"] == w64["iterations"], (f, res, w64)
            assert res["correspondences"] == w64["correspondences"], (f, res, w64)
        print(line)
    for v in views:
        v.close()


def test_edge_cases_cost_and_determinism(built_lib, ppf, stream):
    c = stream
    a, b = view_of(ppf, c["imgs"][0]), view_of(ppf, c["imgs"][1])
    Ti = np.eye(4, dtype=np.float32)
    Ti[:3, 3] = [0.1, 0.2, 0.3]
    # src == dst: the identity at once
    T, res = ppf.egomotion(a, a, Ti)
    assert np.array_equal(T, np.eye(4, dtype=np.float32)) and res["iterations"] == [0, 0, 0] and res["launches"] == 0
    # cost: one launch per scheduled iteration, plus one for each view's maps on first use
    T1, r1 = ppf.egomotion(a, b)
    assert r1["launches"] == 19 + 2, r1
    T2, r2 = ppf.egomotion(a, b)
    assert r2["launches"] == 19, r2
    assert T1.tobytes() == T2.tobytes() and plain(r1) == plain(r2)               # two calls repeat bit for bit
    p = ppf.default_egomotion_params(levels=[(2, 3), (3, 0), (1, 2)])
    assert ppf.egomotion(a, b, None, p)[1]["launches"] == 5
    ms = sorted(ppf.egomotion(a, b)[1]["ms_total"] for _ in range(20))
    print("oslam_view_egomotion at 640x480, 19 launches: median of 20 calls %.3f ms inside the library (min %.3f)"
          % (ms[10], ms[0]))
    # a destination without a valid pixel: fewer than 6 correspondences, T_init comes back bit for bit
    empty = view_of(ppf, np.zeros_like(c["imgs"][0]))
    T, res = ppf.egomotion(a, empty, Ti)
    assert T.tobytes() == Ti.tobytes() and res["iterations"] == [0, 0, 0] and res["ok"] == 0 and res["correspondences"] == 0
    assert res["overlap"] == 0.0 and res["converged"] == 0 and res["launches"] == 19 + 1
    empty.close()
    # T_init at the truth.  Two views of one image: the truth is exactly the identity, every residual is 0 and every
    # level converges in its first iteration
    a2 = view_of(ppf, c["imgs"][0])
    T, res = ppf.egomotion(a, a2)
    assert res["iterations"] == [1, 1, 1] and res["converged"] == 1 and res["overlap"] == 1.0 and res["rmse"] == 0.0, res
    assert np.array_equal(T, np.eye(4, dtype=np.float32))
    a2.close()
    # the moving pair from its ground truth: the first step of a level is the distance of the rule's fixed point from
    # the truth, which the host test bounds; with those bounds as stop criteria every level converges at once
    G = E.truth(c["traj"][0], c["traj"][1]).astype(np.float32)
    p = ppf.default_egomotion_params(stop_rot=float(np.radians(E.ROT_BOUND)), stop_trans=E.TRANS_BOUND)
    T, res = ppf.egomotion(a, b, G, p)
    print("from the truth:", res)
    assert res["iterations"] == [1, 1, 1] and res["converged"] == 1, res
    # one level {1, n} equals the default's last level when started from the same pose: a level starts from the float32
    # pose the last one left, so the call splits at a level boundary bit for bit
    p2 = ppf.default_egomotion_params(levels=[(4, 4), (2, 5)])
    Tm, rm = ppf.egomotion(a, b, None, p2)
    Tl, rl = ppf.egomotion(a, b, Tm, ppf.default_egomotion_params(levels=[(1, 10)]))
    assert Tl.tobytes() == T1.tobytes(), refine_ref.pose_error(Tl, T1)
    assert rm["iterations"][:2] == r1["iterations"][:2] and rl["iterations"][0] == r1["iterations"][2], (rl, rm, r1)
    assert (rl["correspondences"], rl["rmse"], rl["overlap"], rl["converged"], rl["ok"]) == \
        (r1["correspondences"], r1["rmse"], r1["overlap"], r1["converged"], r1["ok"]), (rl, r1)
    # and at the first boundary: {4, 4} alone, then {2, 5} and {1, 10} from its pose
    Ta, ra = ppf.egomotion(a, b, None, ppf.default_egomotion_params(levels=[(4, 4)]))
    Tb, rb = ppf.egomotion(a, b, Ta, ppf.default_egomotion_params(levels=[(2, 5), (1, 10)]))
    assert Tb.tobytes() == T1.tobytes() and ra["iterations"][0] == r1["iterations"][0]
    assert rb["iterations"][:2] == r1["iterations"][1:] and rb["correspondences"] == r1["correspondences"]
    a.close()
    b.close()


def test_tracker_follows_an_object_under_a_moving_camera(built_lib, ppf, synth, stream):
    c = stream
    clouds = [synth.make_model(k, 1500) for k in range(3)]
    clouds = [(np.ascontiguousarray(p * np.float32(E.OBJECT_SCALE)), n) for p, n in clouds]
    d = synth.d_dist_for(clouds[0][0], 0.05)
    models = [ppf.Model(p, n, d_dist=d) for p, n in clouds]
    db = ppf.Database(models)
    # the object nearest the camera (3.6 m): the most pixels per point spacing.  Measured with tests/track_ref.py on the CPU
    # from the true camera motion: 0.68 .. 1.31 degrees and 0.197 .. 0.245 d_dist (d_dist is 0.055 m here, a pixel is
    # 0.007 m wide at that depth); the farthest object (4.6 m) reaches 0.31 d_dist with the same true motion.  The bound
    # is the one tests/test_gpu_track.py asserts, in units of a d_dist that is 3.6 times smaller here (0.25 d_dist is
    # 1.4 cm, two pixels); the headroom is 2 %.  The frames, the maps and k_track are deterministic, so it holds until the
    # renderer or the maps change, and then this error of the tracking stage itself has to be measured again
    k = 1
    poses = [(np.linalg.inv(Twc) @ E.object_pose(synth, 0, k)).astype(np.float32) for Twc in c["traj"]]
    views = [view_of(ppf, im) for im in c["imgs"]]
    ident = np.eye(4, dtype=np.float32)
    with_cam, plain_t, ident_t, none_t = (ppf.Tracker(db) for _ in range(4))
    for t in (with_cam, plain_t, ident_t, none_t):
        t.update([dict(model=k, T=poses[0])])
    lost_without = 0
    for f in range(1, len(views)):
        T_cam, res = ppf.egomotion(views[f - 1], views[f])
        assert res["ok"], (f, res)
        tracks, _ = with_cam.step(views[f], T_cam=T_cam)
        assert len(tracks) == 1 and tracks[0]["found"] and tracks[0]["misses"] == 0, (f, tracks)
        rot, tr = refine_ref.pose_error(tracks[0]["T"], poses[f])
        crot, ctr = refine_ref.pose_error(with_cam.camera(), c["traj"][f])
        a, _ = plain_t.step(views[f])
        b, _ = ident_t.step(views[f], T_cam=ident)
        assert len(a) == len(b) and all(x["T"].tobytes() == y["T"].tobytes() and plain(x["track"]) == plain(y["track"]) and
                                        (x["id"], x["found"], x["misses"]) == (y["id"], y["found"], y["misses"])
                                        for x, y in zip(a, b)), f
        n, _ = none_t.step(views[f], T_cam=None)
        assert [x["T"].tobytes() for x in n] == [x["T"].tobytes() for x in a]
        lost_without += not (a and a[0]["found"])
        print("frame %d: with T_cam rot %.3f deg trans %.3f d_dist, camera %.4f deg %.4f m; without prediction: %s"
              % (f, rot, tr / d, crot, ctr, "found" if a and a[0]["found"] else "not found" if a else "deleted"))
        assert rot < 2.0 and tr < 0.25 * d, (f, rot, tr / d)
        assert crot < E.CHAIN_ROT_BOUND and ctr < E.CHAIN_TRANS_BOUND, (f, crot, ctr)
    print("without prediction the track was not found on %d of 9 frames (not asserted)" % lost_without)
    for t in (with_cam, plain_t, ident_t, none_t):
        t.close()
    for v in views:
        v.close()
    db.close()
    for m in models:
        m.close()
