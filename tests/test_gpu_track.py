"""GPU: the tracking stage (oslam_view_normals, oslam_track, oslam_db_track, oslam_track_correspondences) against the
numpy restatement of tests/track_ref.py, and the tracker (oslam_tracker_step) on the smooth-motion stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

DYN = ("launches", "ms_total")
CAM, MAX_JUMP = K.STREAM_CAM, K.STREAM_MAX_JUMP
ROT_BOUND, TRANS_BOUND = 2.0, 0.25            # degrees, d_dist: tests/test_gpu_refine.py::test_refine_reaches_ground_truth


def view_of(ppf, img, cam=CAM, max_jump=MAX_JUMP):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=max_jump)


def scene_of(ppf, img, d):
    return ppf.Scene.from_depth(img, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], leaf=d, d_dist=0.0,
                                ref_point_downsample_factor=4, z_min=CAM["z_min"], z_max=CAM["z_max"], max_jump=MAX_JUMP)


def plain(d):
    """a result dict without the fields that depend on the call"""
    return {k: (plain(v) if isinstance(v, dict) else v) for k, v in d.items() if k not in DYN}


@pytest.fixture(scope="module")
def stream(ppf, synth):
    """Model 0 (1500 points) on the smooth-motion stream of tests/test_track_host.py: the frames 0..9 and the wall."""
    mp, mn = synth.make_model(0, 1500)
    d = synth.d_dist_for(mp, 0.05)
    dense, _ = synth.make_model(0, 300000)
    poses = K.smooth_poses(synth, d, frames=10)
    imgs = [K.render(synth, dense, T) for T in poses]
    model = ppf.Model(mp, mn, d_dist=d)
    yield dict(mp=mp, mn=mn, d=d, poses=poses, imgs=imgs, wall=K.render(synth, dense, None), model=model)
    model.close()


def test_view_normals_equal_depth_to_cloud(built_lib, ppf, stream):
    c = stream
    fimg = c["imgs"][0].astype(np.float32) * np.float32(0.001)
    fimg[::7, ::5] = np.nan
    fimg[3::11, ::3] = -1.0
    fimg[5::13, 1::4] = np.inf
    for img, scale in ((c["imgs"][0], 0.001), (fimg, 1.0)):
        cam = dict(CAM, depth_scale=scale)
        view = view_of(ppf, img, cam)
        vtx, nrm, has = ppf.view_normals(view)
        cp, cn = ppf.depth_to_cloud(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=scale, z_min=cam["z_min"],
                                    z_max=cam["z_max"], max_jump=MAX_JUMP)
        assert int(has.sum()) == len(cp) > 100000
        assert np.array_equal(vtx[has].view(np.uint32), cp.view(np.uint32))
        assert np.array_equal(nrm[has].view(np.uint32), cn.view(np.uint32))
        assert not vtx[~has].any() and not nrm[~has].any()
        V, N, ok = K.view_maps(img, cam, MAX_JUMP)
        assert np.array_equal(ok, has) and np.array_equal(V.view(np.uint32), vtx.view(np.uint32))
        assert np.array_equal(N.view(np.uint32), nrm.view(np.uint32))
        view.close()


def test_correspondences_equal_restatement(built_lib, ppf, stream):
    c = stream
    f = 4
    truth = c["poses"][f]
    off = truth.copy()
    off[:3, :3] = (K.axis_rotation((0.3, -1.0, 0.4), 3.0) @ truth[:3, :3].astype(np.float64)).astype(np.float32)
    behind = truth.copy()
    behind[2, 3] = K.STREAM_WALL + 1.5
    away = truth.copy()
    away[0, 3] += 50.0
    poses = {"truth": truth, "previous": c["poses"][f - 1], "off3": off, "behind": behind, "away": away}
    view = view_of(ppf, c["imgs"][f])
    maps = K.view_maps(c["imgs"][f], CAM, MAX_JUMP)
    r = np.float32(2.0) * np.float32(c["d"])
    n = {}
    for name, T in poses.items():
        got = ppf.track_correspondences(c["model"], view, T, 2.0, 0.8)
        want, _, _ = K.correspondences(c["mp"], c["mn"], T, maps, CAM, r, 0.8)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
        n[name] = int((got >= 0).sum())
    got = ppf.track_correspondences(c["model"], view, poses["previous"], 0.7, 0.95)
    want, _, _ = K.correspondences(c["mp"], c["mn"], poses["previous"], maps, CAM, np.float32(0.7) * np.float32(c["d"]), 0.95)
    assert np.array_equal(got, want)
    view.close()
    assert n["truth"] > 300 and n["previous"] > 100 and n["off3"] > 100 and n["behind"] == 0 and n["away"] == 0, n


def test_track_equals_restatement_and_verify(built_lib, ppf, stream):
    c = stream
    for f in (1, 5, 9):
        view = view_of(ppf, c["imgs"][f])
        T0 = c["poses"][f - 1]
        T1, res, found = ppf.track([c["model"]], view, T0[None])
        W, w = K.track(c["mp"], c["mn"], T0, c["imgs"][f], CAM, c["d"], MAX_JUMP)
        ang, dt = refine_ref.pose_error(T1[0], W)
        print("frame %d: device vs restatement %.5f deg %.2e d_dist, iterations %d / %d, correspondences %d / %d"
              % (f, ang, dt / c["d"], res[0]["iterations"], w["iterations"], res[0]["correspondences"], w["correspondences"]))
        assert ang < 0.01 and dt < 1e-3 * c["d"], (f, ang, dt / c["d"])
        assert abs(res[0]["iterations"] - w["iterations"]) <= 1, (res[0], w)
        ver = c["model"].verify(view, T1[0])
        assert plain(res[0]["verify"]) == plain(ver), (res[0]["verify"], ver)
        assert bool(res[0]["found"]) == bool(ver["found"]) == bool(found[0]) and found[0]
        rot, tr = refine_ref.pose_error(T1[0], c["poses"][f])
        assert rot < ROT_BOUND and tr < TRANS_BOUND * c["d"]
        # a judgement with other parameters is oslam_verify's with them
        vp = ppf.default_verify_params(window=2, depth_tol=0.5, min_coverage=0.9)
        T2, res2, _ = ppf.track([c["model"]], view, T0[None], ppf.default_track_params(verify=vp))
        assert np.array_equal(T2, T1) and plain(res2[0]["verify"]) == plain(c["model"].verify(view, T2[0], vp))
        view.close()
    # the object removed from the image, and a pose out of view: not found, the pose kept when nothing corresponds
    view = view_of(ppf, c["wall"])
    T1, res, found = ppf.track([c["model"]], view, c["poses"][3][None])
    assert not found[0] and res[0]["verify"]["supported"] == 0
    away = c["poses"][3].copy()
    away[0, 3] += 50.0
    T1, res, found = ppf.track([c["model"]], view, away[None])
    assert not found[0] and res[0]["iterations"] == 0 and res[0]["correspondences"] == 0 and np.array_equal(T1[0], away)
    view.close()


def test_track_is_deterministic_and_launches_once(built_lib, ppf, synth, stream):
    c = stream
    clouds = [synth.make_model(k, 300 + 37 * k) for k in range(1, 50)]
    others = [ppf.Model(p, n, d_dist=synth.d_dist_for(p, 0.05)) for p, n in clouds]
    models = [c["model"]] + others
    db = ppf.Database(models)
    f = 3
    view = view_of(ppf, c["imgs"][f])
    rng = synth.SplitMix64(11)
    T = np.zeros((50, 4, 4), np.float32)
    for j in range(50):
        T[j] = c["poses"][f - 1]
        if j:
            T[j, :3, :3] = synth.random_rotation(rng)
    T[7] = 0
    T[31] = 0
    fresh = ppf.track(models[:1], view, T[:1])
    assert fresh[1][0]["launches"] == 2                       # k_view_normals and k_track
    a = ppf.track(models, view, T)
    b = ppf.track(models, view, T)
    assert np.array_equal(a[0], b[0]) and [plain(r) for r in a[1]] == [plain(r) for r in b[1]] and np.array_equal(a[2], b[2])
    assert all(r["launches"] == 1 for r in a[1])
    dbr = db.track(view, np.arange(50), T)
    assert np.array_equal(dbr[0], a[0]) and [plain(r) for r in dbr[1]] == [plain(r) for r in a[1]]
    for j in (0, 1, 7, 20, 31, 49):
        s = ppf.track([models[j]], view, T[j][None])
        assert np.array_equal(s[0][0], a[0][j]) and plain(s[1][0]) == plain(a[1][j]), j
        assert s[1][0]["launches"] == (0 if j in (7, 31) else 1)
    for j in (7, 31):
        assert not a[0][j].any() and not a[2][j] and a[1][j]["iterations"] == 0 and a[1][j]["verify"]["supported"] == 0
    assert np.array_equal(a[0][0], fresh[0][0]) and a[2][0]
    # several instances of one model are several entries
    two = ppf.track([models[0], models[0]], view, np.stack([T[0], c["poses"][f]]))
    assert np.array_equal(two[0][0], a[0][0]) and two[2].all()
    for it in (1, 30):
        p = ppf.default_track_params(max_iterations=it)
        for ms, Tm in ((models[:1], T[:1]), (models, T)):
            r = ppf.track(ms, view, Tm, p)
            assert all(x["launches"] == 1 for x in r[1]) and max(x["iterations"] for x in r[1]) <= it
    r0 = ppf.track(models[:1], view, T[:1], ppf.default_track_params(max_iterations=0))
    assert np.array_equal(r0[0][0], T[0]) and r0[1][0]["iterations"] == 0 and r0[1][0]["launches"] == 1
    assert plain(r0[1][0]["verify"]) == plain(c["model"].verify(view, T[0]))
    view.close()
    db.close()
    for m in others:
        m.close()


@pytest.fixture(scope="module")
def db10(ppf, synth):
    """The 10-model database of tests/test_gpu_verify.py (members 0..9, voxel-gridded at d_dist) and the stream's frames
    with their scenes' parameters."""
    raw = [synth.make_model(k, 1500) for k in range(10)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    poses = K.smooth_poses(synth, d, frames=10)
    imgs = [K.render(synth, dense, T) for T in poses]
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)
    shapes = [(instances_ref.centroid(g[0]), instances_ref.extent(g[0])) for g in grids]
    yield dict(db=db, d=d, poses=poses, imgs=imgs, wall=K.render(synth, dense, None), shapes=shapes)
    db.close()
    for m in models:
        m.close()


def same_instance(shapes, model, A, B):
    c, ext = shapes[model]
    sep2, cos_thr, rot_on = instances_ref.thresholds(0.5, np.pi, ext)
    return instances_ref.same_instance(instances_ref.transformed_centroid(A, c), A, instances_ref.transformed_centroid(B, c), B,
                                       sep2, cos_thr, rot_on)


def test_stream_follows_the_detection_without_voting(built_lib, ppf, db10):
    c = db10
    db, d = c["db"], c["d"]
    tracker = ppf.Tracker(db)
    sc, view = scene_of(ppf, c["imgs"][0], d), view_of(ppf, c["imgs"][0])
    det = db.detect(sc, view)
    tracks, searched = tracker.step(view, sc)
    sc.close()
    view.close()
    print("frame 0: db.detect ->", [(x["model"], x["instance"]) for x in det])
    assert searched and len(tracks) == len(det) >= 1
    assert [(t["model"], t["T"].tobytes()) for t in tracks] == [(x["model"], x["T"].tobytes()) for x in det]
    mine = [t for t in tracks if t["model"] == 0]
    assert mine, "db.detect did not report model 0 on frame 0"
    me = min(mine, key=lambda t: np.linalg.norm(t["T"][:3, 3] - c["poses"][0][:3, 3]))["id"]
    born = {t["id"] for t in tracks}
    for f in range(1, 10):
        view = view_of(ppf, c["imgs"][f])
        tracks, searched = tracker.step(view)
        view.close()
        assert not searched and {t["id"] for t in tracks} <= born
        t = [x for x in tracks if x["id"] == me]
        assert len(t) == 1 and t[0]["found"] and t[0]["misses"] == 0 and t[0]["hits"] == f + 1 and t[0]["age"] == f, (f, t)
        rot, tr = refine_ref.pose_error(t[0]["T"], c["poses"][f])
        print("frame %d: rot %.3f deg, trans %.3f d_dist, correspondences %d, iterations %d, others %s"
              % (f, rot, tr / d, t[0]["track"]["correspondences"], t[0]["track"]["iterations"],
                 [(x["id"], x["model"], x["found"]) for x in tracks if x["id"] != me]))
        assert rot < ROT_BOUND and tr < TRANS_BOUND * d, (f, rot, tr / d)
        assert t[0]["track"]["launches"] == 2              # a fresh view per frame: k_view_normals and k_track
    view = view_of(ppf, c["wall"])
    for k in (1, 2, 3):
        tracks, searched = tracker.step(view)
        t = [x for x in tracks if x["id"] == me]
        assert not searched and {x["id"] for x in tracks} <= born
        if k < 3:
            assert len(t) == 1 and t[0]["misses"] == k and not t[0]["found"], (k, t)
        else:
            assert t == [], t
    view.close()
    tracker.close()


def test_search_frames_keep_one_track_per_instance(built_lib, ppf, db10):
    c = db10
    db, d = c["db"], c["d"]
    tracker = ppf.Tracker(db, ppf.default_tracker_params(detect_every=3))
    ids = set()
    for f in range(10):
        sc, view = scene_of(ppf, c["imgs"][f], d), view_of(ppf, c["imgs"][f])
        tracks, searched = tracker.step(view, sc)
        assert searched or f % 3, f                                # a search is due on every third frame (and when no track lives)
        if searched:
            for x in db.detect(sc, view):
                n = sum(t["model"] == x["model"] and same_instance(c["shapes"], x["model"], x["T"], t["T"]) for t in tracks)
                assert n == 1, (f, x["model"], n)
        for i, a in enumerate(tracks):
            for b in tracks[i + 1:]:
                assert a["model"] != b["model"] or not same_instance(c["shapes"], a["model"], a["T"], b["T"]), (f, a["id"], b["id"])
        assert [t["id"] for t in tracks] == sorted(t["id"] for t in tracks)
        new = {t["id"] for t in tracks} - ids
        assert all(i > max(ids, default=-1) for i in new)           # ids are never reused
        ids |= new
        sc.close()
        view.close()
    assert any(t["model"] == 0 and t["found"] for t in tracks)
    tracker.close()
