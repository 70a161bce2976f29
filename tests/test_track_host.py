"""CPU: the tracking stage's yardstick, its calibration, the tracker's logic on the host and the arguments
(include/oslam.h at oslam_track and oslam_tracker_step).

Calibration (test_restatement_follows_the_smooth_stream): model 0 (1500 points, d_dist 0.198), a seed-93 start rotation,
then per frame 3 degrees about (1, 2, 0.5) and 0.5 d_dist along x, z from 5.5 m receding 5 cm per frame, a wall at 9 m,
640x480 frames rendered from 300000 surface samples; frame 0 starts from the ground truth, every later frame from the
pose tracked one frame before (the poses are chained).  Measured with tests/track_ref.py on the CPU when the defaults were
set (bounds of the test: rotation < 2.0 degrees, translation < 0.25 d_dist, those of
tests/test_gpu_refine.py::test_refine_reaches_ground_truth):

    frame  rot err (deg)  trans err (d_dist)  correspondences  iterations  supported  view_fitness  coverage  found
    1      0.149          0.075               447              10          474        1.000         0.721     1
    2      0.121          0.079               437              10          475        1.000         0.721     1
    3      0.158          0.087               433              6           471        1.000         0.721     1
    4      0.213          0.100               435              10          473        1.000         0.722     1
    5      0.290          0.073               430              10          472        1.000         0.717     1
    6      0.210          0.090               437              10          468        1.000         0.713     1
    7      0.289          0.096               428              10          466        1.000         0.714     1
    8      0.314          0.113               426              10          469        1.000         0.716     1
    9      0.361          0.101               427              10          470        1.000         0.723     1

The largest errors, 0.361 degrees and 0.113 d_dist, leave a factor of two and more to the bounds.
With the object removed from the image (the wall alone) the judgement counts 0 supported points and `found` is 0; with
the pose moved out of view every facing point is OUT and `found` is 0.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402

ROT_BOUND, TRANS_BOUND = 2.0, 0.25            # degrees, d_dist


@pytest.fixture(scope="module")
def stream(synth):
    mp, mn = synth.make_model(0, 1500)
    d = synth.d_dist_for(mp, 0.05)
    dense, _ = synth.make_model(0, 300000)
    poses = K.smooth_poses(synth, d, frames=10)
    return dict(mp=mp, mn=mn, d=d, dense=dense, poses=poses)


def test_maps_equal_the_depth_oracle(oracle, synth, stream):
    """Part 1: the restated maps, compacted in row-major order, are the cloud of oracle/oracle_depth.c bit for bit."""
    c = stream
    img = K.render(synth, c["dense"], c["poses"][0])
    cam = K.STREAM_CAM
    fimg = img.astype(np.float32) * np.float32(0.001)
    fimg[::7, ::5] = np.nan
    fimg[3::11, ::3] = -1.0
    for im, scale in ((img, 0.001), (fimg, 1.0)):
        cm = dict(cam, depth_scale=scale)
        V, N, ok = K.view_maps(im, cm, K.STREAM_MAX_JUMP)
        op, on = oracle.depth_to_cloud(im, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=scale, z_min=cam["z_min"],
                                       z_max=cam["z_max"], max_jump=K.STREAM_MAX_JUMP)
        gp, gn = K.cloud_of_maps(V, N, ok)
        assert len(gp) == len(op) > 100000
        assert np.array_equal(gp.view(np.uint32), op.view(np.uint32)) and np.array_equal(gn.view(np.uint32), on.view(np.uint32))


def test_restatement_follows_the_smooth_stream(synth, stream):
    c = stream
    T = c["poses"][0]
    rows = []
    for f in range(1, 10):
        img = K.render(synth, c["dense"], c["poses"][f])
        T, r = K.track(c["mp"], c["mn"], T, img, K.STREAM_CAM, c["d"], K.STREAM_MAX_JUMP)
        rot, tr = refine_ref.pose_error(T, c["poses"][f])
        rows.append((f, rot, tr / c["d"], r["correspondences"], r["iterations"], r["verify"]["supported"],
                     r["verify"]["view_fitness"], r["verify"]["coverage"], r["found"]))
        print("frame %d  rot %.3f deg  trans %.3f d_dist  corr %d  it %d  sup %d  vf %.3f  cov %.3f  found %d" % rows[-1])
    for row in rows:
        assert row[1] < ROT_BOUND and row[2] < TRANS_BOUND and row[8], row
    # the object removed from the image, and the pose moved out of view
    wall = K.render(synth, c["dense"], None)
    _, r = K.track(c["mp"], c["mn"], T, wall, K.STREAM_CAM, c["d"], K.STREAM_MAX_JUMP)
    assert not r["found"] and r["verify"]["supported"] == 0, r
    away = T.copy()
    away[0, 3] += 50.0
    To, r = K.track(c["mp"], c["mn"], away, img, K.STREAM_CAM, c["d"], K.STREAM_MAX_JUMP)
    assert not r["found"] and r["correspondences"] == 0 and r["iterations"] == 0 and np.array_equal(To, away), r
    assert r["verify"]["out"] == len(c["mp"]) - r["verify"]["back"]


def test_correspondence_gates_by_hand():
    """One point before a fronto-parallel plane at z = 4: the pixel's normal, the radius and the normal gate decide."""
    cam = dict(fx=10.0, fy=10.0, cx=4.0, cy=4.0, depth_scale=1.0, z_min=0.5, z_max=10.0)
    img = np.full((9, 9), 4.0, np.float32)
    maps = K.view_maps(img, cam, 0.05)
    assert maps[2][1:-1, 1:-1].all() and not maps[2][0].any() and not maps[2][:, 0].any()
    assert np.array_equal(maps[1][4, 4], np.float32([0, 0, -1]))
    T = np.eye(4, dtype=np.float32)
    mp, mn = np.float32([[0.0, 0.0, 3.9]]), np.float32([[0.0, 0.0, -1.0]])

    def pix(p=mp, n=mn, r=0.2, dot=0.8, m=maps):
        return int(K.correspondences(p, n, T, m, cam, r, dot)[0][0])
    assert pix() == 4 * 9 + 4
    assert pix(r=0.05) == -1                                   # farther than the radius
    assert pix(n=-mn) == -1                                    # BACK
    assert pix(n=np.float32([[0.8, 0.0, -0.6]])) == -1 and pix(n=np.float32([[0.6, 0.0, -0.8]])) == 4 * 9 + 4
    assert pix(p=np.float32([[-1.56, 0.0, 3.9]])) == -1        # pixel column 0: no normal there
    assert pix(p=np.float32([[9.0, 0.0, 3.9]])) == -1          # OUT
    img2 = img.copy()
    img2[4, 5] = 4.2                                           # a depth step next to the pixel: no normal
    assert pix(m=K.view_maps(img2, cam, 0.05)) == -1


# ---------------------------------------------------------------- the tracker's logic, no device
def pose(x, y=0.0, z=5.0, deg=0.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = K.axis_rotation((0, 0, 1), deg)
    T[:3, 3] = [x, y, z]
    return T


def strip(tracks):
    return [(t["id"], t["model"], np.asarray(t["T"], np.float32).tobytes(), t["age"], t["hits"], t["misses"], t["found"])
            for t in tracks]


CENTROIDS = np.float32([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0]])
EXTENTS = np.float32([2.0, 1.0])


def both(ppf, **kw):
    p = ppf.default_tracker_params(**kw)
    return ppf.Tracker.from_shapes(CENTROIDS, EXTENTS, p), K.Tracker.from_shapes(CENTROIDS, EXTENTS, **kw)


def test_tracker_update_birth_association_and_ids(built_lib, ppf):
    lib_t, ref_t = both(ppf)
    lists = [
        [dict(model=0, T=pose(0.0)), dict(model=1, T=pose(0.0))],             # two births: ids 0, 1 (different models)
        [dict(model=0, T=pose(0.9))],                                          # 0.9 < 0.5 * 2.0: the same instance, no birth
        [dict(model=0, T=pose(1.0))],                                          # exactly min_separation * extent: not < sep2
        [dict(model=1, T=pose(0.45)), dict(model=1, T=pose(0.55))],            # model 1: extent 1.0 -> 0.45 matches, 0.55 is born
        [dict(model=0, T=pose(0.5)), dict(model=0, T=pose(0.5))],              # between tracks 0 and 2: matched, twice
        [dict(model=0, T=pose(3.0)), dict(model=0, T=pose(3.2))],              # the second one matches the track the first started
    ]
    want_n = [2, 2, 3, 4, 4, 5]
    for dets, n in zip(lists, want_n):
        got = lib_t.update(dets)
        want = ref_t.update(dets)
        assert strip(got) == strip(want)
        assert len(got) == n, (dets, got)
    tr = lib_t.tracks()
    assert [t["id"] for t in tr] == [0, 1, 2, 3, 4] and [t["model"] for t in tr] == [0, 1, 0, 1, 0]
    assert all(t["hits"] == 1 and t["misses"] == 0 and t["age"] == 0 and t["found"] == 1 for t in tr)
    assert np.array_equal(tr[2]["T"], pose(1.0)) and np.array_equal(tr[0]["T"], pose(0.0))   # a match changes nothing
    lib_t.close()


def test_tracker_update_rotation_gate_and_errors(built_lib, ppf):
    lib_t, ref_t = both(ppf, assoc_max_angle=math.radians(30.0))
    for dets in ([dict(model=0, T=pose(0.0))], [dict(model=0, T=pose(0.1, deg=20.0))], [dict(model=0, T=pose(0.1, deg=60.0))]):
        assert strip(lib_t.update(dets)) == strip(ref_t.update(dets))
    assert len(lib_t.tracks()) == 2                       # 20 degrees: the same instance; 60 degrees: a second one
    with pytest.raises(ppf.OslamError) as e:
        lib_t.update([dict(model=2, T=pose(0.0))])        # no such member
    assert e.value.code == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        lib_t.update([dict(model=0, T=2 * np.eye(4))])
    assert e.value.code == ppf.OSLAM_E_INVALID
    assert len(lib_t.tracks()) == 2
    L = ppf.lib()
    out = (ppf.TrackState * 4)()
    n = C.c_size_t(0)
    assert L.oslam_tracker_tracks(lib_t._h, out, 1, C.byref(n)) == ppf.OSLAM_E_LIMIT and n.value == 2
    # a tracker made from shapes cannot step
    fake_v = C.create_string_buffer(4096)
    assert L.oslam_tracker_step(lib_t._h, None, C.cast(fake_v, C.c_void_p), out, 4, C.byref(n), None) == ppf.OSLAM_E_INVALID
    lib_t.close()


def test_restated_tracker_counts_misses_and_deletes(synth, stream):
    """The restated step on the CPU: a track born from a hand-made detection follows two frames, then the object leaves:
    misses 1, 2, 3 and the track is gone on the third (max_misses 2); nothing is born without a search."""
    c = stream
    t = K.Tracker([(c["mp"], c["mn"], c["d"])], cam=K.STREAM_CAM, max_jump=K.STREAM_MAX_JUMP)
    img0 = K.render(synth, c["dense"], c["poses"][0])
    tr, searched = t.step(img0, detect=lambda: [dict(model=0, T=c["poses"][0])])
    assert searched and [(x["id"], x["age"], x["hits"]) for x in tr] == [(0, 0, 1)]
    for f in (1, 2):
        tr, searched = t.step(K.render(synth, c["dense"], c["poses"][f]))
        assert not searched and len(tr) == 1 and tr[0]["id"] == 0 and tr[0]["found"] and tr[0]["misses"] == 0
        assert tr[0]["age"] == f and tr[0]["hits"] == f + 1
        rot, dt = refine_ref.pose_error(tr[0]["T"], c["poses"][f])
        assert rot < ROT_BOUND and dt < TRANS_BOUND * c["d"]
    wall = K.render(synth, c["dense"], None)
    kept = tr[0]["T"].copy()
    for k in (1, 2):
        tr, searched = t.step(wall)
        assert not searched and len(tr) == 1 and tr[0]["misses"] == k and not tr[0]["found"]
        assert np.array_equal(tr[0]["T"], kept)
    tr, searched = t.step(wall)
    assert tr == [] and not searched
    tr, searched = t.step(wall, detect=lambda: [dict(model=0, T=c["poses"][0])])
    assert searched and tr[0]["id"] == 1                  # ids are not reused


# ---------------------------------------------------------------- ABI
def test_track_defaults(built_lib, ppf):
    p = ppf.default_track_params()
    want = K.default_params()
    assert p.max_iterations == want["max_iterations"] == 10
    assert p.max_corr_dist == np.float32(2.0) and p.min_normal_dot == np.float32(0.8)
    assert p.stop_rot == np.float32(1e-5) and p.stop_trans == np.float32(1e-4) and list(p.reserved) == [0, 0, 0, 0]
    v, dv = p.verify, ppf.default_verify_params()
    assert (v.depth_tol, v.window, v.min_view_fitness, v.min_coverage, v.min_supported) == \
        (dv.depth_tol, dv.window, dv.min_view_fitness, dv.min_coverage, dv.min_supported)
    t = ppf.default_tracker_params()
    assert t.max_misses == 2 and t.detect_every == 10 and t.assoc_min_separation == np.float32(0.5)
    assert t.assoc_max_angle == np.float32(math.pi) and t.track.max_iterations == 10
    assert t.detect.instances.keep_not_found == 1 and t.arbitrate.min_owned_share == np.float32(0.52)
    assert ppf.default_track_params(max_iterations=3).max_iterations == 3
    with pytest.raises(TypeError):
        ppf.default_track_params(no_such_field=1)
    with pytest.raises(TypeError):
        ppf.default_tracker_params(no_such_field=1)
    for kw in (dict(detect_every=0), dict(assoc_min_separation=-1.0), dict(assoc_max_angle=4.0),
               dict(track=ppf.default_track_params(max_corr_dist=0.0))):
        with pytest.raises(ppf.OslamError) as e:
            ppf.Tracker.from_shapes(CENTROIDS, EXTENTS, ppf.default_tracker_params(**kw))
        assert e.value.code == ppf.OSLAM_E_INVALID, kw


def test_track_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Every OSLAM_E_INVALID case of oslam_track / oslam_db_track / the taps, with stand-in handles (zeroed host memory:
    device 0, usable) on a machine with or without a GPU."""
    L = ppf.lib()
    fake_m, fake_v, fake_db = C.create_string_buffer(4096), C.create_string_buffer(4096), C.create_string_buffer(4096)
    m, v, db = C.cast(fake_m, C.c_void_p), C.cast(fake_v, C.c_void_p), C.cast(fake_db, C.c_void_p)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    arr1 = (C.c_void_p * 1)(m)
    To = np.zeros(16, np.float32)
    res = (ppf.TrackResult * 1)()
    mem = np.zeros(1, np.uint32)

    def call(T=eye, params=None, models=arr1, vv=v, out=To, H=1):
        T = np.ascontiguousarray(T, np.float32).reshape(-1)
        p = params if params is not None else ppf.default_track_params()
        return L.oslam_track(models, ppf._p(T), H, vv, C.byref(p), ppf._p(out) if out is not None else None, res)

    def call_db(T=eye, params=None, d=db, members=mem, vv=v, out=To, H=1):
        T = np.ascontiguousarray(T, np.float32).reshape(-1)
        p = params if params is not None else ppf.default_track_params()
        return L.oslam_db_track(d, ppf._p(members) if members is not None else None, ppf._p(T), H, vv, C.byref(p),
                                ppf._p(out) if out is not None else None, res)

    assert call(models=None) == ppf.OSLAM_E_INVALID
    assert call(vv=None) == ppf.OSLAM_E_INVALID
    assert call(out=None) == ppf.OSLAM_E_INVALID
    assert L.oslam_track(arr1, None, 1, v, None, ppf._p(To), res) == ppf.OSLAM_E_INVALID
    assert call(models=(C.c_void_p * 1)(None)) == ppf.OSLAM_E_INVALID
    assert call_db(d=None) == ppf.OSLAM_E_INVALID
    assert call_db(members=None) == ppf.OSLAM_E_INVALID
    assert call_db(vv=None) == ppf.OSLAM_E_INVALID
    assert call_db(out=None) == ppf.OSLAM_E_INVALID
    assert call(H=0) == ppf.OSLAM_E_INVALID and call_db(H=0) == ppf.OSLAM_E_INVALID
    big = ppf.ARBITRATE_MAX_HYPOTHESES + 1
    Tb = np.zeros((big, 16), np.float32)
    assert L.oslam_track((C.c_void_p * big)(*[m.value] * big), ppf._p(Tb), big, v, None,
                         ppf._p(np.zeros((big, 16), np.float32)), None) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_track(db, ppf._p(np.zeros(big, np.uint32)), ppf._p(Tb), big, v, None,
                            ppf._p(np.zeros((big, 16), np.float32)), None) == ppf.OSLAM_E_INVALID
    bad_T = []
    T = eye.copy(); T[3] = np.nan; bad_T.append(T)
    T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad_T.append(T)
    T = eye.copy(); T[0] = -1; bad_T.append(T)
    T = eye.copy(); T[13] = 0.5; bad_T.append(T)
    for T in bad_T:
        assert call(T) == ppf.OSLAM_E_INVALID, T
        assert call_db(T) == ppf.OSLAM_E_INVALID, T
        assert L.oslam_track_correspondences(m, v, ppf._p(T), 2.0, 0.8, ppf._p(np.zeros(4, np.int32))) == ppf.OSLAM_E_INVALID
    bad_p = [dict(max_corr_dist=0.0), dict(max_corr_dist=-1.0), dict(max_corr_dist=float("nan")), dict(max_corr_dist=float("inf")),
             dict(min_normal_dot=float("nan")), dict(stop_rot=float("inf")), dict(stop_trans=float("nan")), dict(stop_rot=-1.0),
             dict(max_iterations=1001), dict(verify=ppf.default_verify_params(window=4)),
             dict(verify=ppf.default_verify_params(depth_tol=0.0)), dict(verify=ppf.default_verify_params(min_coverage=2.0))]
    for kw in bad_p:
        p = ppf.default_track_params(**kw)
        assert call(params=p) == ppf.OSLAM_E_INVALID, kw
        assert call_db(params=p) == ppf.OSLAM_E_INVALID, kw
    # a model and a view on different devices: the stand-in view says device 1
    other = C.create_string_buffer(4096)
    C.cast(other, C.POINTER(C.c_int))[0] = 1
    assert call(vv=C.cast(other, C.c_void_p)) == ppf.OSLAM_E_INVALID
    assert "different devices" in L.oslam_last_error().decode()
    assert L.oslam_track_correspondences(m, C.cast(other, C.c_void_p), ppf._p(eye), 2.0, 0.8,
                                         ppf._p(np.zeros(4, np.int32))) == ppf.OSLAM_E_INVALID
    # a member index outside the (empty stand-in) database
    assert call_db() == ppf.OSLAM_E_INVALID
    # all-zero poses are skipped without a device: zeros out, found 0
    To[:] = 7
    assert call(np.zeros(16, np.float32)) == ppf.OSLAM_OK
    assert not To.any() and res[0].found == 0 and res[0].launches == 0 and res[0].verify.supported == 0
    pix = np.zeros(4, np.int32)
    assert L.oslam_track_correspondences(None, v, ppf._p(eye), 2.0, 0.8, ppf._p(pix)) == ppf.OSLAM_E_INVALID
    assert L.oslam_track_correspondences(m, v, ppf._p(eye), 2.0, 0.8, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_track_correspondences(m, v, ppf._p(eye), 0.0, 0.8, ppf._p(pix)) == ppf.OSLAM_E_INVALID
    assert L.oslam_track_correspondences(m, v, ppf._p(eye), 2.0, float("nan"), ppf._p(pix)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_normals(None, ppf._p(np.zeros(3, np.float32)), ppf._p(np.zeros(1, np.uint8))) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_normals(v, None, ppf._p(np.zeros(1, np.uint8))) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_vertices(v, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_track_params_default(None) == ppf.OSLAM_E_INVALID
    assert L.oslam_tracker_params_default(None) == ppf.OSLAM_E_INVALID
    h = C.c_void_p(0)
    assert L.oslam_tracker_create(None, None, C.byref(h)) == ppf.OSLAM_E_INVALID
    assert L.oslam_tracker_create(db, None, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_tracker_update(None, None, 0) == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(call(params=ppf.default_track_params(max_iterations=2000)))
    assert e.value.code == ppf.OSLAM_E_INVALID and "max_iterations" in str(e.value)
