"""GPU: the camera motion kernels (k_ego_step, k_ego_corr) and the fusion kernels (k_tsdf_integrate, k_tsdf_raycast) on
the inputs of tests/fusion_edge_inputs.py against the numpy restatements (camera_ref, volume_ref): lattices of one
workgroup, of 7, 8 and 9 slots, of exactly 256 slots and of a short last workgroup; two views of different sizes; the
pinned float32 order at 640x480 as an assertion; volumes of 16^3 and of 8 live lanes in the last x tile from cameras
inside them; weights through 255/256 and at max_weight; rays with a zero direction component, behind the surface, across
an unseen gap and cut by z_min/z_max.  tests/test_fusion_edge_inputs.py asserts on the CPU that these inputs reach their
paths."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import fusion_edge_inputs as X  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402
import volume_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

DYN = ("launches", "ms_total")
ROT_FLOOR = 0.01                                  # degrees: tests/test_gpu_camera.py


def view_of(ppf, img, cam):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=E.MAX_JUMP)


def plain(d):
    return {k: v for k, v in d.items() if k not in DYN}


def bits(x):
    return np.float32(x).tobytes()


def assert_ego(ppf, label, va, vb, ma, mb, dst_cam, levels, built=0, T_init=None):
    """One call of oslam_view_egomotion against both restatements, and its repetition.  -> the device's (T, result)"""
    p = ppf.default_egomotion_params(levels=levels)
    T, r = ppf.egomotion(va, vb, T_init, p)
    T2, r2 = ppf.egomotion(va, vb, T_init, p)
    assert T.tobytes() == T2.tobytes() and plain(r) == plain(r2), (label, r, r2)           # a call repeats bit for bit
    assert r["launches"] == X.scheduled(levels) + built and r2["launches"] == X.scheduled(levels), (label, r, r2)
    W32, w32 = E.egomotion(ma, mb, dst_cam, T_init, sums="f32", levels=levels)
    W64, w64 = E.egomotion(ma, mb, dst_cam, T_init, levels=levels)
    nl = len(levels)
    # the count of correspondences goes through every block, slot and strand as an exact float integer
    assert r["iterations"][:nl] == w32["iterations"] and not any(r["iterations"][nl:]), (label, r, w32)
    assert r["correspondences"] == w32["correspondences"], (label, r, w32)
    assert (r["converged"], r["ok"]) == (w32["converged"], w32["ok"]), (label, r, w32)
    assert bits(r["overlap"]) == bits(w32["overlap"]) and bits(r["rmse"]) == bits(w32["rmse"]), (label, r, w32)
    if w32["correspondences"] < 6 and not any(w32["iterations"]):
        Ti = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32)
        assert T.tobytes() == Ti.tobytes(), label                                          # T_init comes back bit for bit
        return T, r
    s_ang, s_dt = refine_ref.pose_error(W32, W64)
    ang, dt = refine_ref.pose_error(T, W64)
    a32, d32 = refine_ref.pose_error(T, W32)
    depth = E.mean_depth(ma)
    b_ang, b_dt = max(ROT_FLOOR, 8.0 * s_ang), max(np.radians(ROT_FLOOR) * depth, 8.0 * s_dt)
    same = T.tobytes() == W32.tobytes()
    print("%s %s: cond %.4g; device vs float64 sums %.3e deg %.3e m (bound %.3e deg %.3e m), vs the pinned float32 order "
          "%.3e deg %.3e m, equal bits: %s; %d correspondences, iterations %s" % (
              label, levels, w32["cond"], ang, dt, b_ang, b_dt, a32, d32, same, r["correspondences"], r["iterations"]))
    assert ang <= b_ang and dt <= b_dt, (label, ang, dt, b_ang, b_dt)
    if w32["cond"] <= X.COND_STREAM_640:
        assert same, (label, w32["cond"], a32, d32)
    r["bits_held"] = bool(w32["cond"] <= X.COND_STREAM_640)
    return T, r


@pytest.fixture(scope="module")
def room(synth):
    return X.ego_world(synth)


@pytest.mark.parametrize("name", list(X.EGO_CASES))
def test_ego_lattices_equal_restatement(built_lib, ppf, synth, room, name):
    c = X.ego_case(synth, room[0], room[1], name)
    assert X.lattice_of(c["w"], c["h"], c["stride"]) == c["lattice"]
    a, b = view_of(ppf, c["imgs"][0], c["cam"]), view_of(ppf, c["imgs"][1], c["cam"])
    T, r1 = assert_ego(ppf, name, a, b, c["maps"][0], c["maps"][1], c["cam"], [(c["stride"], 1)], built=2)
    T, r = assert_ego(ppf, name, a, b, c["maps"][0], c["maps"][1], c["cam"], c["schedule"])
    if name in X.BITS_HELD:                               # below the gate: the pose's bits were asserted in both calls
        assert r1["bits_held"] and r["bits_held"], name
    if name == "1x1":
        Ti = np.eye(4, dtype=np.float32)
        Ti[:3, 3] = [0.1, 0.2, 0.3]
        T, r = assert_ego(ppf, name, a, b, c["maps"][0], c["maps"][1], c["cam"], c["schedule"], T_init=Ti)
        assert T.tobytes() == Ti.tobytes() and r["ok"] == 0 and r["iterations"] == [0, 0, 0] and r["correspondences"] == 0
    else:
        assert r["correspondences"] >= 6 and r["iterations"][:len(c["schedule"])] == [it for _, it in c["schedule"]]
    a.close()
    b.close()


def test_ego_between_different_views(built_lib, ppf, synth, room):
    s, d = (X.ego_case(synth, room[0], room[1], k) for k in X.DIFFERENT_VIEWS)
    a, b = view_of(ppf, s["imgs"][0], s["cam"]), view_of(ppf, d["imgs"][1], d["cam"])
    ma, mb = s["maps"][0], d["maps"][1]
    p = E.default_params()
    G = E.truth(room[1][0], room[1][1]).astype(np.float32)
    for T in (np.eye(4, dtype=np.float32), G):
        got = ppf.egomotion_correspondences(a, b, T)
        want, _, _ = E.correspondences(ma, mb, T, d["cam"], p["max_corr_dist"], p["min_normal_dot"])
        assert got.shape == (s["h"], s["w"]) and np.array_equal(got.reshape(-1), want), np.flatnonzero(got.reshape(-1) != want)[:8]
        assert (want >= 0).sum() > want.size // 2 and want.max() >= s["w"] * s["h"]
        got = ppf.egomotion_correspondences(a, b, T, ppf.default_egomotion_params(max_corr_dist=0.05, min_normal_dot=0.99))
        want, _, _ = E.correspondences(ma, mb, T, d["cam"], 0.05, 0.99)
        assert np.array_equal(got.reshape(-1), want)
    for levels in ([(4, 1)], [(4, 2), (2, 2), (1, 3)], [(16, 1), (3, 2)]):
        assert_ego(ppf, "83x61 -> 333x251", a, b, ma, mb, d["cam"], levels)
    # and the other way round: the large source against the small destination
    assert_ego(ppf, "333x251 -> 83x61", b, a, mb, ma, s["cam"], [(4, 2), (1, 2)])
    a.close()
    b.close()


@pytest.fixture(scope="module")
def world_640(synth):
    return E.make_world(synth, 0), E.trajectory(synth, 0)


@pytest.mark.parametrize("f", [1, 5, 9])
def test_pinned_order_at_640x480(built_lib, ppf, synth, world_640, f):
    """What tests/test_gpu_camera.py prints for frames 1, 5 and 9 of its stream, asserted: the pose of the default
    schedule has the bits of the sums="f32" restatement."""
    world, traj = world_640
    imgs = [E.render(synth, world, traj[k]) for k in (f - 1, f)]
    maps = [K.view_maps(im, E.CAM, E.MAX_JUMP) for im in imgs]
    a, b = view_of(ppf, imgs[0], E.CAM), view_of(ppf, imgs[1], E.CAM)
    levels = E.default_params()["levels"]
    W32, w32 = E.egomotion(maps[0], maps[1], E.CAM, sums="f32")
    assert w32["cond"] <= X.COND_STREAM_640, w32
    T, r = assert_ego(ppf, "640x480 frame %d" % f, a, b, maps[0], maps[1], E.CAM, levels, built=2)
    assert T.tobytes() == W32.tobytes(), refine_ref.pose_error(T, W32)
    a.close()
    b.close()


# ---------------------------------------------------------------- fusion
def assert_words(dev, ref, label):
    q, w = dev.voxels()
    bad = np.flatnonzero((q != ref.q).ravel() | (w != ref.w).ravel())
    assert bad.size == 0, (label, bad.size, bad[:8], q.ravel()[bad[:8]], ref.q.ravel()[bad[:8]], w.ravel()[bad[:8]],
                           ref.w.ravel()[bad[:8]])
    return q, w


@pytest.mark.parametrize("n", X.VOLUME_SIZES)
def test_integration_equals_restatement(built_lib, ppf, n):
    spec = X.volume_spec(n)
    dev = ppf.Volume(**spec)
    total = 0
    for name, m, T, img, cam in X.integration_cases():
        if m != n:
            continue
        ref = V.Volume(**spec)
        v = view_of(ppf, img, cam)
        z = V.z_image(img, cam)
        for rep in range(2):                                  # a second frame on top: the voxels are read back
            want = ref.integrate(z, cam, T)
            res = dev.integrate(v, T)
            assert res["updated"] == want and res["launches"] == 1, (name, rep, res, want)
            q, w = assert_words(dev, ref, (name, rep))
        total += want
        dev.reset()
        q0, w0 = dev.voxels()
        assert not q0.any() and not w0.any()
        for rep in range(2):
            dev.integrate(v, T)
        q2, w2 = dev.voxels()
        assert q2.tobytes() == q.tobytes() and w2.tobytes() == w.tobytes(), name          # after a reset: equal bits
        dev.reset()
        v.close()
    assert total > 0
    dev.close()


@pytest.mark.parametrize("max_weight", X.MAX_WEIGHTS)
def test_weights_equal_restatement(built_lib, ppf, max_weight):
    n, T, imgs, cam = X.weight_case()
    spec = X.volume_spec(n, max_weight)
    dev, ref = ppf.Volume(**spec), V.Volume(**spec)
    views = [view_of(ppf, im, cam) for im in imgs]
    z = [V.z_image(im, cam) for im in imgs]
    kept = {}
    for rnd in range(2):
        for s in range(X.WEIGHT_STEPS):
            res = dev.integrate(views[s % 2], T)
            if rnd == 0:
                assert res["updated"] == ref.integrate(z[s % 2], cam, T), s
            if s + 1 in X.WEIGHT_CHECKS:
                if rnd == 0:
                    q, w = assert_words(dev, ref, (max_weight, s + 1))
                    assert w.max() == min(s + 1, max_weight)
                    kept[s + 1] = (q.tobytes(), w.tobytes())
                else:
                    q, w = dev.voxels()
                    assert (q.tobytes(), w.tobytes()) == kept[s + 1], (max_weight, s + 1)
        dev.reset()
    for v in views:
        v.close()
    dev.close()


def fuse_device(ppf, n):
    dev = ppf.Volume(**X.volume_spec(n))
    for img, cam, T in X.fuse_frames(n):
        v = view_of(ppf, img, cam)
        dev.integrate(v, T)
        v.close()
    return dev


def assert_raycast(ppf, dev, ref, label, T, cam, w, h):
    rv, res = dev.raycast(T, cam["fx"], cam["fy"], cam["cx"], cam["cy"], w, h, z_min=cam["z_min"], z_max=cam["z_max"],
                          max_jump=E.MAX_JUMP)
    maps, z = ppf.view_maps(rv)
    wz, wmaps, wcnt = ref.raycast(T, X.full_cam(cam), w, h)
    rec = V.records(wmaps)
    print("%s: %d hits, %d normals of %d pixels" % (label, res["hits"], res["normals"], w * h))
    assert z.tobytes() == wz.tobytes(), (label, np.flatnonzero(z.ravel() != wz.ravel())[:8])
    assert maps.tobytes() == rec.tobytes(), (label, np.flatnonzero((maps != rec).any(axis=2).ravel())[:8])
    assert (res["hits"], res["normals"]) == (wcnt["hits"], wcnt["normals"]) and res["launches"] == 1, (label, res, wcnt)
    po, no = ppf.view_to_cloud(rv)
    wp, wn = K.cloud_of_maps(*wmaps)
    assert po.tobytes() == wp.tobytes() and no.tobytes() == wn.tobytes(), label
    rv.close()
    return wcnt


def test_raycast_equals_restatement(built_lib, ppf):
    dev, ref = fuse_device(ppf, X.RAY_N), X.fused(X.RAY_N)
    assert_words(dev, ref, "fused")
    hits = 0
    for name, T, cam, w, h in X.ray_cases():
        hits += assert_raycast(ppf, dev, ref, name, T, cam, w, h)["hits"]
    assert hits > 5000
    dev.close()


@pytest.mark.parametrize("n", X.VOLUME_SIZES[:2])
def test_raycast_of_small_volumes_equals_restatement(built_lib, ppf, n):
    dev, ref = fuse_device(ppf, n), X.fused(n)
    assert_words(dev, ref, "fused")
    for name, T, cam, w, h in X.small_ray_cases(n):
        assert assert_raycast(ppf, dev, ref, "%s %s" % (n, name), T, cam, w, h)["normals"] > 50
    dev.close()


def test_special_raycasts_equal_restatement(built_lib, ppf):
    for name, n, frames, T, cam, w, h in X.special_ray_cases():
        spec = X.volume_spec(n)
        dev, ref = ppf.Volume(**spec), V.Volume(**spec)
        for img, fcam, Tf in frames:
            v = view_of(ppf, img, fcam)
            assert dev.integrate(v, Tf)["updated"] == ref.integrate(V.z_image(img, fcam), fcam, Tf)
            v.close()
        assert_words(dev, ref, name)
        assert_raycast(ppf, dev, ref, name, T, cam, w, h)
        dev.close()
