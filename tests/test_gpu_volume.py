"""GPU: the fusion stage (oslam_volume_integrate, oslam_volume_raycast, oslam_volume_track, oslam_view_to_cloud) against
the numpy restatement of tests/volume_ref.py, bit for bit: the volume's words, the ray-cast z image, its maps and the
pinned counts.  All volumes and images are synthetic (the room of tests/camera_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402
import volume_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

DYN = ("launches", "ms_total")
ROT_FLOOR = 0.01                                  # degrees: tests/test_gpu_view_edges.py
BIG = dict(nx=128, ny=128, nz=128, voxel=0.07, origin=[-2.9, -4.3, 0.3], mu=0.42, max_weight=2)
RAGGED_VOL = dict(nx=40, ny=72, nz=24, voxel=0.1, origin=[-2.0, -4.0, 3.9], mu=0.25, max_weight=2)


def view_of(ppf, img, cam=E.CAM):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=E.MAX_JUMP)


def plain(d):
    return {k: v for k, v in d.items() if k not in DYN}


def raycast(vol, T, cam, w, h):
    return vol.raycast(T, cam["fx"], cam["fy"], cam["cx"], cam["cy"], w, h, z_min=cam["z_min"], z_max=cam["z_max"],
                       max_jump=E.MAX_JUMP)


def holed(img):
    """a float image in metres with the NaN, negative and inf holes of tests/test_gpu_camera.py"""
    im = img.astype(np.float32) * np.float32(0.001)
    im[::7, ::5] = np.nan
    im[3::11, ::3] = -1.0
    im[5::13, 1::4] = np.inf
    return im


@pytest.fixture(scope="module")
def stream(ppf, synth):
    """Seed 0 of tests/test_camera_host.py, three frames at 640x480 and at the ragged 333x251."""
    world = E.make_world(synth, 0)
    traj = E.trajectory(synth, 0)
    imgs = [E.render(synth, world, T) for T in traj[:3]]
    rimgs = [E.render(synth, world, T, **edge_inputs.RAGGED) for T in traj[:3]]
    return dict(world=world, traj=traj, imgs=imgs, rimgs=rimgs)


@pytest.fixture(scope="module")
def before(built_lib, ppf, stream):
    """egomotion between two plain depth views before any volume exists in the process"""
    a, b = view_of(ppf, stream["imgs"][0]), view_of(ppf, stream["imgs"][1])
    T, r = ppf.egomotion(a, b)
    a.close()
    b.close()
    return T, plain(r)


def cases(stream):
    fcam = dict(E.CAM, depth_scale=1.0)
    frames = [(stream["imgs"][0], E.CAM), (holed(stream["imgs"][1]), fcam), (stream["imgs"][2], E.CAM)]
    rframes = [(im, edge_inputs.ragged_cam()) for im in stream["rimgs"]]
    return [("128^3, 640x480", BIG, frames), ("40x72x24, 333x251", RAGGED_VOL, rframes)]


def fuse_both(ppf, stream, spec, frames, n):
    """n frames into a device volume and a restated one -> (device, restatement, views)"""
    dev = ppf.Volume(**spec)
    ref = V.Volume(**spec)
    views = []
    for f in range(n):
        img, cam = frames[f]
        T = stream["traj"][f].astype(np.float32)
        v = view_of(ppf, img, cam)
        res = dev.integrate(v, T)
        want = ref.integrate(V.z_image(img, cam), cam, T)
        assert res["updated"] == want and res["launches"] == 1, (f, res, want)
        views.append(v)
    return dev, ref, views


def test_integration_equals_restatement(before, built_lib, ppf, stream):
    for name, spec, frames in cases(stream):
        for n in (1, 3):
            dev, ref, views = fuse_both(ppf, stream, spec, frames, n)
            q, w = dev.voxels()
            bad = np.flatnonzero((q != ref.q).ravel() | (w != ref.w).ravel())
            print("%s after %d frame(s): %d of %d voxels seen, weights up to %d, %d differ" % (
                name, n, int((w > 0).sum()), w.size, int(w.max()), bad.size))
            assert bad.size == 0, (name, n, bad[:8], q.ravel()[bad[:8]], ref.q.ravel()[bad[:8]])
            assert (w > 0).sum() > w.size // 20
            if n == 3:
                assert w.max() == 2                              # saturated at max_weight
                # two runs from a reset volume give equal bits
                dev.reset()
                q0, w0 = dev.voxels()
                assert not q0.any() and not w0.any()
                for f in range(3):
                    dev.integrate(views[f], stream["traj"][f].astype(np.float32))
                q2, w2 = dev.voxels()
                assert q2.tobytes() == q.tobytes() and w2.tobytes() == w.tobytes()
            for v in views:
                v.close()
            dev.close()


def test_raycast_equals_restatement(before, built_lib, ppf, stream):
    outside = np.eye(4, dtype=np.float32)
    outside[:3, 3] = [0.3, -0.4, -2.5]                          # behind the volume's near face, looking in
    away = np.eye(4, dtype=np.float32)
    away[:3, :3] = K.axis_rotation((0.0, 1.0, 0.0), 180.0).astype(np.float32)
    away[:3, 3] = [0.3, -0.4, -2.5]                             # the same place, looking away: every ray misses the box
    for name, spec, frames in cases(stream):
        dev, ref, views = fuse_both(ppf, stream, spec, frames, 3)
        cam = frames[0][1]
        h, w = frames[0][0].shape
        poses = [("inside", stream["traj"][1].astype(np.float32)), ("inside, frame 2", stream["traj"][2].astype(np.float32)),
                 ("outside", outside), ("away", away)]
        for pname, T in poses:
            rv, res = raycast(dev, T, cam, w, h)
            maps, z = ppf.view_maps(rv)
            wz, wmaps, wcnt = ref.raycast(T, cam, w, h)
            rec = V.records(wmaps)
            print("%s, %s: %d hits, %d normals of %d pixels (restatement %s)" % (name, pname, res["hits"], res["normals"], w * h,
                                                                            wcnt))
            assert z.tobytes() == wz.tobytes(), (name, pname, np.flatnonzero(z.ravel() != wz.ravel())[:8])
            assert np.array_equal(maps[..., 3] != 0, wmaps[2])
            assert maps.tobytes() == rec.tobytes(), (name, pname, np.flatnonzero((maps != rec).any(axis=2).ravel())[:8])
            assert (res["hits"], res["normals"]) == (wcnt["hits"], wcnt["normals"]) and res["launches"] == 1
            if pname == "away":
                assert res["hits"] == 0 and not z.any() and not maps.any()
            elif name.startswith("128"):
                assert res["normals"] > w * h // 4, (name, pname, res)
            # a ray-cast view is a view: the cloud of its maps
            po, no = ppf.view_to_cloud(rv)
            wp, wn = K.cloud_of_maps(*wmaps)
            assert po.tobytes() == wp.tobytes() and no.tobytes() == wn.tobytes(), (name, pname)
            rv.close()
        for v in views:
            v.close()
        dev.close()


def test_a_raycast_view_is_a_view(before, built_lib, ppf, synth, stream):
    name, spec, frames = cases(stream)[0]
    dev, ref, views = fuse_both(ppf, stream, spec, frames, 3)
    cam = E.CAM
    T1 = stream["traj"][1].astype(np.float32)
    rv, _ = raycast(dev, T1, cam, 640, 480)
    _, wmaps, _ = ref.raycast(T1, cam, 640, 480)
    p = E.default_params()
    fmaps = K.view_maps(stream["imgs"][2], cam, E.MAX_JUMP)
    for T in (np.eye(4, dtype=np.float32), E.truth(stream["traj"][2], stream["traj"][1]).astype(np.float32)):
        got = ppf.egomotion_correspondences(views[2], rv, T)
        want, _, _ = E.correspondences(fmaps, wmaps, T, cam, p["max_corr_dist"], p["min_normal_dot"])
        print("frame 2 against the ray cast at frame 1's pose: %d of %d pixels correspond" % ((want >= 0).sum(), want.size))
        assert np.array_equal(got.reshape(-1), want) and (want >= 0).sum() > want.size // 10
    # oslam_verify on it runs and classes every point
    pts, nrm = synth.make_model(1, 1500)
    pts = np.ascontiguousarray(pts * np.float32(E.OBJECT_SCALE))
    m = ppf.Model(pts, nrm, d_dist=synth.d_dist_for(pts, 0.05))
    Tm = (np.linalg.inv(stream["traj"][1]) @ E.object_pose(synth, 0, 1)).astype(np.float32)
    res = m.verify(rv, Tm)
    print("oslam_verify of object 1 against the ray-cast view:", res)
    assert res["back"] + res["out"] + res["supported"] + res["occluded"] + res["conflict"] + res["unknown"] == len(pts)
    assert res["supported"] > 0
    m.close()
    rv.close()
    for v in views:
        v.close()
    dev.close()


def test_view_to_cloud_of_a_depth_view_is_depth_to_cloud(before, built_lib, ppf, stream):
    fcam = dict(E.CAM, depth_scale=1.0)
    for name, img, cam in (("640x480", stream["imgs"][0], E.CAM), ("333x251", stream["rimgs"][0], edge_inputs.ragged_cam()),
                           ("float with holes", holed(stream["imgs"][1]), fcam)):
        v = view_of(ppf, img, cam)
        po, no = ppf.view_to_cloud(v)
        wp, wn = ppf.depth_to_cloud(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"],
                                    z_min=cam["z_min"], z_max=cam["z_max"], max_jump=E.MAX_JUMP)
        print("%s: %d points" % (name, len(po)))
        assert len(po) == len(wp) > img.size // 10 and po.tobytes() == wp.tobytes() and no.tobytes() == wn.tobytes(), name
        po2, _ = ppf.view_to_cloud(v)                             # the maps exist now: the same again
        assert po2.tobytes() == po.tobytes()
        v.close()


def test_tracking_equals_the_glue_and_follows_the_restatement(before, built_lib, ppf, synth):
    """oslam_volume_track against its pinned composition bit for bit, and Volume.step over the there-and-back stream of
    tests/test_volume_host.py against the restatement's loop."""
    seed = 0
    s = V.small_stream(synth, seed)
    cam = V.SMALL_CAM
    views = [view_of(ppf, im, cam) for im in s["imgs"]]
    dev = V.room_volume(seed, cls=ppf.Volume)
    ref = V.room_volume(seed)
    want = V.there_and_back(ref, s)
    depth = E.mean_depth(s["maps"][0])
    for k, (f, Tw, rw) in enumerate(want):
        if k == 1:
            # the first tracked step, taken apart: ray cast, egomotion, composition
            rv, _ = raycast(dev, dev.T, cam, V.SMALL["width"], V.SMALL["height"])
            ppf.egomotion(views[f], rv)                           # builds the frame's maps
            Te, re_ = ppf.egomotion(views[f], rv)
            Tt, rt = dev.track(views[f], dev.T)
            assert Tt.tobytes() == V.compose(dev.T, Te).tobytes()
            assert plain(rt) == plain(re_) and rt["launches"] == re_["launches"] + 1      # the ray cast is one launch more
            rv.close()
            ref1 = V.room_volume(seed)
            ref1.integrate(s["z"][0], cam, np.eye(4, dtype=np.float32))
            T32, r32 = ref1.track(s["maps"][f], cam, np.eye(4, dtype=np.float32), sums="f32")
            T64, r64 = ref1.track(s["maps"][f], cam, np.eye(4, dtype=np.float32))
            s_ang, s_dt = refine_ref.pose_error(T32, T64)
            ang, dt = refine_ref.pose_error(Tt, T64)
            a32, d32 = refine_ref.pose_error(Tt, T32)
            print("oslam_volume_track vs the restatement: float64 sums %.3e deg %.3e m, the pinned float32 order %.3e deg %.3e m "
                  "(equal bits: %s); spread of the restatement %.3e deg %.3e m" % (ang, dt, a32, d32, Tt.tobytes() == T32.tobytes(),
                                                                                   s_ang, s_dt))
            assert rt["iterations"] == r64["iterations"] and rt["correspondences"] == r64["correspondences"], (rt, r64)
            assert Tt.tobytes() == T32.tobytes()                  # the pinned float32 order: bit for bit
            assert ang <= max(ROT_FLOOR, 8.0 * s_ang) and dt <= max(np.radians(ROT_FLOOR) * depth, 8.0 * s_dt)
        T, r = dev.step(views[f])
        rot, tr = refine_ref.pose_error(T, s["traj"][f])
        drot, dtr = refine_ref.pose_error(T, Tw)
        print("frame %d: device %.4f deg %.4f m from the truth, %.3e deg %.3e m from the restatement's pose%s" % (
            f, rot, tr, drot, dtr, "" if r is None else ", overlap %.3f (restatement %.3f)" % (r["overlap"], rw["overlap"])))
        if r is None:
            assert k == 0 and T.tobytes() == Tw.tobytes()
            continue
        assert r["ok"] == 1 and rw["ok"] == 1, (f, r, rw)
        assert drot <= ROT_FLOOR and dtr <= np.radians(ROT_FLOOR) * depth, (f, drot, dtr)
    assert rot <= V.MODEL_ROT_BOUND and tr <= V.MODEL_TRANS_BOUND, (rot, tr)
    q, w = dev.voxels()
    print("after the loop: %d voxels differ from the restatement's volume (its poses differ by rounding)" % int(
        ((q != ref.q) | (w != ref.w)).sum()))
    for v in views:
        v.close()
    dev.close()


def test_siblings_are_unchanged(before, built_lib, ppf, stream):
    """after all of the above, egomotion between two plain depth views gives the bits it gave before a volume existed"""
    T0, r0 = before
    vol = ppf.Volume(**RAGGED_VOL)
    a, b = view_of(ppf, stream["imgs"][0]), view_of(ppf, stream["imgs"][1])
    vol.integrate(a, np.eye(4, dtype=np.float32))
    T, r = ppf.egomotion(a, b)
    assert T.tobytes() == T0.tobytes() and plain(r) == r0
    a.close()
    b.close()
    vol.close()
