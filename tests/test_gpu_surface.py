"""GPU: the surface extraction (oslam_volume_surface, oslam_scene_from_volume, oslam_volume_set_voxels) against the numpy
restatement of tests/surface_ref.py, bit for bit: points, normals, their order and the two counts.  The volumes are
written with Volume.set_voxels or fused on the device and read back for the restatement.

A workgroup owns 1024 consecutive voxels: 16^3 is 4 workgroups, 40 x 72 x 24 is 67.5 (its rows of 40 are no multiple
of a wave, so a chunk straddles rows and slabs, and the last run is ragged), 128^3 is 2048, eight tiles of the scan."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import refine_ref as R  # noqa: E402
import surface_ref as S  # noqa: E402
import volume_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED = (40, 72, 24)
BIG = dict(nx=128, ny=128, nz=128, voxel=0.07, origin=[-2.9, -4.3, 0.3], mu=0.42, max_weight=2)        # tests/test_gpu_volume.py
RAGGED_VOL = dict(nx=40, ny=72, nz=24, voxel=0.1, origin=[-2.0, -4.0, 3.9], mu=0.25, max_weight=2)


def on_device(ppf, ref):
    """a device volume with the restated volume's parameters and words"""
    dev = ppf.Volume(ref.n[0], ref.n[1], ref.n[2], float(ref.voxel), [float(x) for x in ref.origin], mu=float(ref.mu),
                     max_weight=ref.max_weight)
    dev.set_voxels(ref.q, ref.w)
    return dev


def restated(dev, spec):
    """the restatement's volume with the device volume's words"""
    ref = V.Volume(**spec)
    ref.q, ref.w = dev.voxels()
    return ref


def check(name, dev, ref, min_weight=1):
    xyz, nrm, res = dev.surface(min_weight)
    wx, wn, wc = S.surface(ref, min_weight)
    print("%s, min_weight %d: %d crossings, %d points (restatement %d, %d), %d launches" % (
        name, min_weight, res["crossings"], res["points"], wc, len(wx), res["launches"]))
    assert (res["crossings"], res["points"]) == (wc, len(wx)) and len(xyz) == len(wx), name
    bad = np.flatnonzero((xyz.view(np.uint32) != wx.view(np.uint32)).any(axis=1) | (nrm.view(np.uint32) != wn.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (name, bad[:8], xyz[bad[:4]], wx[bad[:4]], nrm[bad[:4]], wn[bad[:4]])
    assert xyz.tobytes() == wx.tobytes() and nrm.tobytes() == wn.tobytes(), name
    xyz2, nrm2, res2 = dev.surface(min_weight)                      # two calls give equal bytes
    assert xyz2.tobytes() == xyz.tobytes() and nrm2.tobytes() == nrm.tobytes() and res2["points"] == res["points"]
    return xyz, nrm, res


def view_of(ppf, img, cam=E.CAM):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=E.MAX_JUMP)


def fused(ppf, spec, frames, poses):
    dev = ppf.Volume(**spec)
    for (img, cam), T in zip(frames, poses):
        v = view_of(ppf, img, cam)
        assert dev.integrate(v, T.astype(np.float32))["updated"] > 0
        v.close()
    return dev


def test_smallest_volume(built_lib, ppf):
    zero = S.blank(16, 16, 16)
    dev = on_device(ppf, zero)
    L = ppf.lib()
    xyz = np.full((4, 3), 7.0, np.float32)
    nrm, n, res = xyz.copy(), C.c_size_t(9), ppf.SurfaceResult()
    ppf._check(L.oslam_volume_surface(dev._h, None, ppf._p(xyz), ppf._p(nrm), 4, C.byref(n), C.byref(res)))
    assert n.value == 0 and (res.crossings, res.points, res.launches) == (0, 0, 2) and (xyz == 7.0).all() and (nrm == 7.0).all()
    dev.close()
    ref = S.checkerboard()
    dev = on_device(ppf, ref)
    _, _, res = check("16^3 checkerboard", dev, ref)
    assert res["crossings"] == 11520 and 0 < res["points"] < 11520 and res["launches"] == 3
    dev.close()
    for a, ref in enumerate(S.single_crossings()):
        dev = on_device(ppf, ref)
        _, _, res = check("16^3 single crossing on " + "xyz"[a], dev, ref)
        assert (res["crossings"], res["points"]) == (1, 0)
        dev.close()
    ref = S.wrap_bait()
    dev = on_device(ppf, ref)
    _, _, res = check("16^3 wrap bait", dev, ref)
    assert (res["crossings"], res["points"]) == (0, 0)
    dev.close()


def test_ragged_volume_written(built_lib, ppf):
    ref = S.sparse_random(*RAGGED, seed=5)
    dev = on_device(ppf, ref)
    q, w = dev.voxels()                                             # set_voxels followed by voxels returns the same arrays
    assert q.tobytes() == ref.q.tobytes() and w.tobytes() == ref.w.tobytes()
    xyz, nrm, res = check("40x72x24 sparse", dev, ref)
    check("40x72x24 sparse", dev, ref, 3)
    assert res["points"] > 50
    # cap one below the count: OSLAM_E_LIMIT with n_out equal to the count, and nothing written; so with cap 0
    L = ppf.lib()
    for cap in (res["points"] - 1, 0):
        po = np.full((res["points"], 3), 7.0, np.float32)
        no, n, r = po.copy(), C.c_size_t(0), ppf.SurfaceResult()
        rc = L.oslam_volume_surface(dev._h, None, ppf._p(po), ppf._p(no), cap, C.byref(n), C.byref(r))
        assert rc == ppf.OSLAM_E_LIMIT and n.value == res["points"] == r.points and (po == 7.0).all() and (no == 7.0).all()
    # NULL outputs count only
    n = C.c_size_t(0)
    ppf._check(L.oslam_volume_surface(dev._h, None, None, None, 0, C.byref(n), None))
    assert n.value == res["points"]
    dev.close()
    for mw in (1, 3):
        ref = S.edge_inputs(*RAGGED, min_weight=mw)
        dev = on_device(ppf, ref)
        _, _, res = check("40x72x24 edge inputs", dev, ref, mw)
        assert res["points"] > 0 and res["crossings"] > res["points"]
        dev.close()


@pytest.fixture(scope="module")
def world(synth):
    return E.make_world(synth, 0), E.trajectory(synth, 0)


def test_ragged_volume_fused(built_lib, ppf, synth, world):
    pts, traj = world
    frames = [(E.render(synth, pts, T, **edge_inputs.RAGGED), edge_inputs.ragged_cam()) for T in traj[:3]]
    dev = fused(ppf, RAGGED_VOL, frames, traj[:3])
    ref = restated(dev, RAGGED_VOL)
    _, _, res = check("40x72x24 fused from three 333x251 frames", dev, ref)
    check("40x72x24 fused from three 333x251 frames", dev, ref, 2)
    assert res["points"] > 100
    dev.close()


def test_more_workgroups_than_a_scan_tile(built_lib, ppf, synth, world):
    pts, traj = world
    dev = fused(ppf, BIG, [(E.render(synth, pts, traj[0]), E.CAM)], traj[:1])
    ref = restated(dev, BIG)
    _, nrm, res = check("128^3 fused from a 640x480 frame", dev, ref)
    assert res["points"] > 0 and np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    dev.close()


def test_scene_from_volume_equals_the_steps(built_lib, ppf):
    ref = S.sparse_random(*RAGGED, seed=11, share=0.2)
    dev = on_device(ppf, ref)
    xyz, nrm, res = dev.surface()
    assert res["points"] > 200
    for leaf in (0.0, 0.12):
        got = ppf.Scene.from_volume(dev, leaf, d_dist=0.1)
        want = ppf.Scene(xyz, nrm, d_dist=0.1) if leaf == 0.0 else ppf.Scene(*ppf.voxel_grid(xyz, nrm, leaf=leaf), d_dist=0.1)
        print("leaf %.2f: %d scene points of %d extracted" % (leaf, got.numPoints(), res["points"]))
        assert got.numPoints() == want.numPoints() > 1 and (leaf == 0.0) == (got.numPoints() == res["points"])
        for r in (0, got.numPoints() // 2, got.numPoints() - 1):
            assert np.array_equal(got.getHashKeys(r), want.getHashKeys(r)), (leaf, r)
        got.close()
        want.close()
    dev.close()


def test_a_scanned_object_is_registered_against_the_extracted_scene(built_lib, ppf, synth):
    """A synth object fused from four views at their true poses (surface_ref.object_views), a model of the object's own
    cloud registered and refined against Scene.from_volume: the acceptance test of tests/test_gpu_refine.py for a
    recovered rigid motion (found, below 2 degrees and a quarter of d_dist).  That criterion means something only when the
    scene shows the object: more than half of the model's points must have an extracted point within two voxels, which
    no single view gives (a view sees at most the half that faces it; measured 0.344).

    The frames are rendered with back faces culled, at 640 x 480 (surface_ref.object_views says why).  An earlier
    version of this test drew the open synth sheet from both sides at 320 x 240: 21 % of the extracted normals then
    pointed inwards, refinement started at the truth itself drifted to 0.42 d_dist, and the translation missed the
    bound at 0.422 d_dist (rotation 0.726 degrees): a map of a sheet seen from both sides is not a map of the object."""
    o = S.object_views(synth)
    dev = fused(ppf, S.OBJECT, [(im, dict(S.OBJECT_CAM)) for im in o["imgs"]], o["poses"])
    ref = restated(dev, S.OBJECT)
    xyz, nrm, res = check("64^3 scanned object", dev, ref)
    mp, mn = synth.make_model(0, 1500)
    mp = np.ascontiguousarray(mp * np.float32(S.OBJECT_SCALE))
    d = synth.d_dist_for(mp, 0.05)
    cover = S.coverage(mp, o["T_obj"], S.surface(ref)[0], 2 * S.OBJECT["voxel"])
    print("coverage of the model by the extracted cloud within two voxels: %.3f (%d points)" % (cover, len(xyz)))
    assert cover > 0.5
    grid = ppf.voxel_grid(mp, mn, leaf=d)
    model = ppf.Model(grid[0], grid[1], d_dist=d)
    scene = ppf.Scene.from_volume(dev, d, d_dist=0.0, ref_point_downsample_factor=2)
    T0 = model.ppf_lookup(scene).copy()
    T1, info = model.refine(scene, T0)
    a0, e0 = R.pose_error(T0, o["T_obj"])
    a1, e1 = R.pose_error(T1, o["T_obj"])
    print("registration %.3f deg %.3f d_dist, refined %.3f deg %.3f d_dist, %d scene points, %s" % (
        a0, e0 / d, a1, e1 / d, scene.numPoints(), info))
    assert info["found"] and a1 < 2.0 and e1 / d < 0.25, (a1, e1 / d, info)
    model.close()
    scene.close()
    dev.close()
