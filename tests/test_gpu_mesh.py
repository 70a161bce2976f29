"""GPU: the mesh extraction (oslam_volume_mesh) against the numpy restatement of tests/mesh_ref.py, bit for bit: positions,
normals, triangle indices, their order and the three counts.  The volumes are written with Volume.set_voxels or fused on
the device and read back for the restatement, as in tests/test_gpu_surface.py, whose helpers are used here.

A workgroup owns 1024 consecutive voxels: 16^3 is 4 workgroups, 40 x 72 x 24 is 67.5 (its rows of 40 are no multiple of a
wave, so a chunk straddles rows and slabs, and the last run is ragged), 128^3 is 2048, eight tiles of the scan."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import mesh_ref as M  # noqa: E402
import surface_ref as S  # noqa: E402
import test_gpu_surface as TS  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED = (40, 72, 24)


def check(name, dev, ref, min_weight=1):
    xyz, nrm, tri, res = dev.mesh(min_weight)
    wx, wn, wt, wc = M.mesh(ref, min_weight)
    print("%s, min_weight %d: %d vertices, %d triangles, %d cubes (restatement %d, %d, %d), %d launches" % (
        name, min_weight, res["vertices"], res["triangles"], res["cubes"], len(wx), len(wt), wc, res["launches"]))
    assert (res["vertices"], res["triangles"], res["cubes"]) == (len(wx), len(wt), wc), name
    assert xyz.shape == wx.shape and nrm.shape == wn.shape and tri.shape == wt.shape and tri.dtype == np.uint32
    bad = np.flatnonzero((xyz.view(np.uint32) != wx.view(np.uint32)).any(axis=1) | (nrm.view(np.uint32) != wn.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (name, bad[:8], xyz[bad[:4]], wx[bad[:4]], nrm[bad[:4]], wn[bad[:4]])
    badt = np.flatnonzero((tri != wt).any(axis=1))
    assert badt.size == 0, (name, badt[:8], tri[badt[:4]], wt[badt[:4]])
    assert xyz.tobytes() == wx.tobytes() and nrm.tobytes() == wn.tobytes() and tri.tobytes() == wt.tobytes(), name
    xyz2, nrm2, tri2, res2 = dev.mesh(min_weight)                   # two calls give equal bytes
    assert xyz2.tobytes() == xyz.tobytes() and nrm2.tobytes() == nrm.tobytes() and tri2.tobytes() == tri.tobytes()
    assert {k: v for k, v in res2.items() if k != "ms_total"} == {k: v for k, v in res.items() if k != "ms_total"}
    xyz3, nrm3, tri3, _ = dev.mesh(min_weight, normals=False)       # without normals: the same vertices and triangles
    assert nrm3 is None and xyz3.tobytes() == xyz.tobytes() and tri3.tobytes() == tri.tobytes()
    sx, sn, sres = dev.surface(min_weight)                          # the vertices with a normal are the cloud extraction's
    has = (nrm != 0).any(axis=1)
    assert sres["crossings"] == res["vertices"] and xyz[has].tobytes() == sx.tobytes() and nrm[has].tobytes() == sn.tobytes()
    return xyz, nrm, tri, res


def closed_where_the_cubes_are_full(vol, tri, min_weight=1):
    """the closedness property of tests/test_mesh_host.py on the device's own triangles"""
    import test_mesh_host as TH
    return TH.open_edges_lie_on_silent_faces(vol, tri, min_weight)


def test_smallest_volumes(built_lib, ppf):
    dev = TS.on_device(ppf, S.blank(16, 16, 16))
    L = ppf.lib()
    xyz = np.full((4, 3), 7.0, np.float32)
    nrm, tri = xyz.copy(), np.full((4, 3), 7, np.uint32)
    nv, nt, res = C.c_size_t(9), C.c_size_t(9), ppf.MeshResult()
    ppf._check(L.oslam_volume_mesh(dev._h, None, ppf._p(xyz), ppf._p(nrm), 4, ppf._p(tri), 4, C.byref(nv), C.byref(nt), C.byref(res)))
    assert (nv.value, nt.value) == (0, 0) and (res.vertices, res.triangles, res.cubes) == (0, 0, 0)
    assert (xyz == 7.0).all() and (nrm == 7.0).all() and (tri == 7).all()
    blank_launches = res.launches
    dev.close()
    ref = S.checkerboard()
    dev = TS.on_device(ppf, ref)
    _, _, tri, res = check("16^3 checkerboard", dev, ref)
    full, case = M.cube_cases(ref)
    assert full.all() and set(np.unique(case)) == {0x69, 0x96}      # four negative corners, every face ambiguous
    assert (res["vertices"], res["cubes"], res["triangles"]) == (11520, 15 ** 3, 4 * 15 ** 3)
    assert res["launches"] == blank_launches + 2                    # the blank volume ran neither k_mesh_vertices nor k_mesh_triangles
    n_open, n_border = closed_where_the_cubes_are_full(ref, tri)
    assert n_open == n_border > 0
    dev.close()
    for a, ref in enumerate(S.single_crossings()):
        dev = TS.on_device(ppf, ref)
        _, nrm, _, res = check("16^3 single crossing on " + "xyz"[a], dev, ref)
        assert (res["vertices"], res["triangles"], res["cubes"]) == (1, 0, 0) and not nrm.any()
        dev.close()
    ref = S.wrap_bait()
    dev = TS.on_device(ppf, ref)
    _, _, _, res = check("16^3 wrap bait", dev, ref)
    assert (res["vertices"], res["triangles"], res["cubes"]) == (0, 0, 0)
    dev.close()


@pytest.mark.parametrize("share", [0.0, 0.02])
def test_ragged_random_signs(built_lib, ppf, share):
    ref = M.random_signs(*RAGGED, seed=7, unseen_share=share)
    dev = TS.on_device(ppf, ref)
    xyz, nrm, tri, res = check("40x72x24 random signs, %.2f unseen" % share, dev, ref)
    assert len(np.unique(M.cube_cases(ref)[1])) == 256 and res["triangles"] > 100000
    n_open, n_border = closed_where_the_cubes_are_full(ref, tri)    # on the device's own output
    print("%d open edges, %d on the border" % (n_open, n_border))
    assert n_border > 0 and (n_open == n_border) == (share == 0.0)
    # a cap one short, vertices then triangles: OSLAM_E_LIMIT, both counts returned, the buffers untouched
    L = ppf.lib()
    for v_short, t_short in ((1, 0), (0, 1)):
        po = np.full((res["vertices"], 3), 7.0, np.float32)
        no, to = po.copy(), np.full((res["triangles"], 3), 7, np.uint32)
        nv, nt, r = C.c_size_t(0), C.c_size_t(0), ppf.MeshResult()
        rc = L.oslam_volume_mesh(dev._h, None, ppf._p(po), ppf._p(no), res["vertices"] - v_short, ppf._p(to),
                                 res["triangles"] - t_short, C.byref(nv), C.byref(nt), C.byref(r))
        assert rc == ppf.OSLAM_E_LIMIT and (nv.value, nt.value) == (res["vertices"], res["triangles"]) == (r.vertices, r.triangles)
        assert r.cubes == res["cubes"] and (po == 7.0).all() and (no == 7.0).all() and (to == 7).all()
    # NULL outputs count only
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    ppf._check(L.oslam_volume_mesh(dev._h, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), None))
    assert (nv.value, nt.value) == (res["vertices"], res["triangles"])
    dev.close()


@pytest.mark.parametrize("min_weight", [1, 3])
def test_ragged_edge_inputs(built_lib, ppf, min_weight):
    ref = S.edge_inputs(*RAGGED, min_weight=min_weight)
    dev = TS.on_device(ppf, ref)
    _, nrm, tri, res = check("40x72x24 edge inputs", dev, ref, min_weight)
    assert res["triangles"] > 0 and 0 < (nrm != 0).any(axis=1).sum() < res["vertices"]
    closed_where_the_cubes_are_full(ref, tri, min_weight)
    dev.close()


@pytest.fixture(scope="module")
def world(synth):
    return E.make_world(synth, 0), E.trajectory(synth, 0)


def test_ragged_volume_fused(built_lib, ppf, synth, world):
    pts, traj = world
    frames = [(E.render(synth, pts, T, **edge_inputs.RAGGED), edge_inputs.ragged_cam()) for T in traj[:3]]
    dev = TS.fused(ppf, TS.RAGGED_VOL, frames, traj[:3])
    ref = TS.restated(dev, TS.RAGGED_VOL)
    _, _, tri, res = check("40x72x24 fused from three 333x251 frames", dev, ref)
    check("40x72x24 fused from three 333x251 frames", dev, ref, 2)
    assert res["triangles"] > 100
    closed_where_the_cubes_are_full(ref, tri)
    dev.close()


def test_more_workgroups_than_a_scan_tile(built_lib, ppf, synth, world):
    pts, traj = world
    dev = TS.fused(ppf, TS.BIG, [(E.render(synth, pts, traj[0]), E.CAM)], traj[:1])
    ref = TS.restated(dev, TS.BIG)
    _, _, _, res = check("128^3 fused from a 640x480 frame", dev, ref)
    assert res["triangles"] > 0
    dev.close()
