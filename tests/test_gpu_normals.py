"""oslam_cloud_normals on the device against its restatement (tests/normals_ref.py), bit for bit: moments (int64), normals,
curvature and valid flags, at the sizes and shapes where the grid or the kernel takes another path; then the two
conveniences and the command-line front end on the end-to-end case of tests/test_normals_host.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_calib as CAL  # noqa: E402
import normals_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
VIEW = (0.4, 0.6, 3.0)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(ppf, p, radius, view=VIEW, result=None, **fields):
    """The device's four outputs equal the restatement's; -> the device's (normals, curvature, valid)."""
    m = ppf.normal_moments(p, radius)
    ref_m = N.moments(p, radius)
    assert same_bits(m, ref_m)
    nrm, curv, valid = ppf.estimate_normals(p, radius, view, result=result, **fields)
    rn, rc, rv = N.from_moments(ref_m, p, view, **fields)
    assert np.array_equal(valid, rv)
    assert same_bits(nrm, rn)
    assert same_bits(curv, rc)
    return nrm, curv, valid


@pytest.fixture(scope="module")
def cube():
    return CAL.cube_cloud()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_random_cube(built_lib, ppf, cube, n):
    res = {}
    _, _, valid = check(ppf, cube[:n], CAL.CUBE_RADIUS, result=res)
    assert res["n_valid"] == int(valid.sum()) and res["launches"] == 6 and res["edge"] >= CAL.CUBE_RADIUS
    if n == 1000:
        assert valid.mean() > 0.9
    if n <= 65:
        _, _, valid = check(ppf, cube[:n], 2.0)             # few points, all of them neighbours: the valid path at small n
        assert valid.all() == (n >= 5)


def test_one_cell_plane_borders(built_lib, ppf, cube):
    res = {}
    check(ppf, cube[:300] * F(0.05), 0.125, result=res)          # every point in one cell
    assert res["n_cells"] == 1
    flat = cube[:500].copy()
    flat[:, 2] = F(0.25)                                          # a planar cloud: one grid dimension is 1
    nrm, _, valid = check(ppf, flat, 0.1, result=res)
    assert valid.any() and (np.abs(nrm[valid, 2]) == 1).all()
    # points on the bounding box's faces and on cell borders: a lattice whose step is the radius, and one whose step is the
    # grid's edge as the host computes it
    g = np.arange(5)
    for step in (0.25, float(F(0.25)) * (1.0 + 1e-4)):
        gx, gy, gz = np.meshgrid(g * step, g * step, g * step, indexing="ij")
        p = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(F)
        check(ppf, p, 0.25, min_neighbours=3)
        check(ppf, p, 0.36)


def test_two_distant_clusters_enlarge_the_edge(built_lib, ppf, cube):
    radius = 0.1
    a = cube[:300] * F(0.3)
    b = cube[300:600] * F(0.3) + F(1e4 * radius)                 # 10^4 radii away along every axis: 10^12 cells of one radius
    res = {}
    _, _, valid = check(ppf, np.concatenate([a, b]), radius, result=res)
    assert res["edge"] > radius * 1.01 and res["n_cells"] <= 1 << 24
    assert valid[:300].any() and valid[300:].any()


def test_degenerate_inputs(built_lib, ppf):
    p, parts = N.degenerate_cloud()
    nrm, curv, valid = check(ppf, p, 0.5, (10.0, 0.75, 0.0))     # the viewpoint lies in the plane's tangent plane
    for name in ("few", "coincident", "collinear", "nonfinite"):
        assert not valid[parts[name]].any()
    assert valid[parts["plane"]].all() and (nrm[parts["plane"]] == np.array((0, 0, 1), F)).all()
    only_bad = np.full((3, 3), np.nan, F)                         # no finite point at all
    nrm, curv, valid = check(ppf, only_bad, 0.5)
    assert not valid.any()


def test_orient_stride_and_null_outputs(built_lib, ppf, cube):
    p = cube[:257]
    free, _, v0 = check(ppf, p, 0.2, orient=0)
    towards, _, v1 = check(ppf, p, 0.2, orient=1)
    assert np.array_equal(v0, v1) and v0.any()
    flipped = (free != towards).any(axis=1)
    assert flipped.any() and not flipped.all()
    assert same_bits(np.where(flipped[:, None], -free, free), towards)
    wide = np.full((len(p), 12), np.nan, F)                       # pcl::PointNormal: 48 bytes, the rest is never read
    wide[:, :3] = p
    for x, y in zip(ppf.estimate_normals(wide, 0.2, VIEW), ppf.estimate_normals(p, 0.2, VIEW)):
        assert same_bits(x, y)
    assert same_bits(ppf.normal_moments(wide, 0.2), ppf.normal_moments(p, 0.2))
    nrm, curv, valid = ppf.estimate_normals(p, 0.2, VIEW, want=())
    assert curv is None and valid is None and same_bits(nrm, towards)


def test_twice_and_permuted(built_lib, ppf, cube):
    """The order-free claim where the cells' internal order really varies: the same call twice, and a permuted cloud."""
    a = ppf.estimate_normals(cube, CAL.CUBE_RADIUS, VIEW)
    b = ppf.estimate_normals(cube, CAL.CUBE_RADIUS, VIEW)
    perm = np.random.default_rng(9).permutation(len(cube))
    c = ppf.estimate_normals(cube[perm], CAL.CUBE_RADIUS, VIEW)
    for x, y, z in zip(a, b, c):
        assert same_bits(x, y) and same_bits(x[perm], z)
    assert same_bits(ppf.normal_moments(cube, CAL.CUBE_RADIUS)[perm], ppf.normal_moments(cube[perm], CAL.CUBE_RADIUS))


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def e2e(synth, oracle):
    return N.e2e_case(synth, oracle)


def test_from_points_and_from_mesh(built_lib, ppf, oracle, e2e):
    c = e2e
    mn, mv = N.mesh_normals(c["mp"], c["tri"])
    sn, _, sv = N.estimate(c["sp"], c["radius"])
    scene = ppf.Scene(c["sp"][sv], sn[sv], d_dist=c["d_dist"])
    model = ppf.Model(c["mp"][mv], mn[mv], d_dist=c["d_dist"])
    T_ref = model.ppf_lookup(scene)
    scene2 = ppf.Scene.from_points(c["sp"], c["radius"], (0, 0, 0), d_dist=c["d_dist"])
    model2 = ppf.Model.from_mesh(c["mp"], c["tri"], d_dist=c["d_dist"])
    assert scene2.numPoints() == int(sv.sum()) and model2.numPoints() == int(mv.sum())
    T = model2.ppf_lookup(scene2)
    assert np.array_equal(T, T_ref)
    ok, dt, dr = N.accepted(oracle, T, c)
    print("translation %.3f of %.3f allowed, rotation %.2f of 12 degrees" % (dt, 0.1 * c["diameter"], np.degrees(dr)))
    assert ok
    for h in (scene, model, scene2, model2):
        h.close()


def alignment(ppf, *args):
    exe = os.path.join(os.path.dirname(ppf.LIB_PATH), "oslam_alignment")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)


def test_alignment_front_end(built_lib, ppf, e2e, tmp_path):
    """The same two clouds as normal-less PLY files: the model's normals from its faces, the scene's from --normal_radius."""
    c = e2e
    mfile, sfile, vfile = (str(tmp_path / x) for x in ("model.ply", "scene.ply", "truth.txt"))
    N.write_ply_plain(mfile, c["mp"], c["tri"])
    N.write_ply_plain(sfile, c["sp"])
    np.savetxt(vfile, c["truth"])
    # the leaf keeps every scene point (it is below their spacing): the voxel grid only reorders them
    args = ["--scene_files", sfile, "--model_files", mfile, "--tau_d", str(N.E2E_TAU_D), "--scene_leaf_size", "0.05",
            "--validation_files", vfile, "--dev", "0"]
    r = alignment(ppf, *args, "--normal_radius", "%.9g" % c["radius"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["1"], r.stderr
    assert "triangles" in r.stderr and "estimating normals" in r.stderr
    r = alignment(ppf, *args)                                     # without the flag the points-only file is refused
    assert r.returncode != 0 and "--normal_radius" in r.stderr and r.stdout.strip() == ""
