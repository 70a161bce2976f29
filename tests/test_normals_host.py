"""Normals for clouds and meshes that come without them, without a GPU: the rule's restatement (tests/normals_ref.py) on
exact and degenerate inputs, the calibration (tests/normals_calib.py), the host entry points
oslam_mesh_normals and oslam_ply_read_mesh, the argument checks of every new entry and the end-to-end precondition on the
CPU oracle.
"""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_calib as CAL  # noqa: E402
import normals_ref as N  # noqa: E402

F = np.float32


lattice = N.lattice


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the restatement
def test_lattice_plane_is_exact():
    p = lattice()
    for view, want in (((0, 0, 0), (0.0, 0.0, -1.0)), ((0, 0, 5), (0.0, 0.0, 1.0))):
        nrm, curv, valid = N.estimate(p, 0.5, view)
        assert valid.all()
        assert (nrm == np.array(want, F)).all()
        assert (curv == 0).all()
    nrm, _, _ = N.estimate(p, 0.5, orient=0)
    assert (nrm == np.array((0.0, 0.0, 1.0), F)).all()        # V starts as I and the z column is never rotated


def test_permutation_permutes_bit_for_bit():
    p = CAL.cube_cloud(600, seed=3)
    perm = np.random.default_rng(4).permutation(len(p))
    a, b = N.estimate(p, 0.12, (0.5, 0.5, 3.0)), N.estimate(p[perm], 0.12, (0.5, 0.5, 3.0))
    assert same_bits(N.moments(p, 0.12)[perm], N.moments(p[perm], 0.12))
    for x, y in zip(a, b):
        assert same_bits(x[perm], y)


degenerate_cloud = N.degenerate_cloud


def test_degenerate_inputs():
    p, parts = degenerate_cloud()
    m = N.moments(p, 0.5)
    nrm, curv, valid = N.from_moments(m, p, (10.0, 0.75, 0.0))       # the viewpoint lies in the plane z = 0
    for name in ("few", "coincident", "collinear", "nonfinite"):
        s = parts[name]
        assert not valid[s].any(), name
        assert (nrm[s] == 0).all() and (curv[s] == 0).all(), name
    assert (m[parts["few"], 0] == 4).all()
    assert (m[parts["coincident"], 0] == 6).all() and (m[parts["coincident"], 1:] == 0).all()
    assert (m[parts["nonfinite"]] == 0).all()
    # neighbours at exactly the radius count: the centre of the 7 x 7 lattice has 13 within 0.5 (d2 == r2 for four of them)
    centre = parts["plane"].start + 3 * 7 + 3
    assert m[centre, 0] == 13
    assert m[parts["collinear"].start + 4, 0] == 5
    # the non-finite points are nobody's neighbours: the plane's moments are those of the plane alone
    assert same_bits(m[parts["plane"]], N.moments(p[parts["plane"]], 0.5))
    # an exact zero of the sign test keeps the solver's sign
    assert valid[parts["plane"]].all()
    assert (nrm[parts["plane"]] == np.array((0.0, 0.0, 1.0), F)).all()


def test_jacobi_agrees_with_eigh():
    p = CAL.cube_cloud()
    m = N.moments(p, CAL.CUBE_RADIUS)
    nrm, curv, valid = N.from_moments(m, p, orient=0)
    assert valid.mean() > 0.9
    for i in np.flatnonzero(valid)[:200]:
        mm = m[i].astype(np.float64)
        mean = mm[1:4] / mm[0]
        S = np.array([[mm[4], mm[5], mm[6]], [mm[5], mm[7], mm[8]], [mm[6], mm[8], mm[9]]]) / mm[0] - np.outer(mean, mean)
        w, V = np.linalg.eigh(S)
        assert abs(float(np.dot(nrm[i], V[:, 0]))) > 1.0 - 1e-5 or (w[1] - w[0]) < 1e-3 * w[2]
        assert abs(curv[i] - w[0] / w.sum()) < 1e-5


# ---------------------------------------------------------------- calibration
@pytest.fixture(scope="module")
def calib_rows(synth, oracle):
    rows = CAL.table(synth, oracle)
    print()
    print(CAL.fmt(rows))
    return rows


def test_sweep_count(calib_rows):
    """OSLAM_NORMALS_SWEEPS is the smallest count after which one more sweep changes no float32 output: on the room's
    clouds and on the volumetric cube cloud one sweep more changes nothing, and the last sweep still changes something."""
    for r in calib_rows:
        assert r["more_changes"] == 0, (r["noise"], r["factor"])
        assert r["fewer_changes"] > 0, (r["noise"], r["factor"])
    cube = CAL.cube_cloud()
    ch = CAL.sweep_changes(N.moments(cube, CAL.CUBE_RADIUS), cube, first=N.SWEEPS - 1, last=N.SWEEPS)
    print("cube cloud: outputs changed by sweep %d and %d: %s" % (N.SWEEPS, N.SWEEPS + 1, ch))
    assert ch[0] > 0 and ch[1] == 0


def test_calibration_table(calib_rows):
    """Bounds relative to the depth front end's normals on the same points, at the radius README recommends, 3 spacings
    (the whole table with the measured values: DESIGN.md 7r)."""
    by = {(r["noise"], r["factor"]): r for r in calib_rows}
    clean, noisy = by[(0.0, 3.0)], by[(1.0, 3.0)]
    print("object points with a known normal at 3 spacings: %d clean, %d noisy" % (clean["n_curved"], noisy["n_curved"]))
    assert clean["n_curved"] > 1000 and noisy["n_curved"] > 1000
    # Clean frame: the walls and the floor are exact for both (median 0), so the objects decide.  Measured: 10.12 degrees
    # median against the front end's 8.43 (1.20 times).  Margin: 1.5 times the front end's median, since a disc 6 spacings
    # wide smooths the objects' bumps more than the front end's cross of 3 pixels.
    assert clean["truth"][0] <= clean["front_truth"][0] + 1e-3
    assert clean["curved"][0] < 1.5 * clean["front_curved"][0]
    # Noise of one spacing: averaging over 22 neighbours must beat the front end's four.  Measured: 11.67 degrees median
    # against 38.39 on all points (0.30 times), 11.97 against 45.48 on the objects (0.26 times).  Margin: at most half of
    # the front end's median: five times the neighbours average the noise down by about the root of five.
    assert noisy["truth"][0] < 0.5 * noisy["front_truth"][0]
    assert noisy["curved"][0] < 0.5 * noisy["front_curved"][0]
    # the share of points that get a normal (measured: 0.9892 clean, 0.9930 noisy) and its growth with the radius
    assert clean["valid"] > 0.95 and noisy["valid"] > 0.95
    for noise in (0.0, 1.0):
        shares = [by[(noise, k)]["valid"] for k in CAL.FACTORS]
        assert shares == sorted(shares)


def test_line_ratio_default_rejects_only_lines(calib_rows):
    """The default line_ratio removes the collinear neighbourhoods (the pixel rows of the clean frame at small radii, where
    lmid is exactly 0) and next to nothing else: on the noisy frames, where no neighbourhood is exactly collinear, the
    smallest lmid / lmax is 0.0139 and nothing is removed; on the clean frames at most 5 of 72889 points lie between 0 and
    the default.  The bound is a policy: the default may cost at most a thousandth of the points."""
    for r in calib_rows:
        a = N.from_moments(r["moments"], r["points"], line_ratio=N.LINE_RATIO)[2]
        b = N.from_moments(r["moments"], r["points"], line_ratio=0.0)[2]
        extra = int((b & ~a).sum())
        print("noise %.1f factor %.1f: %d points removed by the default line_ratio beyond the exact lines" % (r["noise"], r["factor"], extra))
        assert not (a & ~b).any()
        assert extra == 0 if r["noise"] > 0 else extra < 1e-3 * len(a)


# ---------------------------------------------------------------- oslam_mesh_normals
def test_mesh_normals_icosphere(built_lib, ppf):
    p, tri = N.icosphere(2)
    assert len(p) == 162 and len(tri) == 320
    nrm, valid = ppf.mesh_normals(p, tri)
    ref, rvalid = N.mesh_normals(p, tri)
    assert same_bits(nrm, ref) and np.array_equal(valid, rvalid) and valid.all()
    # no vertex normal can leave the cone of its faces' normals: the bound is the largest angle between a face normal and
    # the radial direction of one of its corners, the flat-face angle of this subdivision
    a, b, c = (p[tri[:, k]].astype(np.float64) for k in range(3))
    fn = np.cross(b - a, c - a)
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    flat = max(float(N.angle_deg(fn, p[tri[:, k]]).max()) for k in range(3))
    assert 5.0 < flat < 15.0
    assert N.angle_deg(nrm, p).max() < flat
    inward, _ = ppf.mesh_normals(p, tri[:, ::-1])
    assert N.angle_deg(inward, -p).max() < flat
    # the reference's PointNormal stride
    wide = np.zeros((len(p), 12), F)
    wide[:, :3] = p
    assert same_bits(ppf.mesh_normals(wide, tri)[0], nrm)


def test_mesh_normals_edge_cases(built_lib, ppf):
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0], [3, 0, 0], [4, 0, 0]], F)
    tri = np.array([[0, 1, 2], [4, 5, 6], [4, 4, 5]], np.uint32)      # one good, one collinear, one with a repeated corner
    nrm, valid = ppf.mesh_normals(p, tri)
    assert valid.tolist() == [True, True, True, False, False, False, False]
    assert (nrm[:3] == np.array((0, 0, 1), F)).all() and (nrm[3:] == 0).all()
    ref, rvalid = N.mesh_normals(p, tri)
    assert same_bits(nrm, ref) and np.array_equal(valid, rvalid)
    out, ok = np.full((len(p), 3), 7.0, F), np.full(len(p), 7, np.uint8)
    bad = np.array([[0, 1, 7]], np.uint32)
    rc = built_lib.oslam_mesh_normals(ppf._p(p), len(p), 12, ppf._p(bad), 1, ppf._p(out), ppf._p(ok))
    assert rc == ppf.OSLAM_E_INVALID
    assert (out == 7).all() and (ok == 7).all()                       # nothing written


# ---------------------------------------------------------------- oslam_ply_read_mesh
def write_ply(path, binary, verts, faces, normals=None, count_type="uchar", index_type="int"):
    fmt = {"uchar": "B", "uint8": "B", "int": "i", "int32": "i", "uint32": "I", "uint": "I", "ushort": "H"}
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment a test file",
            "element vertex %d" % len(verts), "property float x", "property float y", "property float z"]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    head += ["property uchar red"]
    if faces is not None:
        head += ["element face %d" % len(faces), "property list %s %s vertex_indices" % (count_type, index_type)]
    head += ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for k, v in enumerate(verts):
            row = list(v) + (list(normals[k]) if normals is not None else [])
            if binary:
                f.write(struct.pack("<%df" % len(row), *row) + struct.pack("<B", k % 256))
            else:
                f.write((" ".join("%.9g" % x for x in row) + " %d\n" % (k % 256)).encode())
        for face in faces or []:
            if binary:
                f.write(struct.pack("<" + fmt[count_type], len(face)) + struct.pack("<%d%s" % (len(face), fmt[index_type]), *face))
            else:
                f.write((" ".join(str(x) for x in [len(face)] + list(face)) + "\n").encode())


VERTS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], F)
FACES = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [4, 2, 3, 0, 1]]
FANS = [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [4, 2, 3], [4, 3, 0], [4, 0, 1]]


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("types", [("uchar", "int"), ("uint8", "uint32"), ("ushort", "ushort")])
def test_ply_read_mesh_lists_and_fans(built_lib, ppf, tmp_path, binary, types):
    path = str(tmp_path / "m.ply")
    write_ply(path, binary, VERTS, FACES, count_type=types[0], index_type=types[1])
    p, n, t = ppf.ply_read_mesh(path)
    assert same_bits(p, VERTS) and n is None
    assert t.dtype == np.uint32 and t.tolist() == FANS
    with pytest.raises(ppf.OslamError):
        ppf.ply_read(path)                                            # the existing reader still wants normals


@pytest.mark.parametrize("binary", [False, True])
def test_ply_read_mesh_normals_and_no_faces(built_lib, ppf, tmp_path, binary):
    nrm = np.tile(np.array([[0, 0.6, 0.8]], F), (len(VERTS), 1))
    path = str(tmp_path / "n.ply")
    write_ply(path, binary, VERTS, FACES, normals=nrm)
    p, n, t = ppf.ply_read_mesh(path)
    assert same_bits(p, VERTS) and same_bits(n, nrm) and t.tolist() == FANS
    p2, n2 = ppf.ply_read(path)                                       # and reads what it read before, faces skipped
    assert same_bits(p2, VERTS) and same_bits(n2, nrm)
    write_ply(path, binary, VERTS, None)
    p, n, t = ppf.ply_read_mesh(path)
    assert same_bits(p, VERTS) and n is None and t.shape == (0, 3)
    with pytest.raises(ppf.OslamError):
        ppf.ply_read(path)
    write_ply(path, binary, VERTS, [[0, 1, 5]])                       # an index outside the vertices
    with pytest.raises(ppf.OslamError):
        ppf.ply_read_mesh(path)


@pytest.mark.parametrize("binary", [False, True])
def test_ply_mesh_round_trip(built_lib, ppf, tmp_path, binary):
    p, tri = N.icosphere(1)
    nrm, _ = ppf.mesh_normals(p, tri)
    path = str(tmp_path / "r.ply")
    ppf.ply_write_mesh(path, p, nrm, tri, binary=binary)
    p2, n2, t2 = ppf.ply_read_mesh(path)
    assert same_bits(p2, p) and same_bits(n2, nrm) and np.array_equal(t2, tri)
    p3, n3 = ppf.ply_read(path)
    assert same_bits(p3, p) and same_bits(n3, nrm)
    ppf.ply_write(path, p, nrm, binary=binary)                        # a cloud file: no face element at all
    p4, n4, t4 = ppf.ply_read_mesh(path)
    assert same_bits(p4, p) and same_bits(n4, nrm) and len(t4) == 0


# ---------------------------------------------------------------- argument checks
def test_argument_checks(built_lib, ppf):
    L, INV = built_lib, ppf.OSLAM_E_INVALID
    p = lattice(3, 3)
    nrm, curv, valid = np.full((9, 3), 7.0, F), np.full(9, 7.0, F), np.full(9, 7, np.uint8)
    mom = np.full((9, 10), 7, np.int64)
    res = ppf.NormalsResult()
    good = ppf.default_normals_params(radius=0.5)
    assert (good.min_neighbours, good.orient, tuple(good.viewpoint)) == (5, 1, (0.0, 0.0, 0.0))
    assert abs(good.line_ratio - N.LINE_RATIO) < 1e-9
    assert L.oslam_normals_params_default(None) == INV

    def cloud(xyz=p, n=9, stride=12, np_=good, out=nrm):
        return L.oslam_cloud_normals(None if xyz is None else ppf._p(xyz), n, stride, None if np_ is None else C.byref(np_), 0,
                                     None if out is None else ppf._p(out), ppf._p(curv), ppf._p(valid), C.byref(res))

    def moments(xyz=p, n=9, stride=12, np_=good, out=mom):
        return L.oslam_cloud_normal_moments(None if xyz is None else ppf._p(xyz), n, stride,
                                            None if np_ is None else C.byref(np_), 0, None if out is None else ppf._p(out))
    for call in (cloud, moments):
        assert call(xyz=None) == INV
        assert call(np_=None) == INV
        assert call(out=None) == INV
        assert call(n=0) == INV
        assert call(stride=8) == INV
        for radius in (0.0, -1.0, float("nan"), float("inf")):
            assert call(np_=ppf.default_normals_params(radius=radius)) == INV, radius
        assert call(np_=ppf.default_normals_params(radius=0.5, min_neighbours=2)) == INV
        assert call(np_=ppf.default_normals_params(radius=0.5, viewpoint=(0, float("nan"), 0))) == INV
        assert call(np_=ppf.default_normals_params(radius=0.5, line_ratio=-0.1)) == INV
    assert (nrm == 7).all() and (curv == 7).all() and (valid == 7).all() and (mom == 7).all()     # a refused call writes nothing

    tri = np.array([[0, 1, 3]], np.uint32)
    assert L.oslam_mesh_normals(None, 9, 12, ppf._p(tri), 1, ppf._p(nrm), ppf._p(valid)) == INV
    assert L.oslam_mesh_normals(ppf._p(p), 9, 12, None, 1, ppf._p(nrm), ppf._p(valid)) == INV
    assert L.oslam_mesh_normals(ppf._p(p), 9, 12, ppf._p(tri), 1, None, ppf._p(valid)) == INV
    assert L.oslam_mesh_normals(ppf._p(p), 9, 8, ppf._p(tri), 1, ppf._p(nrm), ppf._p(valid)) == INV
    assert (nrm == 7).all() and (valid == 7).all()
    a, b, c, nv, nt = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
    assert L.oslam_ply_read_mesh(None, C.byref(a), C.byref(b), C.byref(c), C.byref(nv), C.byref(nt)) == INV
    assert L.oslam_ply_read_mesh(b"x.ply", None, C.byref(b), C.byref(c), C.byref(nv), C.byref(nt)) == INV
    assert L.oslam_ply_read_mesh(b"x.ply", C.byref(a), C.byref(b), None, C.byref(nv), C.byref(nt)) == INV
    assert L.oslam_ply_read_mesh(b"/nonexistent/x.ply", C.byref(a), C.byref(b), C.byref(c), C.byref(nv), C.byref(nt)) == INV
    with pytest.raises(TypeError):
        ppf.default_normals_params(radius=1.0, nonsense=1)


# ---------------------------------------------------------------- end to end, on the CPU oracle
def test_end_to_end_precondition(built_lib, ppf, synth, oracle):
    """A model from a mesh and a scene from points alone register on the CPU oracle within the reference's acceptance test
    (alignment.cpp:141-144).  Cases tried: this one (surface 0 as a 24 x 16 grid mesh, 384 vertices, before a wall in a
    96 x 72 frame, about 6000 scene points, radius 3 spacings) was the first and passed: 0.23 units of 0.39 allowed and
    10.6 of 12 degrees."""
    c = N.e2e_case(synth, oracle)
    assert 300 <= len(c["mp"]) <= 500 and 2000 <= len(c["sp"]) <= 8000
    mn, mv = ppf.mesh_normals(c["mp"], c["tri"])
    sn, _, sv = N.estimate(c["sp"], c["radius"])
    assert mv.all() and sv.mean() > 0.95
    T, _, _ = oracle.align(c["mp"][mv], mn[mv], c["sp"][sv], sn[sv], 1, c["d_dist"])
    ok, dt, dr = N.accepted(oracle, T, c)
    print("translation %.3f of %.3f allowed, rotation %.2f of 12 degrees" % (dt, 0.1 * c["diameter"], np.degrees(dr)))
    assert ok
