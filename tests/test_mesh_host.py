"""CPU: the marching-cubes table (tools/gen_mc_table.py against the library's compiled-in copy and against the face rule
restated here), the mesh restatement (tests/mesh_ref.py) against the properties a mesh must have, the PLY mesh writer and
the arguments of oslam_volume_mesh (include/oslam.h).

Closedness and winding are one property of the directed edges of the triangles: every directed edge occurs at most once
and its reverse exactly once.  A segment on a cube face is drawn by the two cubes at the face in opposite directions, a
fan diagonal twice inside its cube; an edge is open (no reverse) only where the cube behind its face does not emit:
outside the volume, or a cube that is not full.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as M  # noqa: E402
import surface_ref as S  # noqa: E402

G = M.G
RAGGED = (40, 72, 24)


# ---------------------------------------------------------------- the table
def test_library_table_equals_the_generator(built_lib, ppf):
    rows, max_tri = G.table()
    assert max_tri == 5
    for case in range(256):
        assert ppf.mc_table_row(case) == rows[case], case
    L = ppf.lib()
    n, buf = C.c_uint(0), np.zeros(15, np.uint8)
    assert L.oslam_mc_table_row(256, ppf._p(buf), C.byref(n)) == ppf.OSLAM_E_INVALID
    assert L.oslam_mc_table_row(3, None, C.byref(n)) == L.oslam_mc_table_row(3, ppf._p(buf), None) == ppf.OSLAM_E_INVALID
    header = open(os.path.join(os.path.dirname(ppf.LIB_PATH), "csrc", "oslam_mc_table.h")).read()
    assert header == G.header()[0]                                   # the committed header is the generator's output


def face_rule(case, axis, side):
    """The face rule restated without the generator: -> the set of undirected segments {edge, edge} of the face
    offset_axis == side, edges as (start corner, end corner)."""
    u, v = [a for a in range(3) if a != axis]

    def corner(du, dv):
        c = [0, 0, 0]
        c[axis], c[u], c[v] = side, du, dv
        return tuple(c)

    def neg(c):
        return bool(case >> (c[0] + 2 * c[1] + 4 * c[2]) & 1)

    ring = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
    edges = [frozenset((ring[i], ring[(i + 1) % 4])) for i in range(4)]
    crossing = [e for e in edges if len({neg(c) for c in e}) == 2]
    if len(crossing) == 2:
        return {frozenset(crossing)}
    if len(crossing) == 4:                                           # ambiguous: cut off the negative corners
        return {frozenset(e for e in edges if c in e) for c in ring if neg(c)}
    assert not crossing
    return set()


def test_every_row_follows_the_face_rule():
    rows, _ = G.table()
    ends = {e: frozenset(G.edge_ends(e)) for e in range(12)}
    seen_ambiguous = 0
    for case, row in enumerate(rows):
        crossing = {e for e in range(12) if len({bool(case >> (c[0] + 2 * c[1] + 4 * c[2]) & 1) for c in ends[e]}) == 2}
        assert {e for tri in row for e in tri} == crossing, case
        # the fans' diagonals cancel (each is walked once in each direction); what is left are the loops' segments
        directed = [(t[a], t[(a + 1) % 3]) for t in row for a in range(3)]
        assert len(set(directed)) == len(directed), case
        boundary = {d for d in directed if (d[1], d[0]) not in directed}
        want = set()
        for axis in range(3):
            for side in (0, 1):
                segs = face_rule(case, axis, side)
                seen_ambiguous += len(segs) == 2
                want |= segs
        got = {frozenset((ends[a], ends[b])) for a, b in boundary}
        assert got == want and len(boundary) == len(want), case
        # a diagonal never lies in a face of the cube
        for a, b in set(directed) - boundary:
            assert not (G.edge_faces(a) & G.edge_faces(b)), (case, a, b)
    assert seen_ambiguous > 0 and rows[1] == [(0, 4, 8)]


# ---------------------------------------------------------------- properties of the restated mesh
def open_edges_lie_on_silent_faces(vol, tri, min_weight=1):
    """Every directed edge at most once; its reverse once, or never where the cube behind the edge's face does not emit.
    -> (open edges, open edges whose face is the volume's border)"""
    nv = int(tri.max()) + 1 if len(tri) else 0
    d, own, rcnt = M.edge_census(tri, nv)
    assert own.max() == 1 and rcnt.max() <= 1
    cube, edges = M.triangle_origins(vol, min_weight)
    assert len(cube) == len(tri)
    full, _ = M.cube_cases(vol, min_weight)
    cube3, e0, e1 = np.concatenate([cube] * 3), np.concatenate([edges[:, 0], edges[:, 1], edges[:, 2]]), \
        np.concatenate([edges[:, 1], edges[:, 2], edges[:, 0]])
    n_open = n_border = 0
    for at in np.flatnonzero(rcnt == 0):
        faces = G.edge_faces(int(e0[at])) & G.edge_faces(int(e1[at]))
        assert len(faces) == 1, "an open edge must be a segment on a face of its cube"
        (axis, side), = faces
        behind = cube3[at].copy()
        behind[axis] += 1 if side else -1
        inside = all(0 <= behind[b] < vol.n[b] - 1 for b in range(3))
        assert not (inside and full[behind[2], behind[1], behind[0]]), (at, cube3[at], behind)
        n_open += 1
        n_border += not inside
    return n_open, n_border


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_signs_closed_and_consistently_wound(seed):
    vol = M.random_signs(*RAGGED, seed=seed, unseen_share=0.0)
    xyz, nrm, tri, cubes = M.mesh(vol)
    full, case = M.cube_cases(vol)
    assert full.all() and len(np.unique(case)) == 256                # the input was chosen so that every case occurs
    key = M.vertices(vol, normals=False)[0]
    d, own, rcnt = M.edge_census(tri, len(xyz))
    assert own.max() == 1                                            # every directed edge at most once
    planes = M.boundary_planes(vol, key)
    on_border = (planes[d[:, 0]] & planes[d[:, 1]]).any(axis=1)
    assert np.all((rcnt == 1) | on_border) and rcnt.max() == 1       # its reverse exactly once, unless on the border
    n_open, n_border = open_edges_lie_on_silent_faces(vol, tri)
    print("seed %d: %d vertices, %d triangles, %d cubes, %d open edges, all on the border" % (seed, len(xyz), len(tri), cubes, n_open))
    assert n_open == n_border > 0
    sx, sn, crossings = S.surface(vol)
    has = (nrm != 0).any(axis=1)
    assert crossings == len(xyz) and xyz[has].tobytes() == sx.tobytes() and nrm[has].tobytes() == sn.tobytes()
    assert (vol.q == 0).sum() > 100 and (vol.q == 32767).sum() > 100 and (vol.q == -32767).sum() > 100


def test_unseen_voxels_silence_exactly_their_cubes():
    vol = M.random_signs(*RAGGED, seed=4, unseen_share=0.02)
    xyz, nrm, tri, cubes = M.mesh(vol)
    cube, _ = M.triangle_origins(vol)
    nx, ny, nz = vol.n
    emitted = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    emitted[cube[:, 2], cube[:, 1], cube[:, 0]] = True
    unseen = vol.w == 0
    touches = np.zeros_like(emitted)
    mixed = np.zeros_like(emitted)
    neg = vol.q < 0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
                touches |= unseen[sl]
                mixed |= neg[sl] != neg[:-1, :-1, :-1]
    assert 0.1 < touches.mean() < 0.2                                # 1 - 0.98^8 = 0.149
    assert not (emitted & touches).any() and np.array_equal(emitted, mixed & ~touches) and emitted.sum() == cubes
    n_open, n_border = open_edges_lie_on_silent_faces(vol, tri)
    print("%d cubes emit, %d touch an unseen voxel; %d open edges, %d of them on the border" % (cubes, touches.sum(), n_open, n_border))
    assert n_open > n_border > 0
    referenced = np.zeros(len(xyz), bool)
    referenced[tri.ravel()] = True
    assert not referenced.all()                                      # vertices next to unseen voxels may be referenced by none


def test_min_weight_restated():
    vol = M.random_signs(*RAGGED, seed=5, unseen_share=0.0)
    a, b = M.mesh(vol, 1), M.mesh(vol, 3)
    assert len(b[0]) < len(a[0]) and len(b[2]) < len(a[2]) and b[3] < a[3]
    open_edges_lie_on_silent_faces(vol, b[2], 3)


def test_sphere():
    vol = M.sphere()
    c, r = np.array([0.61, 0.58, 0.63]), 0.33
    xyz, nrm, tri, cubes = M.mesh(vol)
    sx, sn, crossings = S.surface(vol)
    has = (nrm != 0).any(axis=1)
    assert has.all() and crossings == len(xyz) and xyz.tobytes() == sx.tobytes() and nrm.tobytes() == sn.tobytes()
    d, own, rcnt = M.edge_census(tri, len(xyz))
    assert own.max() == 1 and np.all(rcnt == 1)                      # closed
    referenced = np.unique(tri)
    und = np.unique(np.sort(d, axis=1), axis=0)
    assert len(referenced) - len(und) + len(tri) == 2                # V - E + F: one sphere
    p = xyz.astype(np.float64)[tri.astype(np.int64)] - c
    nrm_t = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area2 = np.linalg.norm(nrm_t, axis=1)
    volume = (p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6.0
    good = area2 > 1e-12
    assert volume > 0 and np.all((nrm_t[good] * p[good].mean(axis=1)).sum(axis=1) > 0)
    print("sphere: %d vertices, %d triangles, %d cubes, %d degenerate; area %.5f (4 pi r^2 = %.5f), volume %.5f (4/3 pi r^3 = %.5f):"
          " measurements, the field is not linear along an edge"
          % (len(xyz), len(tri), cubes, (~good).sum(), 0.5 * area2.sum(), 4 * np.pi * r * r, volume, 4.0 / 3.0 * np.pi * r ** 3))


def test_restatement_is_deterministic_and_normals_are_optional():
    vol = M.random_signs(*RAGGED, seed=6, unseen_share=0.02)
    a, b, c = M.mesh(vol), M.mesh(vol), M.mesh(vol, normals=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert c[1] is None and c[0].tobytes() == a[0].tobytes() and c[2].tobytes() == a[2].tobytes() and a[3] == c[3]
    assert a[2].dtype == np.uint32 and a[0].dtype == np.float32


# ---------------------------------------------------------------- PLY
def parse_ply_faces(path, nv):
    """the face element of a PLY file written by oslam_ply_write_mesh, parsed here: -> int64 [nt, 3]"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[0] == "ply" and "element vertex %d" % nv in lines and "property list uchar int vertex_indices" in lines
    nt = int([ln for ln in lines if ln.startswith("element face ")][0].split()[2])
    assert lines.index("element vertex %d" % nv) < lines.index("element face %d" % nt)
    if "format ascii 1.0" in lines:
        rows = body.decode().split("\n")
        assert len(rows) == nv + nt + 1 and rows[-1] == ""
        f = np.array([[int(x) for x in r.split()] for r in rows[nv:nv + nt]], np.int64).reshape(-1, 4)
    else:
        assert "format binary_little_endian 1.0" in lines and len(body) == nv * 24 + nt * 13
        rec = np.frombuffer(body[nv * 24:], np.dtype([("n", "u1"), ("v", "<i4", 3)]))
        f = np.concatenate([rec["n"][:, None].astype(np.int64), rec["v"].astype(np.int64)], axis=1).reshape(-1, 4)
    assert np.all(f[:, 0] == 3)
    return f[:, 1:]


@pytest.mark.parametrize("binary", [False, True])
def test_ply_mesh_round_trip(built_lib, ppf, tmp_path, binary):
    xyz, nrm, tri, _ = M.mesh(M.sphere())
    path = str(tmp_path / "mesh.ply")
    ppf.ply_write_mesh(path, xyz, nrm, tri, binary=binary)
    px, pn = ppf.ply_read(path)                                      # oslam_ply_read: the vertices, the faces skipped
    assert px.tobytes() == xyz.tobytes() and pn.tobytes() == nrm.tobytes()
    assert np.array_equal(parse_ply_faces(path, len(xyz)), tri.astype(np.int64))
    # a vertex-only file is still what it was
    cloud = str(tmp_path / "cloud.ply")
    ppf.ply_write(cloud, xyz, nrm, binary=binary)
    cx, cn = ppf.ply_read(cloud)
    assert cx.tobytes() == xyz.tobytes() and cn.tobytes() == nrm.tobytes()
    cloud_body, mesh_body = (open(f, "rb").read().split(b"end_header\n", 1)[1] for f in (cloud, path))
    assert mesh_body.startswith(cloud_body)                          # the vertex element is written as oslam_ply_write writes it
    # no normals: zeros; no triangles: an empty face element; an index past the vertices is refused
    ppf.ply_write_mesh(path, xyz, None, tri[:0], binary=binary)
    px, pn = ppf.ply_read(path)
    assert px.tobytes() == xyz.tobytes() and not pn.any() and len(parse_ply_faces(path, len(xyz))) == 0
    bad = tri.copy()
    bad[-1, 2] = len(xyz)
    with pytest.raises(ppf.OslamError):
        ppf.ply_write_mesh(path, xyz, nrm, bad, binary=binary)
    L = ppf.lib()
    assert L.oslam_ply_write_mesh(None, ppf._p(xyz), ppf._p(nrm), len(xyz), ppf._p(tri), len(tri), 1) == ppf.OSLAM_E_INVALID
    assert L.oslam_ply_write_mesh(os.fsencode(path), None, ppf._p(nrm), len(xyz), ppf._p(tri), len(tri), 1) == ppf.OSLAM_E_INVALID
    assert L.oslam_ply_write_mesh(os.fsencode(path), ppf._p(xyz), ppf._p(nrm), len(xyz), None, len(tri), 1) == ppf.OSLAM_E_INVALID


# ---------------------------------------------------------------- ABI
def test_mesh_defaults(built_lib, ppf):
    p = ppf.default_mesh_params()
    assert p.min_weight == 1 and list(p.reserved) == [0] * 7 and C.sizeof(ppf.MeshParams) == 32
    assert C.sizeof(ppf.MeshResult) == 20
    assert ppf.default_mesh_params(min_weight=7).min_weight == 7
    with pytest.raises(TypeError):
        ppf.default_mesh_params(no_such_field=1)
    assert ppf.lib().oslam_mesh_params_default(None) == ppf.OSLAM_E_INVALID


def test_mesh_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Every OSLAM_E_INVALID case with a stand-in handle (zeroed host memory: device 0), on a machine with or without a
    GPU."""
    L = ppf.lib()
    fa = C.create_string_buffer(4096)
    vol = C.cast(fa, C.c_void_p)
    INV = ppf.OSLAM_E_INVALID
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    buf, tri = np.zeros(64, np.float32), np.zeros(64, np.uint32)
    ok = ppf.default_mesh_params()

    def mesh(vo=vol, mp=ok, xyz=buf, nrm=buf, v_cap=4, tr=tri, t_cap=4, nv_out=C.byref(nv), nt_out=C.byref(nt)):
        return L.oslam_volume_mesh(vo, C.byref(mp) if mp is not None else None, ppf._p(xyz) if xyz is not None else None,
                                   ppf._p(nrm) if nrm is not None else None, v_cap, ppf._p(tr) if tr is not None else None,
                                   t_cap, nv_out, nt_out, None)

    assert mesh(vo=None) == mesh(nv_out=None) == mesh(nt_out=None) == INV
    assert mesh(xyz=None, nrm=None) == mesh(tr=None) == INV                      # one output without the other
    assert mesh(xyz=None, tr=None, v_cap=0, t_cap=0) == INV                      # normals without vertices
    assert mesh(xyz=None, nrm=None, tr=None, v_cap=4, t_cap=0) == INV            # caps without outputs
    assert mesh(xyz=None, nrm=None, tr=None, v_cap=0, t_cap=4) == INV
    for mw in (0, 65536):
        bad = ppf.default_mesh_params(min_weight=mw)
        assert mesh(mp=bad) == mesh(mp=bad, nrm=None) == mesh(mp=bad, xyz=None, nrm=None, tr=None, v_cap=0, t_cap=0) == INV, mw
        assert "min_weight" in L.oslam_last_error().decode()
