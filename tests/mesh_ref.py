"""Numpy restatement of the mesh extraction (include/oslam.h at oslam_volume_mesh): the yardstick of the device path.

Built on surface_ref (the edges, the volumes) and on the generator's table (tools/gen_mc_table.py), not on the compiled
header.  float32 with the header's operation order, so positions, normals, triangle indices, their order and the three
counts equal the device's bit for bit.  numpy only.

The rule, restated.  Vertex v is the v-th crossing of the surface extraction in its order: every edge between two seen
voxels (w >= min_weight) with (q0 < 0) != (q1 < 0), ascending 3 * voxel + axis, with or without a normal; a crossing
without a normal gets (0, 0, 0).  Cube (i, j, k), i <= nx-2, j <= ny-2, k <= nz-2, is full iff its eight corners are
seen; corner c = dx + 2*dy + 4*dz; case = sum((q_c < 0) << c).  Cube edge e = 4*a + m, m the two other offsets in axis
order, has the global id 3 * lin(start voxel) + a.  Triangles: ascending linear index of the cube's corner voxel, then
the table row's order; three uint32 vertex indices each.
"""
import os
import sys

import numpy as np

import surface_ref as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table as G  # noqa: E402

F = np.float32
ROWS, MAX_TRI = G.table()
NTRI = np.array([len(r) for r in ROWS], np.int64)
EDGES = np.full((256, 3 * MAX_TRI), 255, np.int64)
for _case, _row in enumerate(ROWS):
    _flat = [e for tri in _row for e in tri]
    EDGES[_case, :len(_flat)] = _flat
EDGE_START = np.array([G.edge_ends(e)[0] for e in range(12)], np.int64)          # [12][3] offsets of the owning voxel
EDGE_END = np.array([G.edge_ends(e)[1] for e in range(12)], np.int64)


def vertices(vol, min_weight=1, normals=True):
    """-> (key int64 [n] ascending, xyz float32 [n, 3], nrm float32 [n, 3] or None): every crossing of the surface rule"""
    nx, ny, nz = vol.n
    keys, idx, q0s, q1s = [], [], [], []
    for a in range(3):
        s0, s1, q0, q1, _, _ = S._edges(vol, a, min_weight)
        cross = s0 & s1 & ((q0 < 0) != (q1 < 0))
        k, j, i = np.nonzero(cross)
        keys.append(3 * (i + nx * (j + ny * k)) + a)
        idx.append(np.stack([i, j, k], axis=1))
        q0s.append(q0[cross])
        q1s.append(q1[cross])
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    key = key[order]
    assert np.all(np.diff(key) > 0)
    ijk, axis = np.concatenate(idx)[order], key % 3
    q0, q1 = np.concatenate(q0s)[order], np.concatenate(q1s)[order]
    n = len(key)
    with np.errstate(all="ignore"):
        F0, F1 = q0.astype(np.float32) / F(32767.0), q1.astype(np.float32) / F(32767.0)
        t = F0 / (F0 - F1)
        P = [vol.origin[b] + (ijk[:, b].astype(np.float32) + F(0.5)) * vol.voxel for b in range(3)]
        for a in range(3):
            P[a] = np.where(axis == a, P[a] + t * vol.voxel, P[a])
        xyz = np.stack(P, axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
        assert t.dtype == np.float32 and all(p.dtype == np.float32 for p in P)
        if not normals:
            return key, np.ascontiguousarray(xyz), None
        g, ok = [], np.ones(n, bool)
        for b in range(3):
            v1, ok1 = vol._trilinear(*[P[c] + vol.voxel if c == b else P[c] for c in range(3)])
            v0, ok0 = vol._trilinear(*[P[c] - vol.voxel if c == b else P[c] for c in range(3)])
            ok &= ok1 & ok0
            g.append(v1 - v0)
        ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(np.float32)
        has = ok & (ln > F(0)) & (ln <= F(3.0e38))
        nrm = np.stack([g[b] / ln for b in range(3)], axis=1).astype(np.float32).reshape(-1, 3)
        nrm[~has] = F(0)
    return key, np.ascontiguousarray(xyz), np.ascontiguousarray(nrm)


def cube_cases(vol, min_weight=1):
    """-> (full bool, case int64), each [nz-1, ny-1, nx-1]"""
    seen, neg = vol.w >= min_weight, vol.q < 0
    full = np.ones(tuple(d - 1 for d in seen.shape), bool)
    case = np.zeros(full.shape, np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2 & 1
        sl = (slice(dz, seen.shape[0] - 1 + dz), slice(dy, seen.shape[1] - 1 + dy), slice(dx, seen.shape[2] - 1 + dx))
        full &= seen[sl]
        case |= neg[sl].astype(np.int64) << c
    return full, case


def emitting_cubes(vol, min_weight=1):
    """-> (i, j, k, case) of the full cubes with a case other than 0 and 255, ascending linear index of the corner voxel"""
    full, case = cube_cases(vol, min_weight)
    k, j, i = np.nonzero(full & (case != 0) & (case != 255))
    return i, j, k, case[k, j, i]


def mesh(vol, min_weight=1, normals=True):
    """-> (xyz float32 [nv, 3], nrm float32 [nv, 3] or None, tri uint32 [nt, 3], cubes)"""
    nx, ny, nz = vol.n
    key, xyz, nrm = vertices(vol, min_weight, normals)
    i, j, k, cs = emitting_cubes(vol, min_weight)
    rows = EDGES[cs]                                                         # [cubes, 3 * MAX_TRI]
    valid = np.arange(3 * MAX_TRI)[None, :] < 3 * NTRI[cs][:, None]
    e = np.where(valid, rows, 0)
    st = EDGE_START[e]                                                       # [cubes, 3 * MAX_TRI, 3]
    lin = (i[:, None] + st[..., 0]) + nx * ((j[:, None] + st[..., 1]) + ny * (k[:, None] + st[..., 2]))
    gid = (3 * lin + e // 4)[valid]                                          # row-major: cube order, then the row's order
    at = np.searchsorted(key, gid)
    assert len(gid) == 0 or (at.max() < len(key) and np.array_equal(key[at], gid))      # every needed vertex exists
    return xyz, nrm, np.ascontiguousarray(at.reshape(-1, 3).astype(np.uint32)), len(cs)


def triangle_origins(vol, min_weight=1):
    """-> (cube int64 [nt, 3] = (i, j, k) of each triangle's cube, edges int64 [nt, 3] = its corners' cube-edge numbers)"""
    i, j, k, cs = emitting_cubes(vol, min_weight)
    cube = np.repeat(np.stack([i, j, k], axis=1), NTRI[cs], axis=0)
    valid = np.arange(3 * MAX_TRI)[None, :] < 3 * NTRI[cs][:, None]
    return cube, EDGES[cs][valid].reshape(-1, 3)


# ---------------------------------------------------------------- inputs
def random_signs(nx, ny, nz, seed, unseen_share):
    """Every voxel seen (weights 1..5) except the given share; q random over the whole int16 range with a sprinkling of
    exact zeros and +-32767 (one voxel in 48 each)."""
    rng = np.random.default_rng(seed)
    vol = S.blank(nx, ny, nz)
    shape = (nz, ny, nx)
    q = rng.integers(-32767, 32768, shape).astype(np.int16)
    pick = rng.integers(0, 48, shape)
    q[pick == 0] = 0
    q[pick == 1] = 32767
    q[pick == 2] = -32767
    vol.q[:] = q
    vol.w[:] = rng.integers(1, 6, shape).astype(np.uint16)
    vol.w[rng.random(shape) < unseen_share] = 0
    return vol


def sphere(n=24, voxel=0.05, centre=(0.61, 0.58, 0.63), r=0.33):
    """The sphere of tests/test_surface_host.py: F = clamp(sdf / mu), mu = 6 voxels, stored as the integration stores it,
    unseen where sdf < -mu."""
    vol = S.blank(n, n, n, voxel=voxel, mu=6 * voxel)
    c = (np.arange(n, dtype=np.float64) + 0.5) * voxel
    x, y, z = c[None, None, :], c[None, :, None], c[:, None, None]
    sdf = (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r).astype(np.float32)
    f = np.minimum(np.float32(1.0), sdf / vol.mu)
    seen = sdf >= -vol.mu
    vol.q[seen] = np.rint(f[seen] * np.float32(32767.0)).astype(np.int16)
    vol.w[seen] = 1
    return vol


# ---------------------------------------------------------------- properties of a mesh
def directed_edges(tri):
    """-> int64 [3 * nt, 2]: the directed edges of the triangles"""
    t = tri.astype(np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_census(tri, n_vertices):
    """-> (codes of the directed edges, their multiplicities, the multiplicities of their reverses)"""
    d = directed_edges(tri)
    code, rev = d[:, 0] * n_vertices + d[:, 1], d[:, 1] * n_vertices + d[:, 0]
    uniq, cnt = np.unique(code, return_counts=True)
    at = np.searchsorted(uniq, rev)
    at_c = np.minimum(at, len(uniq) - 1)
    rcnt = np.where(uniq[at_c] == rev, cnt[at_c], 0)
    own = cnt[np.searchsorted(uniq, code)]
    return d, own, rcnt


def boundary_planes(vol, key):
    """bool [n, 6]: vertex lies in the plane i == 0, i == nx-1, j == 0, j == ny-1, k == 0, k == nz-1 (both ends of its
    edge do)"""
    nx, ny, nz = vol.n
    lin, a = key // 3, key % 3
    ijk = np.stack([lin % nx, lin // nx % ny, lin // (nx * ny)], axis=1)
    out = np.zeros((len(key), 6), bool)
    for b, nb in enumerate((nx, ny, nz)):
        out[:, 2 * b] = (ijk[:, b] == 0) & (a != b)
        out[:, 2 * b + 1] = (ijk[:, b] == nb - 1) & (a != b)
    return out
