"""Numpy restatement of the mesh of the whole map, voxel store plus window (include/oslam.h at oslam_world_mesh): the
yardstick of the device path.

Built on world_surface_ref (the map G as a lookup, the frame, the trilinear read, the order) and on mesh_ref's table
arrays (the generator's table, not the compiled header).  float32 with the header's operation order, so positions,
normals, keys, triangle indices, their order and the counts equal the device's bit for bit.  Nothing here builds a dense
box.  numpy only.

The rule, restated.  Vertex v is the v-th crossing of world_surface_ref's rule in its order (bricks by (bz, by, bx), inside
a brick 3 * (i + 8 * (j + 8 * k)) + a), with or without a normal; a crossing without a normal gets (0, 0, 0).  Every
global voxel g is the corner of a cube, full iff all eight G(g + (dx, dy, dz)) are seen; corner c = dx + 2*dy + 4*dz;
case = sum((q_c < 0) << c).  Cube edge e = 4*a + m belongs to voxel g + EDGE_START[e] on axis a.  Triangles: cubes in the
order of their corner voxels (bricks, then i + 8 * (j + 8 * k)), then the table row's order; three uint32 vertex indices.
"""
import numpy as np

import mesh_ref as M
import world_surface_ref as WS

F = np.float32


def vertices(m, A, O, voxel, min_weight=1, normals=True):
    """every crossing of the map m in the device's order: -> (xyz float32 [n, 3], nrm float32 [n, 3] or None, keys int32
    [n, 4] = (g_x, g_y, g_z, a))"""
    inv_voxel = F(1.0) / voxel
    g, w0 = m.candidates()
    keep = (w0 >> np.uint32(16)) >= min_weight
    g, w0 = g[keep], w0[keep]
    gs, axs, q0s, q1s = [], [], [], []
    for a in range(3):
        e = np.zeros(3, np.int64)
        e[a] = 1
        w1 = m.at(g + e)
        cross = ((w1 >> np.uint32(16)) >= min_weight) & ((WS._q(w0) < 0) != (WS._q(w1) < 0))
        gs.append(g[cross])
        axs.append(np.full(int(cross.sum()), a, np.int64))
        q0s.append(WS._q(w0[cross]))
        q1s.append(WS._q(w1[cross]))
    g, axis = np.concatenate(gs).reshape(-1, 3), np.concatenate(axs)
    order = WS.order_of(g, axis)
    g, axis = g[order], axis[order]
    q0, q1 = np.concatenate(q0s)[order], np.concatenate(q1s)[order]
    n = len(g)
    r = g - np.array(A, np.int64)
    assert n == 0 or int(np.abs(r).max()) < 1 << 22
    keys = np.concatenate([g, axis[:, None]], axis=1).astype(np.int32)
    with np.errstate(all="ignore"):
        F0, F1 = q0.astype(np.float32) / F(32767.0), q1.astype(np.float32) / F(32767.0)
        t = F0 / (F0 - F1)
        P = [O[b] + (r[:, b].astype(np.float32) + F(0.5)) * voxel for b in range(3)]
        for a in range(3):
            P[a] = np.where(axis == a, P[a] + t * voxel, P[a])
        xyz = np.stack(P, axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
        assert t.dtype == np.float32 and all(p.dtype == np.float32 for p in P)
        if not normals:
            return np.ascontiguousarray(xyz), None, keys
        grad, ok = [], np.ones(n, bool)
        for b in range(3):
            v1, ok1 = WS._trilinear(m, A, O, inv_voxel, *[P[c] + voxel if c == b else P[c] for c in range(3)])
            v0, ok0 = WS._trilinear(m, A, O, inv_voxel, *[P[c] - voxel if c == b else P[c] for c in range(3)])
            ok &= ok1 & ok0
            grad.append(v1 - v0)
        ln = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]).astype(np.float32)
        has = ok & (ln > F(0)) & (ln <= F(3.0e38))
        nrm = np.stack([grad[b] / ln for b in range(3)], axis=1).astype(np.float32).reshape(-1, 3)
        nrm[~has] = F(0)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(nrm), keys


def emitting_cubes(m, min_weight=1):
    """-> (g int64 [n, 3], case int64 [n]) of the full cubes with a case other than 0 and 255, in the device's order"""
    g, w0 = m.candidates()
    g = g[(w0 >> np.uint32(16)) >= min_weight]                    # a cube's corner voxel is seen
    full, case = np.ones(len(g), bool), np.zeros(len(g), np.int64)
    for c in range(8):
        w = m.at(g + np.array([c & 1, c >> 1 & 1, c >> 2 & 1], np.int64))
        full &= (w >> np.uint32(16)) >= min_weight
        case |= (WS._q(w) < 0).astype(np.int64) << c
    keep = full & (case != 0) & (case != 255)
    g, case = g[keep].reshape(-1, 3), case[keep]
    order = WS.order_of(g, np.zeros(len(g), np.int64))
    return g[order], case[order]


def _codes(rows, lo, span):
    c = rows[:, :3].astype(np.int64) - lo
    return ((c[:, 2] * span[1] + c[:, 1]) * span[0] + c[:, 0]) * 3 + rows[:, 3]


def index_of(keys, wanted):
    """the row of each wanted (g_x, g_y, g_z, a) in keys [n, 4] (distinct rows): int64, -1 where it is not there"""
    if len(keys) == 0 or len(wanted) == 0:
        return np.full(len(wanted), -1, np.int64)
    both = np.concatenate([keys[:, :3], wanted[:, :3]]).astype(np.int64)
    lo = both.min(axis=0)
    span = both.max(axis=0) - lo + 1
    assert float(span[0]) * float(span[1]) * float(span[2]) * 3 < 2.0 ** 62
    kc, wc = _codes(keys, lo, span), _codes(wanted, lo, span)
    order = np.argsort(kc, kind="stable")
    at = np.minimum(np.searchsorted(kc[order], wc), len(kc) - 1)
    return np.where(kc[order][at] == wc, order[at], -1)


def triangles(keys, g, case):
    """the triangles of the cubes (g, case) against the vertices' keys: -> (tri uint32 [nt, 3], cube int64 [nt, 3] = the
    corner voxel of each triangle's cube)"""
    rows = M.EDGES[case]                                            # [cubes, 3 * MAX_TRI]
    valid = np.arange(3 * M.MAX_TRI)[None, :] < 3 * M.NTRI[case][:, None]
    e = np.where(valid, rows, 0)
    start = g[:, None, :] + M.EDGE_START[e]                         # [cubes, 3 * MAX_TRI, 3]: the voxel that owns the edge
    wanted = np.concatenate([start, (e // 4)[..., None]], axis=2)[valid]      # row-major: cube order, then the row's
    at = index_of(keys, wanted.reshape(-1, 4))
    assert (at >= 0).all()                                          # every edge of a full cube joins two seen voxels
    return np.ascontiguousarray(at.reshape(-1, 3).astype(np.uint32)), np.repeat(g, M.NTRI[case], axis=0)


def world_mesh(store, store_params, vol=None, min_weight=1, anchor=None, normals=True):
    """-> dict(xyz float32 [nv, 3], nrm float32 [nv, 3] or None, keys int32 [nv, 4], tri uint32 [nt, 3], cube int64 [nt, 3],
    cubes int), in the device's order.  store: {g: word}; store_params: (voxel, origin0) the store was made for; vol: the
    window, or None."""
    A, O, voxel = WS.frame(store_params, vol, anchor)
    m = WS.Map(store, vol)
    xyz, nrm, keys = vertices(m, A, O, voxel, min_weight, normals)
    g, case = emitting_cubes(m, min_weight)
    tri, cube = triangles(keys, g, case)
    return dict(xyz=xyz, nrm=nrm, keys=keys, tri=tri, cube=cube, cubes=len(g))


# ---------------------------------------------------------------- comparisons the tests share
def dense_keys(vol, key):
    """(g_x, g_y, g_z, a) int32 [n, 4] of mesh_ref's vertex keys 3 * lin + a on the dense volume vol (shift_ref's offset)"""
    import shift_ref as H
    nx, ny, _ = vol.n
    lin, off = key // 3, H.state(vol)[1]
    return np.stack([lin % nx + off[0], lin // nx % ny + off[1], lin // (nx * ny) + off[2], key % 3], axis=1).astype(np.int32)


def in_dense_order(mesh):
    """a world mesh as the dense volume gives it: -> (xyz, nrm, keys) sorted by (g_z, g_y, g_x, a) and the triangles as key
    triples int32 [nt, 3, 4], stably sorted by the cube's (g_z, g_y, g_x)"""
    order = WS.dense_order(mesh["keys"])
    cube = mesh["cube"]
    torder = np.lexsort((cube[:, 0], cube[:, 1], cube[:, 2])) if len(cube) else np.zeros(0, np.int64)
    nrm = mesh["nrm"][order] if mesh["nrm"] is not None else None
    return mesh["xyz"][order], nrm, mesh["keys"][order], mesh["keys"][mesh["tri"].astype(np.int64)][torder]
