"""Numpy restatement of the surface of the whole map, voxel store plus window (include/oslam.h at oslam_world_surface):
the yardstick of the device path.

The map.  G(g) is a 32-bit word for every global voxel coordinate g: inside the window's box (off <= g < off + n) the
window's word, seen or not; elsewhere the store's word, or 0 where the store has nothing.  A store entry inside the
window's box is ignored.  Without a volume the map is the store alone.

The frame.  An anchor A picks it: O = shift_ref.window_origin(origin0, A, voxel), a voxel's index is r = g - A.
Crossings, points and normals are surface_ref.surface's with idx = r and origin = O; a voxel outside the map reads as 0,
so there is no last-voxel rule, and the range test of the trilinear base becomes "finite and |b| < 2^22".

Nothing here builds a dense box: G is looked up by searching a sorted array of packed coordinates.  The store is
reload_ref's dict {(gx, gy, gz): word}; volumes are volume_ref.Volume as shift_ref carries them.  float32 with the
header's operation order, so points, normals, their order, the keys and the two counts equal the device's bit for bit.
numpy only.
"""
import numpy as np

import reload_ref as W
import shift_ref as H

F = np.float32
BIAS = 1 << 23                                                        # |g_a| < 2^23 wherever a lookup is made
COORD_MAX = F(4194304.0)                                              # 2^22


def _pack(g):
    g = np.asarray(g, np.int64) + BIAS
    return (g[..., 2] << 48) | (g[..., 1] << 24) | g[..., 0]


class Map:
    """G as a lookup: the window's box answered from the window's words, the rest from the store's sorted keys."""

    def __init__(self, store, vol=None):
        self.vol = vol
        if vol is not None:
            self.words = W.words_of(vol)
            self.lo = np.array(H.state(vol)[1], np.int64)
            self.n = np.array(vol.n, np.int64)
        g = np.array(list(store.keys()), np.int64).reshape(-1, 3)
        w = np.array(list(store.values()), np.uint32).reshape(-1)
        if vol is not None and len(g):
            outside = ~((g >= self.lo) & (g < self.lo + self.n)).all(axis=1)
            g, w = g[outside], w[outside]
        order = np.argsort(_pack(g), kind="stable") if len(g) else np.zeros(0, np.int64)
        self.sg, self.sw, self.sk = g[order], w[order], _pack(g)[order] if len(g) else np.zeros(0, np.int64)

    def at(self, g):
        """uint32 [n]: G at g int64 [n, 3]"""
        g = np.asarray(g, np.int64).reshape(-1, 3)
        out = np.zeros(len(g), np.uint32)
        rest = np.ones(len(g), bool)
        if self.vol is not None:
            c = g - self.lo
            inside = ((c >= 0) & (c < self.n)).all(axis=1)
            out[inside] = self.words[c[inside, 2], c[inside, 1], c[inside, 0]]
            rest = ~inside
        if len(self.sk) and rest.any():
            k = _pack(g[rest])
            pos = np.minimum(np.searchsorted(self.sk, k), len(self.sk) - 1)
            out[rest] = np.where(self.sk[pos] == k, self.sw[pos], np.uint32(0))
        return out

    def candidates(self):
        """(g int64 [n, 3], words uint32 [n]) of every voxel of the map with w > 0"""
        gs, ws = [self.sg], [self.sw]
        if self.vol is not None:
            k, j, i = np.nonzero(W.seen(self.words))
            gs.append(np.stack([i, j, k], axis=1) + self.lo)
            ws.append(self.words[k, j, i])
        return np.concatenate(gs), np.concatenate(ws)


def frame(store_params, vol=None, anchor=None):
    """-> (A int tuple, O float32 [3], voxel float32): store_params = (voxel, origin0) of the store"""
    voxel, origin0 = F(store_params[0]), np.asarray(store_params[1], np.float32)
    if anchor is None:
        anchor = H.state(vol)[1] if vol is not None else (0, 0, 0)
    anchor = tuple(int(x) for x in anchor)
    assert all(abs(x) <= 1 << 20 for x in anchor)
    return anchor, H.window_origin(origin0, anchor, voxel), voxel


def _q(words):
    return (np.asarray(words, np.uint32) & np.uint32(0xffff)).astype(np.uint16).view(np.int16)


def _trilinear(m, A, O, inv_voxel, x, y, z, tile_lo=None, trace=None):
    """volume_ref.Volume._trilinear against the map.  tile_lo int64 [n, 3] with trace: the reads whose base lies outside
    the 12^3 tile that starts there (the device reads those through its table) are counted in trace["outside_tile"]."""
    c = [(p - O[a]) * inv_voxel - F(0.5) for a, p in enumerate((x, y, z))]
    b = [np.floor(v) for v in c]
    ok = np.ones(x.shape, bool)
    for a in range(3):
        ok &= np.isfinite(b[a]) & (np.abs(b[a]) < COORD_MAX)
    f = [c[a] - b[a] for a in range(3)]
    base = np.stack([np.where(ok, b[a], 0).astype(np.int64) + A[a] for a in range(3)], axis=1)
    one = F(1.0)
    if trace is not None:
        t = base - tile_lo
        trace["outside_tile"] = trace.get("outside_tile", 0) + int((ok & ((t < 0) | (t > 10)).any(axis=1)).sum())

    def corner(di, dj, dk):
        nonlocal ok
        w = m.at(base + np.array([di, dj, dk], np.int64))
        ok &= (w >> np.uint32(16)) > 0
        return _q(w).astype(np.float32) / F(32767.0)

    def lerp(p, q, t):
        return p * (one - t) + q * t

    c00 = lerp(corner(0, 0, 0), corner(1, 0, 0), f[0])
    c10 = lerp(corner(0, 1, 0), corner(1, 1, 0), f[0])
    c01 = lerp(corner(0, 0, 1), corner(1, 0, 1), f[0])
    c11 = lerp(corner(0, 1, 1), corner(1, 1, 1), f[0])
    val = lerp(lerp(c00, c10, f[1]), lerp(c01, c11, f[1]), f[2])
    assert val.dtype == np.float32
    return val, ok


def order_of(g, axis):
    """the device's order: bricks by (bz, by, bx) with b = floor(g / 8), inside a brick 3 * (i + 8 * (j + 8 * k)) + a"""
    b, l = g >> 3, g & 7
    return np.lexsort((axis, l[:, 0], l[:, 1], l[:, 2], b[:, 0], b[:, 1], b[:, 2]))


def dense_order(keys):
    """the permutation that sorts keys [n, 4] = (g_x, g_y, g_z, a) into a dense volume's order"""
    return np.lexsort((keys[:, 3], keys[:, 0], keys[:, 1], keys[:, 2]))


def world_surface(store, store_params, vol=None, min_weight=1, anchor=None, trace=None):
    """-> (xyz float32 [n, 3], nrm float32 [n, 3], keys int32 [n, 4] = (g_x, g_y, g_z, a), crossings), in the device's
    order.  store: {g: word}; store_params: (voxel, origin0) the store was made for; vol: the window, or None.
    trace: a dict that receives counts (added to what it holds); the result does not depend on it."""
    A, O, voxel = frame(store_params, vol, anchor)
    inv_voxel = F(1.0) / voxel
    m = Map(store, vol)
    g, w0 = m.candidates()
    keep = (w0 >> np.uint32(16)) >= min_weight
    g, w0 = g[keep], w0[keep]
    gs, axs, q0s, q1s = [], [], [], []
    for a in range(3):
        e = np.zeros(3, np.int64)
        e[a] = 1
        w1 = m.at(g + e)
        cross = ((w1 >> np.uint32(16)) >= min_weight) & ((_q(w0) < 0) != (_q(w1) < 0))
        gs.append(g[cross])
        axs.append(np.full(int(cross.sum()), a, np.int64))
        q0s.append(_q(w0[cross]))
        q1s.append(_q(w1[cross]))
    g, axis = np.concatenate(gs), np.concatenate(axs)
    order = order_of(g, axis)
    g, axis = g[order], axis[order]
    q0, q1 = np.concatenate(q0s)[order], np.concatenate(q1s)[order]
    n = len(g)
    r = g - np.array(A, np.int64)
    tile_lo = ((g >> 3) << 3) - 2
    assert n == 0 or int(np.abs(r).max()) < 1 << 22
    with np.errstate(all="ignore"):
        F0, F1 = q0.astype(np.float32) / F(32767.0), q1.astype(np.float32) / F(32767.0)
        t = F0 / (F0 - F1)
        P = [O[b] + (r[:, b].astype(np.float32) + F(0.5)) * voxel for b in range(3)]
        for a in range(3):
            P[a] = np.where(axis == a, P[a] + t * voxel, P[a])
        grad, ok = [], np.ones(n, bool)
        for b in range(3):
            hi_p = [P[c] + voxel if c == b else P[c] for c in range(3)]
            lo_p = [P[c] - voxel if c == b else P[c] for c in range(3)]
            v1, ok1 = _trilinear(m, A, O, inv_voxel, *hi_p, tile_lo=tile_lo, trace=trace)
            v0, ok0 = _trilinear(m, A, O, inv_voxel, *lo_p, tile_lo=tile_lo, trace=trace)
            ok &= ok1 & ok0
            grad.append(v1 - v0)
        ln = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]).astype(np.float32)
        has = ok & (ln > F(0)) & (ln <= F(3.0e38))
        nrm = np.stack([grad[b] / ln for b in range(3)], axis=1).astype(np.float32)
    xyz = np.stack(P, axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    assert xyz.dtype == np.float32 and nrm.dtype == np.float32 and t.dtype == np.float32
    keys = np.concatenate([g, axis[:, None]], axis=1).astype(np.int32)
    return np.ascontiguousarray(xyz[has]), np.ascontiguousarray(nrm[has].reshape(-1, 3)), np.ascontiguousarray(keys[has]), n


# ---------------------------------------------------------------- the dense volume the rule is pinned to
def bounds(store, vol=None, margin=3):
    """(lo, hi) int tuples: the box of every voxel of the map with w > 0, grown by margin on every side; None when the
    map holds nothing"""
    g, _ = Map(store, vol).candidates()
    if not len(g):
        return None
    return tuple(int(x) - margin for x in g.min(axis=0)), tuple(int(x) + 1 + margin for x in g.max(axis=0))


def dense(store, store_params, vol, lo, hi, blank):
    """A dense volume_ref.Volume (made by blank(nx, ny, nz, voxel=, origin=)) at offset lo whose words are G over
    lo <= g < hi, as shift_ref carries a shifted volume."""
    voxel, origin0 = F(store_params[0]), np.asarray(store_params[1], np.float32)
    n = tuple(int(hi[a]) - int(lo[a]) for a in range(3))
    out = blank(n[0], n[1], n[2], voxel=voxel, origin=origin0)
    out.origin0, out.off = origin0.copy(), tuple(int(x) for x in lo)
    out.origin = H.window_origin(origin0, out.off, voxel)
    k, j, i = np.indices((n[2], n[1], n[0]))
    g = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.int64) + np.array(lo, np.int64)
    W.set_words(out, Map(store, vol).at(g).reshape(n[2], n[1], n[0]))
    return out
