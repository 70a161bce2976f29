"""Numpy restatement of the ray cast of the whole map, voxel store plus window (include/oslam.h at oslam_world_raycast):
the yardstick of the device path.

The march is volume_ref.Volume.raycast's, float32 in the header's order, with the header's four substitutions: the map
and its frame are world_surface_ref's (Map, frame, _trilinear: G(g), the anchor A, O = origin(A), the range test "finite
and |b| < 2^22"); the slab comes from a box B = [box_lo, box_hi) in global voxels, lo = O_a + float32(r_lo + 1) * voxel and
hi = O_a + float32(r_hi - 1) * voxel with r = box - A, by default the bounding box of the map's bricks; a sample is G at
A + floor((P - O) * inv_voxel) under the same range test; the march runs while t_k <= tf and k < 65536.  The z image, the
maps and the two counts equal the device's byte for byte.

Here too: the paint restatement (colour_ref.Volume.paint's vertex and transform, world_colour_ref's colour at the point)
and the track glue over camera_ref.egomotion.  The store is reload_ref's dict {(gx, gy, gz): word}; volumes are
volume_ref.Volume as shift_ref carries them.  numpy only.
"""
import numpy as np

import camera_ref as E
import reload_ref as W
import shift_ref as H
import volume_ref as V
import world_colour_ref as WC
import world_surface_ref as WS

F = np.float32
U = np.uint32
MAX_STEPS = 65536
BOX_MAX = (1 << 20) + 520
EXITS = ("zero_miss", "empty", "exhausted", "back_face", "trilinear", "den", "off_bracket", "z_cut", "no_normal", "hit")


def window_bricks(vol):
    """(first brick, number of bricks) per axis of the aligned 8^3 bricks the window's box overlaps"""
    off = H.state(vol)[1]
    kb0 = [off[a] >> 3 for a in range(3)]
    return kb0, [((off[a] + vol.n[a] - 1) >> 3) - kb0[a] + 1 for a in range(3)]


def table(store, vol=None):
    """int64 [n, 3]: the brick coordinates floor(g / 8) of the device's table, the store's bricks united with the
    window's (a store entry inside the window's box keeps its brick: the window's bricks hold it anyway)"""
    parts = []
    if store:
        parts.append(np.array(list(store.keys()), np.int64).reshape(-1, 3) >> 3)
    if vol is not None:
        kb0, nb = window_bricks(vol)
        k, j, i = np.indices((nb[2], nb[1], nb[0]))
        parts.append(np.stack([i.ravel() + kb0[0], j.ravel() + kb0[1], k.ravel() + kb0[2]], axis=1).astype(np.int64))
    return np.unique(np.concatenate(parts), axis=0) if parts else np.zeros((0, 3), np.int64)


def default_box(store, vol=None):
    """(lo, hi) int tuples: the bounding box of the table's bricks, None for an empty map"""
    b = table(store, vol)
    if not len(b):
        return None
    return tuple(int(8 * x) for x in b.min(axis=0)), tuple(int(8 * (x + 1)) for x in b.max(axis=0))


def steps_refused(cam, mu):
    """the host's OSLAM_E_LIMIT: (double)(z_max - z_min) / (double)step >= 65535"""
    step = F(0.5) * F(mu)
    return float(F(cam["z_max"]) - F(cam["z_min"])) / float(step) >= 65535.0


class _Reader:
    """the reads of the march against the map, with the counters of a trace"""

    def __init__(self, store, store_params, vol, anchor, trace):
        self.A, self.O, self.voxel = WS.frame(store_params, vol, anchor)
        self.inv_voxel = F(1.0) / self.voxel
        self.m = WS.Map(store, vol)
        self.trace = trace
        self.vol = vol
        if vol is not None:
            self.wlo = np.array(H.state(vol)[1], np.int64)
            self.wn = np.array(vol.n, np.int64)
        if trace is not None:
            b = table(store, vol)
            self.bricks = np.sort(WS._pack(b)) if len(b) else np.zeros(0, np.int64)

    def present(self, g):
        """bool [n]: the brick of g has a table entry"""
        if not len(self.bricks):
            return np.zeros(len(g), bool)
        k = WS._pack(g >> 3)
        pos = np.minimum(np.searchsorted(self.bricks, k), len(self.bricks) - 1)
        return self.bricks[pos] == k

    def nearest(self, x, y, z):
        """(F, w, g int64 [n, 3], in range) of the voxel that holds each volume-frame point; w = 0 outside the range"""
        c = [np.floor((p - self.O[a]) * self.inv_voxel) for a, p in enumerate((x, y, z))]
        inr = np.ones(x.shape, bool)
        for a in range(3):
            inr &= np.isfinite(c[a]) & (np.abs(c[a]) < WS.COORD_MAX)
        g = np.stack([np.where(inr, c[a], 0).astype(np.int64) + self.A[a] for a in range(3)], axis=1)
        word = np.where(inr, self.m.at(g), U(0)).astype(U)
        return WS._q(word).astype(np.float32) / F(32767.0), word >> U(16), g, inr

    def trilinear(self, x, y, z):
        """(value, has a value, mixed): world_surface_ref._trilinear; mixed = the eight corners hold a word from inside
        the window's box and a seen word from outside it"""
        val, ok = WS._trilinear(self.m, self.A, self.O, self.inv_voxel, x, y, z)
        mixed = np.zeros(x.shape, bool)
        if self.trace is not None:
            c = [(p - self.O[a]) * self.inv_voxel - F(0.5) for a, p in enumerate((x, y, z))]
            b = [np.floor(v) for v in c]
            inr = np.ones(x.shape, bool)
            for a in range(3):
                inr &= np.isfinite(b[a]) & (np.abs(b[a]) < WS.COORD_MAX)
            base = np.stack([np.where(inr, b[a], 0).astype(np.int64) + self.A[a] for a in range(3)], axis=1)
            self.trace["cross_brick"] = self.trace.get("cross_brick", 0) + int((inr & ((base & 7) == 7).any(axis=1)).sum())
            if self.vol is not None:
                win, sto = np.zeros(x.shape, bool), np.zeros(x.shape, bool)
                for d in np.ndindex(2, 2, 2):
                    g = base + np.array(d[::-1], np.int64)
                    inside = ((g >= self.wlo) & (g < self.wlo + self.wn)).all(axis=1)
                    win |= inside
                    sto |= ~inside & ((self.m.at(g) >> U(16)) != 0)
                mixed = inr & win & sto
        return val, ok, mixed


def raycast(store, store_params, T_vol_cam, cam, width, height, vol=None, anchor=None, box=None, mu=None, trace=None):
    """oslam_world_raycast: -> (z float32 [h, w], (V, N, has) as track_ref.view_maps, dict hits normals anchor box_lo
    box_hi).  store: {g: word}; store_params: (voxel, origin0) the store was made for; vol: the window, or None; mu None:
    the volume's.
    trace: a dict that receives the number of rays per exit reason as volume_ref.Volume.raycast counts them, "max_step",
    "gap_then_hit", "exit" ([h, w] of str) and, added to what it holds: "mixed_stencil", the hits whose crossing or
    gradient stencils read corners from both the store and the window; "cross_brick", the trilinear reads whose base has
    a local coordinate of 7; "absent_after_present", the samples in a brick without a table entry that follow a sample
    of the same ray in a brick with one; "samples", all samples in range.  The result does not depend on it."""
    rd = _Reader(store, store_params, vol, anchor, trace)
    A, O, voxel = rd.A, rd.O, rd.voxel
    mu = F(vol.mu) if mu is None else F(mu)
    shape = (height, width)
    n = width * height
    if box is None:
        box = default_box(store, vol)
    if box is None:                                                   # an empty map: a view of zeros
        out = dict(hits=0, normals=0, anchor=A, box_lo=(0, 0, 0), box_hi=(0, 0, 0))
        return np.zeros(shape, np.float32), (np.zeros(shape + (3,), np.float32), np.zeros(shape + (3,), np.float32),
                                             np.zeros(shape, bool)), out
    lo_g, hi_g = tuple(int(x) for x in box[0]), tuple(int(x) for x in box[1])
    assert all(hi_g[a] - lo_g[a] >= 2 and abs(lo_g[a]) <= BOX_MAX and abs(hi_g[a]) <= BOX_MAX for a in range(3))
    assert not steps_refused(cam, mu)
    M = np.asarray(T_vol_cam, np.float32).reshape(4, 4)
    fx, fy, cx, cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
    z_min, z_max = F(cam["z_min"]), F(cam["z_max"])
    u = np.arange(width, dtype=np.float32)[None, :]
    v = np.arange(height, dtype=np.float32)[:, None]
    dx = np.broadcast_to((u - cx) / fx, shape).reshape(-1).astype(np.float32)
    dy = np.broadcast_to((v - cy) / fy, shape).reshape(-1).astype(np.float32)
    o = M[:3, 3]
    D = [(M[a, 0] * dx + M[a, 1] * dy) + M[a, 2] for a in range(3)]
    tn, tf = np.full(n, z_min, np.float32), np.full(n, z_max, np.float32)
    miss = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo = O[a] + F(F(lo_g[a] - A[a] + 1) * voxel)
            hi = O[a] + F(F(hi_g[a] - A[a] - 1) * voxel)
            zero = D[a] == F(0)
            miss |= zero & ~((o[a] >= lo) & (o[a] <= hi))
            ta, tb = (lo - o[a]) / D[a], (hi - o[a]) / D[a]
            tn = np.where(zero, tn, np.maximum(tn, np.minimum(ta, tb)))
            tf = np.where(zero, tf, np.minimum(tf, np.maximum(ta, tb)))
        active = ~miss & (tn <= tf)
    why = np.full(n, "exhausted", dtype="U16") if trace is not None else None
    if trace is not None:
        any_zero = (D[0] == F(0)) | (D[1] == F(0)) | (D[2] == F(0))
        why[miss] = "zero_miss"
        why[~miss & ~active] = "empty"
        gap = np.zeros(n, bool)
        mixed = np.zeros(n, bool)
        prev_present = np.zeros(n, bool)                              # the ray's last sample in range lay in a table brick
        tr = dict(zero_inside=int((any_zero & ~miss).sum()), zero_marched=int((any_zero & active).sum()),
                  absent_after_present=0, samples=0, max_step=-1)
    step = F(0.5) * mu
    have = np.zeros(n, bool)
    Fp, tp, ts = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for k in range(MAX_STEPS):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        t = tn[idx] + F(k) * step
        alive = t <= tf[idx]
        active[idx[~alive]] = False
        idx, t = idx[alive], t[alive]
        if idx.size == 0:
            continue
        x, y, zz = (o[a] + D[a][idx] * t for a in range(3))
        Fc, w, g, inr = rd.nearest(x, y, zz)
        seen = w > 0
        if trace is not None:
            tr["max_step"] = k
            gap[idx[~seen & have[idx]]] = True
            here = rd.present(g)
            tr["samples"] += int(inr.sum())
            tr["absent_after_present"] += int((inr & ~here & prev_present[idx]).sum())
            prev_present[idx[inr]] = here[inr]
        have[idx[~seen]] = False
        cross = seen & have[idx] & (Fp[idx] > F(0)) & (Fc < F(0))
        back = seen & ~cross & have[idx] & (Fp[idx] < F(0)) & (Fc > F(0))
        rest = seen & ~cross & ~back
        active[idx[cross | back]] = False
        if trace is not None:
            why[idx[back]] = "back_face"
        ic = idx[cross]
        if ic.size:
            tpc, tc = tp[ic], t[cross]
            Ft, ok0, m0 = rd.trilinear(*(o[a] + D[a][ic] * tpc for a in range(3)))
            Ftdt, ok1, m1 = rd.trilinear(x[cross], y[cross], zz[cross])
            with np.errstate(all="ignore"):
                den = Ftdt - Ft
                tstar = tpc - (step * Ft) / den
                good = ok0 & ok1 & (den < F(0)) & (tstar >= tpc) & (tstar <= tc) & (tstar >= z_min) & (tstar <= z_max)
            ts[ic[good]] = tstar[good]
            if trace is not None:
                mixed[ic] |= m0 | m1
                with np.errstate(all="ignore"):
                    for name, m in (("z_cut", ~((tstar >= z_min) & (tstar <= z_max))),
                                    ("off_bracket", ~((tstar >= tpc) & (tstar <= tc))), ("den", ~(den < F(0))),
                                    ("trilinear", ~(ok0 & ok1)), ("hit", good)):       # the first that fails names it
                        why[ic[m]] = name
        ir = idx[rest]
        have[ir] = True
        Fp[ir] = Fc[rest]
        tp[ir] = t[rest]
    assert not active.any()
    hit = ts > F(0)
    ih = np.flatnonzero(hit)
    Vx, N, has = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
    if ih.size:
        t = ts[ih]
        p = [o[a] + D[a][ih] * t for a in range(3)]
        g, ok = [], np.ones(ih.size, bool)
        for a in range(3):
            hi_p = [p[b] + voxel if b == a else p[b] for b in range(3)]
            lo_p = [p[b] - voxel if b == a else p[b] for b in range(3)]
            v1, ok1, m1 = rd.trilinear(*hi_p)
            v0, ok0, m0 = rd.trilinear(*lo_p)
            ok &= ok1 & ok0
            g.append(v1 - v0)
            if trace is not None:
                mixed[ih] |= m1 | m0
        with np.errstate(all="ignore"):
            ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(np.float32)
            ok &= (ln > F(0)) & (ln <= F(3.0e38))
            nv = [g[a] / ln for a in range(3)]
            nc = [(M[0, a] * nv[0] + M[1, a] * nv[1]) + M[2, a] * nv[2] for a in range(3)]
            vx, vy = dx[ih] * t, dy[ih] * t
            ok &= ((nc[0] * vx + nc[1] * vy) + nc[2] * t) < F(0)
        sel = ih[ok]
        has[sel] = True
        Vx[sel] = np.stack([vx[ok], vy[ok], t[ok]], axis=1)
        N[sel] = np.stack([nc[0][ok], nc[1][ok], nc[2][ok]], axis=1)
        assert Vx.dtype == np.float32 and N.dtype == np.float32
    if trace is not None:
        why[hit & ~has] = "no_normal"
        tr["gap_then_hit"] = int((gap & hit).sum())
        tr["mixed_stencil"] = int((mixed & hit).sum())
        for name in EXITS:
            tr[name] = int((why == name).sum())
        for key, val in tr.items():
            trace[key] = max(trace.get(key, -1), val) if key == "max_step" else trace.get(key, 0) + val
        trace["exit"] = why.reshape(shape)
    return ts.reshape(shape), (Vx.reshape(shape + (3,)), N.reshape(shape + (3,)), has.reshape(shape)), \
        dict(hits=int(hit.sum()), normals=int(has.sum()), anchor=A, box_lo=lo_g, box_hi=hi_g)


def paint(store, cstore, store_params, z, cam, T_vol_cam, vol=None, anchor=None):
    """oslam_world_paint_view over the z image of a view: colour_ref.Volume.paint's vertex and transform, the colour of
    world_colour_ref.colour_at there.  -> the view's colour image, uint32 [h, w]"""
    M = np.asarray(T_vol_cam, np.float32).reshape(4, 4)
    h, w = z.shape
    fx, fy, cx, cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
    dx = (np.arange(w, dtype=np.float32)[None, :] - cx) / fx
    dy = (np.arange(h, dtype=np.float32)[:, None] - cy) / fy
    z = np.asarray(z, np.float32)
    vx, vy = dx * z, dy * z
    P = np.stack([((M[a, 0] * vx + M[a, 1] * vy) + M[a, 2] * z) + M[a, 3] for a in range(3)], axis=-1)
    assert P.dtype == np.float32
    word = WC.colour_at(store, cstore, store_params, P.reshape(-1, 3), vol, anchor).reshape(h, w)
    return np.where(z > F(0), word, U(0)).astype(U)


def track(store, store_params, frame_maps, cam, T_prev, vol=None, anchor=None, box=None, mu=None, sums="f64", **kw):
    """oslam_world_track: volume_ref.Volume.track with the whole map's ray cast at its head.  -> (T_vol_cam float32 4x4,
    the egomotion result dict)"""
    h, w = frame_maps[2].shape
    _, model, _ = raycast(store, store_params, T_prev, cam, w, h, vol, anchor, box, mu)
    T, r = E.egomotion(frame_maps, model, cam, sums=sums, **kw)
    return V.compose(T_prev, T), r


def window_box(vol):
    return W.window_box(vol)
