"""Numpy restatement of the colour at points of the whole map, colour store plus coloured window (include/oslam.h at
oslam_world_colours): the yardstick of the device path.  It builds on world_surface_ref (the map as a lookup, the frame)
and colour_ref (the rule at a point, whose float sequence is repeated here against the map).

The map.  Gc(g) is a colour word for every global voxel coordinate g: inside the window's box the window's colour word,
elsewhere the store's colour word, or 0.  A store entry inside the window's box is ignored.  Without a volume the store
stands alone.  The frame is world_surface_ref.frame's: anchor A, O = origin(A).

The rule is colour_ref.Volume.colour_at's: u = (P - O) * inv_voxel, c = u - 0.5, b = floor(c), f = c - b; the range test
on b is "finite and |b| < 2^22"; the eight corners are Gc at A + b + (0|1); with all eight wc > 0 the channels are blended,
rounded and clipped; otherwise the voxel A + floor(u), under the same range test, gives its colour if its wc > 0; otherwise
there is none.  The store is reload_colour_ref's two dicts {g: word} and {g: colour word}.  numpy only.
"""
import copy

import numpy as np

import colour_ref as CR
import reload_ref as W
import world_surface_ref as WS

F = np.float32
U = np.uint32


def colour_map(store, cstore, vol=None):
    """Gc as a world_surface_ref.Map: the colours of the store's keys, and the window's colour words over its box"""
    shim = None
    if vol is not None:
        shim = W.set_words(copy.copy(vol), np.asarray(vol.c, U))     # words_of(shim) is vol.c
    return WS.Map({g: cstore[g] for g in store}, shim)


def colour_at(store, cstore, store_params, P, vol=None, anchor=None):
    """The image word of the colour at each volume-frame point of P float32 [n, 3]: a = 255, or the word 0."""
    A, O, voxel = WS.frame(store_params, vol, anchor)
    inv_voxel = F(1.0) / voxel
    m = colour_map(store, cstore, vol)
    P = np.asarray(P, np.float32).reshape(-1, 3)
    out = np.zeros(len(P), U)
    if not len(P):
        return out
    with np.errstate(all="ignore"):
        u = [(P[:, a] - O[a]) * inv_voxel for a in range(3)]
        c = [u[a] - F(0.5) for a in range(3)]
        b = [np.floor(v) for v in c]
        tri = np.ones(len(P), bool)
        for a in range(3):
            tri &= np.isfinite(b[a]) & (np.abs(b[a]) < WS.COORD_MAX)
        f = [c[a] - b[a] for a in range(3)]
        base = np.stack([np.where(tri, b[a], 0).astype(np.int64) + A[a] for a in range(3)], axis=1)
        corner = [m.at(base + np.array([di, dj, dk], np.int64)) for dk in (0, 1) for dj in (0, 1) for di in (0, 1)]   # x fastest
        for w in corner:
            tri &= (w >> U(24)) != 0
        one = F(1.0)

        def lerp(p, q, t):
            return p * (one - t) + q * t

        word = np.full(len(P), 0xff000000, U)
        for sh in (0, 8, 16):
            v = [((w >> U(sh)) & U(255)).astype(np.float32) for w in corner]
            c00, c10 = lerp(v[0], v[1], f[0]), lerp(v[2], v[3], f[0])
            c01, c11 = lerp(v[4], v[5], f[0]), lerp(v[6], v[7], f[0])
            val = np.floor(lerp(lerp(c00, c10, f[1]), lerp(c01, c11, f[1]), f[2]) + F(0.5))
            assert val.dtype == np.float32
            word |= np.clip(np.where(tri, val, 0), 0, 255).astype(U) << U(sh)
        out[tri] = word[tri]
        # otherwise the voxel that holds the point, looked up on its own
        n = [np.floor(u[a]) for a in range(3)]
        inr = ~tri
        for a in range(3):
            inr &= np.isfinite(n[a]) & (np.abs(n[a]) < WS.COORD_MAX)
        near = np.stack([np.where(inr, n[a], 0).astype(np.int64) + A[a] for a in range(3)], axis=1)
        w = m.at(near)
        inr &= (w >> U(24)) != 0
        out[inr] = w[inr] | U(0xff000000)
    return out


def colours(store, cstore, store_params, P, vol=None, anchor=None):
    """oslam_world_colours: -> (rgb uint8 [n, 3], valid bool [n])"""
    return CR.unpack(colour_at(store, cstore, store_params, P, vol, anchor))


def coloured_bounds(store, cstore, vol=None):
    """(lo, hi) int tuples: the box of every voxel of the map with wc > 0 and of every voxel with w > 0, with no margin;
    None when the map holds neither"""
    gs = [WS.Map(store, vol).candidates()[0]]
    m = colour_map(store, cstore, vol)
    gs.append(m.sg[(m.sw >> U(24)) != 0])
    if vol is not None:
        k, j, i = np.nonzero((np.asarray(vol.c, U) >> U(24)) != 0)
        gs.append(np.stack([i, j, k], axis=1) + m.lo)
    g = np.concatenate(gs)
    if not len(g):
        return None
    return tuple(int(x) for x in g.min(axis=0)), tuple(int(x) + 1 for x in g.max(axis=0))


def dense(store, cstore, store_params, vol, lo, hi, blank):
    """Pin (a): a dense coloured volume (made by blank(nx, ny, nz, voxel=, origin=), a colour_ref.Volume) at offset lo
    that holds G and Gc over lo <= g < hi.  colour_ref.Volume.colours on it gives the bytes of colours() with anchor lo at
    every point when the box contains every coloured voxel of the map: outside it both read "uncoloured"."""
    out = WS.dense(store, store_params, vol, lo, hi, blank)
    n = tuple(int(hi[a]) - int(lo[a]) for a in range(3))
    k, j, i = np.indices((n[2], n[1], n[0]))
    g = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.int64) + np.array(lo, np.int64)
    out.c = colour_map(store, cstore, vol).at(g).reshape(n[2], n[1], n[0]).astype(U)
    return out
