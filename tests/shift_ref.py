"""Numpy restatement of the shifting window (include/oslam.h at oslam_volume_shift): the yardstick of the device path.

A shifted volume is a volume_ref.Volume that carries origin0 (the origin it was created with) and off (the window's
offset in voxels); its origin is derived from the two by the header's rule, never accumulated.  The surface that a shift
loses is built on mesh_ref.vertices, surface_ref's crossings with their keys 3 * voxel + axis.  numpy only.
"""
import copy

import numpy as np

import mesh_ref as M

F = np.float32
SHIFT_MAX = 1 << 20


def window_origin(origin0, off, voxel):
    """origin0_a itself where off_a == 0 (a -0.0 keeps its sign), else origin0_a + float32(off_a) * voxel: one float32
    multiply, then one float32 add."""
    origin0 = np.asarray(origin0, np.float32)
    out = origin0.copy()
    for a in range(3):
        if off[a] != 0:
            out[a] = origin0[a] + F(F(off[a]) * F(voxel))
    assert out.dtype == np.float32
    return out


def state(vol):
    """(origin0, off) of a volume_ref.Volume, shifted or not"""
    return getattr(vol, "origin0", vol.origin).copy(), tuple(getattr(vol, "off", (0, 0, 0)))


def shifted(vol, s):
    """A copy of vol with the window moved by s = (sx, sy, sz): the new word at (i, j, k) is the old word at
    (i + sx, j + sy, k + sz) where that voxel exists and 0 elsewhere; off += s.  None where the device refuses (a shift
    or an offset beyond 2^20)."""
    s = [int(x) for x in s]
    origin0, off = state(vol)
    new_off = tuple(off[a] + s[a] for a in range(3))
    if any(abs(x) > SHIFT_MAX for x in s) or any(abs(x) > SHIFT_MAX for x in new_off):
        return None
    out = copy.copy(vol)
    out.origin0, out.off = origin0, new_off
    out.origin = window_origin(origin0, new_off, vol.voxel)
    out.q, out.w = np.zeros_like(vol.q), np.zeros_like(vol.w)
    dst, src = [], []
    for a in (2, 1, 0):                                         # the arrays are [nz, ny, nx]
        n = vol.n[a]
        lo, hi = max(0, -s[a]), min(n, n - s[a])                # destination indices whose source index + s exists
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + s[a], hi + s[a]))
    out.q[tuple(dst)] = vol.q[tuple(src)]
    out.w[tuple(dst)] = vol.w[tuple(src)]
    return out


def kept(vol):
    return int((vol.w > 0).sum())


def stays(vol, ijk, s):
    """bool [n]: voxel ijk [n, 3] is inside the window after a shift by s"""
    ok = np.ones(len(ijk), bool)
    for a in range(3):
        ok &= (ijk[:, a] - int(s[a]) >= 0) & (ijk[:, a] - int(s[a]) < vol.n[a])
    return ok


def leaving_keys(vol, key, s):
    """bool [n]: the crossing with key 3 * voxel + axis leaves under a shift by s: its start voxel or its neighbour along
    the axis does"""
    nx, ny, _ = vol.n
    lin, a = key // 3, key % 3
    ijk = np.stack([lin % nx, lin // nx % ny, lin // (nx * ny)], axis=1).astype(np.int64)
    nb = ijk.copy()
    nb[np.arange(len(key)), a] += 1
    return ~(stays(vol, ijk, s) & stays(vol, nb, s))


def leaving(vol, s, min_weight=1, verts=None):
    """-> (xyz float32 [n, 3], nrm float32 [n, 3], crossings): surface_ref.surface restricted to the leaving crossings.
    verts: mesh_ref.vertices(vol, min_weight) where the caller has it already (it does not depend on s).
    mesh_ref.vertices gives every crossing with its key and (0, 0, 0) where it has no normal; those with a normal, in
    order, are surface_ref.surface's points (tests/test_shift_host.py checks that here, tests/test_mesh_host.py there)."""
    key, xyz, nrm = verts if verts is not None else M.vertices(vol, min_weight)
    if not len(key):
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0
    gone = leaving_keys(vol, key, s)
    pick = gone & (nrm != 0).any(axis=1)
    return np.ascontiguousarray(xyz[pick]), np.ascontiguousarray(nrm[pick]), int(gone.sum())


def follow_defaults(vol):
    """the fields of oslam_follow_params_default"""
    return dict(lookahead=F(0.5 * vol.n[2] * float(vol.voxel)), threshold=F(min(vol.n)) / F(4.0), granule=8)


def follow(vol, T_vol_cam, lookahead=None, threshold=None, granule=None):
    """oslam_volume_follow in double from the float32 inputs -> (sx, sy, sz)"""
    d = follow_defaults(vol)
    la = float(F(d["lookahead"] if lookahead is None else lookahead))
    th = float(F(d["threshold"] if threshold is None else threshold))
    g = int(d["granule"] if granule is None else granule)
    T = np.asarray(T_vol_cam, np.float32).reshape(4, 4).astype(np.float64)
    h = float(vol.voxel)
    dd = []
    for a in range(3):
        c = T[a, 3] + la * T[a, 2]
        centre = float(vol.origin[a]) + 0.5 * vol.n[a] * h
        dd.append((c - centre) / h)
    if all(abs(x) <= th for x in dd):
        return (0, 0, 0)
    return tuple(int(min(max(g * np.rint(x / g), -vol.n[a]), vol.n[a])) for a, x in enumerate(dd))
