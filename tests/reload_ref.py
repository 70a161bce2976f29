"""Numpy restatement of the voxel store and of the shift through it (include/oslam.h at oslam_volume_shift_world): the
yardstick of the device path and of the library's store.

The rule.  A window voxel (i, j, k) of a volume with offset off has the global coordinate g = (i + off_x, j + off_y,
k + off_z).  A word is seen iff word >> 16 != 0, and only seen words are ever stored.  Voxel (i, j, k) leaves under the
shift s iff not (0 <= i - s_x < nx and likewise for y and z); new voxel (i, j, k) enters iff its source (i + s_x, j + s_y,
k + s_z) does not exist in the old window.  The shift with a store: every seen leaving voxel goes into the store under its
g (overwriting a key already there); the window moves as shift_ref.shifted moves it; every store entry whose g lies in
the entering region is removed from the store and written to its voxel, which the plain shift left at 0.

The store here is a dict {(gx, gy, gz): word}, changed in place.  Volumes are volume_ref.Volume as shift_ref carries
them (origin0, off).  numpy only.
"""
import numpy as np

import shift_ref as H


def words_of(vol):
    """uint32 [nz, ny, nx]: int16 q | uint16 w << 16"""
    return vol.q.view(np.uint16).astype(np.uint32) | (vol.w.astype(np.uint32) << np.uint32(16))


def set_words(vol, words):
    words = np.asarray(words, np.uint32)
    vol.q = (words & np.uint32(0xffff)).astype(np.uint16).view(np.int16)
    vol.w = (words >> np.uint32(16)).astype(np.uint16)
    return vol


def seen(words):
    return (np.asarray(words, np.uint32) >> np.uint32(16)) != 0


def _outside(vol, s, sign):
    """bool [nz, ny, nx]: index + sign * s lies outside the window on some axis"""
    out = np.zeros(vol.q.shape, bool)
    for a, ax in ((0, 2), (1, 1), (2, 0)):                           # the arrays are [nz, ny, nx]
        c = np.arange(vol.n[a]) + sign * int(s[a])
        bad = (c < 0) | (c >= vol.n[a])
        shape = [1, 1, 1]
        shape[ax] = vol.n[a]
        out |= bad.reshape(shape)
    return out


def leaves(vol, s):
    """bool [nz, ny, nx]: the voxel is outside the window after a shift by s"""
    return _outside(vol, s, -1)


def enters(vol, s):
    """bool [nz, ny, nx]: the new voxel's source does not exist in the old window"""
    return _outside(vol, s, +1)


def packed(vol, s):
    """-> (lin uint32 [n], words uint32 [n]): the seen voxels that leave under s, ascending lin = (k * ny + j) * nx + i"""
    words = words_of(vol)
    if not any(int(x) for x in s):
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    lin = np.flatnonzero((leaves(vol, s) & seen(words)).ravel())
    return lin.astype(np.uint32), words.ravel()[lin]


def global_of(vol, lin):
    """int64 [n, 3]: g of the window's voxels lin"""
    nx, ny, _ = vol.n
    lin = np.asarray(lin, np.int64)
    off = H.state(vol)[1]
    return np.stack([lin % nx + off[0], lin // nx % ny + off[1], lin // (nx * ny) + off[2]], axis=1)


def window_entries(vol):
    """{g: word} of the window's seen voxels"""
    words = words_of(vol).ravel()
    lin = np.flatnonzero(seen(words))
    return dict(zip(map(tuple, global_of(vol, lin).tolist()), words[lin].tolist()))


def shift_world(vol, store, s):
    """-> (vol', stored, reloaded); store is changed in place.  A zero shift changes nothing."""
    s = [int(x) for x in s]
    if not any(s):
        return vol, 0, 0
    lin, words = packed(vol, s)
    out = H.shifted(vol, s)
    assert out is not None, "a shift or an offset beyond 2^20"
    store.update(zip(map(tuple, global_of(vol, lin).tolist()), words.tolist()))
    reloaded = 0
    if store:
        keys = np.array(list(store.keys()), np.int64).reshape(-1, 3)
        ijk = keys - np.array(out.off, np.int64)
        inside = ((ijk >= 0) & (ijk < np.array(vol.n, np.int64))).all(axis=1)
        keys, ijk = keys[inside], ijk[inside]
        pick = enters(vol, s)[ijk[:, 2], ijk[:, 1], ijk[:, 0]]
        new = words_of(out)
        for g, (i, j, k) in zip(map(tuple, keys[pick].tolist()), ijk[pick].tolist()):
            assert new[k, j, i] == 0
            new[k, j, i] = store.pop(g)
            reloaded += 1
        set_words(out, new)
    return out, len(lin), reloaded


def box(store, lo, hi):
    """uint32 [hz - lz, hy - ly, hx - lx]: the stored words with lo <= g < hi, 0 where nothing is stored"""
    lo, hi = [int(x) for x in lo], [int(x) for x in hi]
    out = np.zeros((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), np.uint32)
    for g, word in store.items():
        if all(lo[a] <= g[a] < hi[a] for a in range(3)):
            out[g[2] - lo[2], g[1] - lo[1], g[0] - lo[0]] = word
    return out


def window_box(vol):
    """(lo, hi) of the window in global coordinates"""
    off = H.state(vol)[1]
    return tuple(off), tuple(off[a] + vol.n[a] for a in range(3))
