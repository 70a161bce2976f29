"""Numpy restatement of the colour store and of the shift of a coloured volume through it (include/oslam.h at
oslam_volume_shift_world, "Colour"): the yardstick of the device path and of the library's colour store.  It builds on
reload_ref (the store of TSDF words) and colour_ref (the coloured volume and its plain shift).

The rule.  A colour store keeps a colour word next to every TSDF word it keeps: the voxel's colour word, as it is,
whenever the voxel's TSDF word is stored, and that means seen voxels (w > 0) only, whatever their wc.  The colour of an
unseen voxel that leaves is dropped.  A record that is reloaded brings its colour word back to its voxel, which the plain
shift of the colours left at 0.  So over a path of shifts that returns to an earlier offset, with no integration in
between, the colour words of the window's seen voxels come back bit for bit; the colour word of an unseen voxel is kept
while the voxel stays in the window and is 0 once it has left.

The store here is two dicts with the same keys, {g: word} (reload_ref's) and {g: colour word}, changed in place.
Volumes are colour_ref.Volume (or anything with q, w, c and n) as shift_ref carries them.  numpy only.
"""
import numpy as np

import colour_ref as CR
import reload_ref as W
import shift_ref as H

U = np.uint32


def put(store, cstore, g, words, colours=None):
    """oslam_world_put / oslam_world_put_colour on the two dicts: unseen words are skipped, a later record wins, colour
    included; without colours the colour kept is 0."""
    words = [int(x) for x in words]
    colours = [0] * len(words) if colours is None else [int(x) for x in colours]
    for gg, word, col in zip(g, words, colours):
        if word >> 16:
            gg = tuple(int(x) for x in gg)
            store[gg] = word
            cstore[gg] = col


def packed(vol, s):
    """-> (lin, words, colours), uint32 [n] each: reload_ref.packed with each record's colour word"""
    lin, words = W.packed(vol, s)
    return lin, words, np.asarray(vol.c, U).ravel()[lin.astype(np.int64)]


def shift_world(vol, store, cstore, s):
    """-> (vol', stored, reloaded); both dicts are changed in place.  A zero shift changes nothing."""
    s = [int(x) for x in s]
    if not any(s):
        return vol, 0, 0
    assert set(store) == set(cstore)
    lin, _, cols = packed(vol, s)
    cstore.update(zip(map(tuple, W.global_of(vol, lin).tolist()), cols.tolist()))
    out, stored, reloaded = W.shift_world(vol, store, s)
    out.c = CR.shifted(vol, s).c
    back = [g for g in cstore if g not in store]
    assert len(back) == reloaded and stored == len(lin)
    for g in back:
        i, j, k = (g[a] - out.off[a] for a in range(3))
        assert out.c[k, j, i] == 0
        out.c[k, j, i] = cstore.pop(g)
    return out, stored, reloaded


def box(store, cstore, lo, hi):
    """-> (words, colours), uint32 [hz - lz, hy - ly, hx - lx] each, 0 where nothing is stored"""
    return W.box(store, lo, hi), W.box({g: cstore[g] for g in store}, lo, hi)


def restored(vol, path):
    """The colour words a path of shifts through a colour store that returns to its start leaves: the original colour
    word where the voxel is seen; where it is not, the original if the voxel stayed in the window all the way and 0 if it
    ever left (test_reload_host.restored's rule for the TSDF words, applied to the colours)."""
    plain = vol
    for s in path:
        plain = CR.shifted(plain, s)
    assert H.state(plain)[1] == H.state(vol)[1]
    return np.where(W.seen(W.words_of(vol)), vol.c, plain.c).astype(U)
