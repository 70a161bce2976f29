"""CPU: colour in the voxel store and the colour of the whole map (include/oslam.h at oslam_volume_shift_world, "Colour",
and at oslam_world_colours).  The library's colour store (csrc/oslam_world.c), which needs no device, against the
restatement of tests/reload_colour_ref.py; the restatements' own invariants; pin (a) of oslam_world_colours on the
restatements alone; every argument check of the new calls on stand-in handles; the colour store linked alone into a small
C program under the address and undefined-behaviour sanitizers; and the calibration.  No call in this file reaches a
device.  Words are 32-bit integers: every comparison but the calibration's is exact.

Calibration (tests/world_colour_calib.py).  The stream, volume and follow parameters of
tests/shift_calib.py with the colour function of tests/colour_world.py, ten frames fused at their true poses on the
restatements, the window following the camera through a colour store and, next to it, through a plain store; then the
colour at every surface point of the whole map against the colour function, per channel, in levels of 255:

    seed   store    surface points   with a colour   median error   95th percentile   shifts   voxels stored
    0      colour   23769            1.0000          1.77           6.85              4        82015
    0      plain    23769            0.7962          1.57           7.84              4        82015
    1      colour   24056            1.0000          1.82           6.41              4        136766
    1      plain    24056            0.4206          0.99           11.77             4        136766
    2      colour   15459            1.0000          1.77           11.07             6        149771
    2      plain    15459            0.8643          1.82           8.33              6        149771

Nothing is reloaded on this walk: the camera turns one way, so the figures measure what the store keeps for the export,
and the bit-for-bit return is the other tests' matter.  The colour store's error is the colour volume's own (DESIGN.md
7t: the colour function's change over a voxel and the band's width); seed 2's 95th percentile is higher than in 7t
because this window is narrower than the room and sees the objects at grazing angles before they leave.  The plain
store's error is over the fewer points it colours, so its columns are not comparable with the colour store's.
The bounds asserted below are a quarter over the colour store's worst seed, as in tests/test_colour_host.py: median <=
1.25 * 1.82, 95th percentile <= 1.25 * 11.07 levels.  That at least 90 % of the map's surface points get a colour through
the colour store is a condition of the test, and the plain store's share must be strictly lower: the difference is what
the colour store is for.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_ref as CR  # noqa: E402
import reload_colour_ref as RC  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_ref as H  # noqa: E402
import surface_ref as S  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import world_colour_calib as CAL  # noqa: E402
import world_colour_ref as WC  # noqa: E402
import world_surface_ref as WS  # noqa: E402

ROOT = TR.ROOT
RAGGED, CHAIN, G_MAX = TR.RAGGED, TR.CHAIN, TR.G_MAX
U = np.uint32
SEEDS = (0, 1, 2)
MEDIAN_BOUND, P95_BOUND, SHARE_MIN = 1.25 * 1.82, 1.25 * 11.07, 0.90
BRICK, COLOUR_BRICK = 2064, 4112


def colour_words(n, seed, unseen_share=0.2):
    """colour words over all 32 bits, [nz, ny, nx], a fifth of them with wc == 0 (and colour bits that must not show)"""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, (n[2], n[1], n[0]), dtype=np.uint64).astype(U)
    words[rng.random(words.shape) < unseen_share] &= U(0xffffff)
    return words


def coloured(vol, seed):
    """vol as a coloured volume of the restatement: c random (colour_words)"""
    vol.c = colour_words(vol.n, seed)
    return vol


def planted(n, seed):
    """test_reload_host.planted with colours.  Its planted unseen voxels (w == 0: near the faces, which leave under the
    shifts used here, and one in the middle, which stays) all get a colour with wc > 0, so both kinds of
    coloured-but-unseen voxel are there; and a seen voxel near a face and one in the middle get wc == 0 with colour bits
    set, the seen-but-uncoloured kind, leaving and staying."""
    vol = coloured(TR.planted(n, seed), seed + 100)
    unseen = np.argwhere(vol.w == 0)
    for k, j, i in unseen:
        vol.c[k, j, i] = U(0x07000000) | U(0x00a1b2c3)
    for i, j, k in [(2, 2, 2), (n[0] // 2 + 1, n[1] // 2, n[2] // 2)]:
        assert vol.w[k, j, i] > 0
        vol.c[k, j, i] = U(0x00332211)
    return vol


def make_world(ppf, colour=True, max_bytes=0, voxel=0.05, origin0=(0.0, 0.0, 0.0)):
    p = ppf.WorldParams()
    p.voxel = voxel
    p.origin0[:] = list(origin0)
    return ppf.World(p, max_bytes=max_bytes, colour=colour)


# ---------------------------------------------------------------- the restatement's invariant
def test_colours_of_seen_voxels_come_back_bit_for_bit():
    vol = planted(RAGGED, 21)
    words0, c0 = W.words_of(vol), vol.c.copy()
    seen, has = W.seen(words0), (c0 >> U(24)) != 0
    # the inputs hold every kind: seen and uncoloured, coloured and unseen, each staying and leaving under the chain
    left = np.zeros(seen.shape, bool)
    cur = vol
    for s in CHAIN:
        ijk = np.argwhere(W.leaves(cur, s)) + np.array(H.state(cur)[1])[::-1]      # global (z, y, x) of what leaves now
        ok = ((ijk >= 0) & (ijk < np.array(seen.shape))).all(axis=1)
        left[tuple(ijk[ok].T)] = True
        cur = CR.shifted(cur, s)
    for kind in (seen & ~has, ~seen & has):
        assert (kind & left).any() and (kind & ~left).any()
    assert (seen & has & left).any() and abs(float((~has).mean()) - 0.2) < 0.02
    store, cstore, cur = {}, {}, vol
    for s in CHAIN:
        lin, rec, cols = RC.packed(cur, s)
        assert cols.tobytes() == cur.c.ravel()[lin.astype(np.int64)].tobytes() and len(cols) == len(lin) == len(rec)
        cur, stored, reloaded = RC.shift_world(cur, store, cstore, s)
        assert set(store) == set(cstore) and stored == len(lin)
        # window and store together hold the colour of every seen voxel exactly once
        g = W.global_of(cur, np.flatnonzero(W.seen(W.words_of(cur)).ravel()))
        both = dict(zip(map(tuple, g.tolist()), cur.c.ravel()[W.seen(W.words_of(cur)).ravel()].tolist()))
        assert not set(both) & set(cstore)
        both.update(cstore)
        k, j, i = np.nonzero(seen)
        assert both == dict(zip(zip(i.tolist(), j.tolist(), k.tolist()), c0[k, j, i].tolist())), s
    assert cur.off == (0, 0, 0) and store == {} and cstore == {}
    assert W.words_of(cur).tobytes() == TR.restored(vol, CHAIN).tobytes()
    want = RC.restored(vol, CHAIN)
    assert cur.c.tobytes() == want.tobytes()
    assert (cur.c[seen] == c0[seen]).all()                          # seen: bit for bit, wc == 0 words included
    assert not cur.c[~seen & left].any() and (cur.c[~seen & ~left] == c0[~seen & ~left]).all()
    # through a plain store the same path loses the colour of everything that left (colour_ref.shifted's statement)
    plain = vol
    for s in CHAIN:
        plain = CR.shifted(plain, s)
    assert (plain.c[seen & left] == 0).all() and (want[seen & left & has] != 0).all()
    # everything leaves and everything returns
    far, stored, _ = RC.shift_world(vol, store, cstore, (RAGGED[0] + 5, -3, 0))
    assert stored == int(seen.sum()) == len(cstore) and not far.c.any()
    back, _, reloaded = RC.shift_world(far, store, cstore, (-RAGGED[0] - 5, 3, 0))
    assert reloaded == stored and cstore == {} and back.c.tobytes() == np.where(seen, c0, 0).astype(U).tobytes()
    assert RC.shift_world(vol, store, cstore, (0, 0, 0)) == (vol, 0, 0)


# ---------------------------------------------------------------- the store through the library
def test_put_then_box_round_trips_colours_across_brick_borders(built_lib, ppf):
    w = make_world(ppf)
    assert w.has_colour() and not make_world(ppf, colour=False).has_colour() and w.params.colour == 1
    edge = [-9, -8, -7, -1, 0, 7, 8]
    g = np.array([(x, y, z) for z in edge for y in edge for x in edge], np.int32)
    words = (np.arange(len(g), dtype=U) + U(1)) << U(16) | U(0xbeef)
    cols = (np.arange(len(g), dtype=U) * U(2654435761)) ^ U(0x5a5a5a5a)
    cols[::5] &= U(0xffffff)                                        # wc == 0: stored as it is
    w.put(g, words, cols)
    store, cstore = {}, {}
    RC.put(store, cstore, g.tolist(), words, cols)
    lo, hi = (-10, -10, -10), (10, 10, 10)
    got, gotc = w.box(lo, hi, colours=True)
    wantw, wantc = RC.box(store, cstore, lo, hi)
    assert got.tobytes() == wantw.tobytes() and gotc.tobytes() == wantc.tobytes() and int((got != 0).sum()) == 343
    assert w.box(lo, hi).tobytes() == wantw.tobytes()               # the plain read of a colour store
    st = w.stats()
    assert (st["voxels"], st["bricks"], st["lo"], st["hi"]) == (343, 64, (-9, -9, -9), (9, 9, 9))
    assert st["bytes"] == 64 * COLOUR_BRICK + 128 * 8
    # the limits of g, on every axis and both signs
    far = np.array([(G_MAX, 0, 0), (-G_MAX, 0, 0), (0, G_MAX, 0), (0, -G_MAX, 0), (0, 0, G_MAX), (0, 0, -G_MAX),
                    (G_MAX, -G_MAX, G_MAX)], np.int32)
    fw = (np.arange(7, dtype=U) + U(500)) << U(16)
    fc = np.arange(7, dtype=U) + U(0xff000001)
    w.put(far, fw, fc)
    for gg, word, col in zip(far.tolist(), fw.tolist(), fc.tolist()):
        a, b = w.box(gg, [c + 1 for c in gg], colours=True)
        assert a.shape == b.shape == (1, 1, 1) and (int(a[0, 0, 0]), int(b[0, 0, 0])) == (word, col), gg
    # a later put wins, colour included, also inside one call; unseen words are skipped and overwrite neither
    w.put([(0, 0, 0), (0, 0, 0), (7, 8, -9)], [5 << 16, 6 << 16 | 1, 0xffff], [111, 222, 333])
    a, b = w.box((0, 0, 0), (1, 1, 1), colours=True)
    assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (6 << 16 | 1, 222)
    a, b = w.box((7, 8, -9), (8, 9, -8), colours=True)
    assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (store[(7, 8, -9)], cstore[(7, 8, -9)]) and w.stats()["voxels"] == 350
    # a plain put on a colour store zeroes the colour
    w.put([(0, 0, 0)], [9 << 16])
    a, b = w.box((0, 0, 0), (1, 1, 1), colours=True)
    assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (9 << 16, 0)
    # take removes the word and its colour: a plain put afterwards finds no stale colour
    a, b = w.box((-9, -9, -9), (-6, -6, -6), take=True, colours=True)
    assert a.tobytes() == RC.box(store, cstore, (-9, -9, -9), (-6, -6, -6))[0].tobytes() and int((b != 0).sum()) > 20
    a, b = w.box((-9, -9, -9), (-6, -6, -6), colours=True)
    assert not a.any() and not b.any()
    w.put([(-9, -9, -9)], [3 << 16])
    a, b = w.box((-9, -9, -9), (-8, -8, -8), colours=True)
    assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (3 << 16, 0)
    w.clear()
    a, b = w.box(lo, hi, colours=True)
    assert w.stats()["voxels"] == w.stats()["bricks"] == 0 and not a.any() and not b.any()
    w.put(g[:5], words[:5], cols[:5])                               # and it still works
    assert w.stats()["voxels"] == 5 and w.box(lo, hi, colours=True)[1].tobytes() == RC.box(*[dict(list(d.items())[:5]) for d in (store, cstore)], lo, hi)[1].tobytes()
    w.close()


def test_bytes_and_max_bytes_count_the_larger_brick(built_lib, ppf):
    LIM = ppf.OSLAM_E_LIMIT
    g = np.array([(8 * b, 0, 0) for b in range(40)], np.int32)
    ones, cols = np.full(40, 1 << 16, U), np.full(40, 0x01020304, U)
    plain = make_world(ppf, colour=False)
    plain.put(g[:39], ones[:39])
    assert plain.stats()["bytes"] == 39 * BRICK + 128 * 8           # a plain store is what it was
    plain.close()
    # 40 bricks need 128 slots: a bound that holds 39 colour bricks and that table refuses the 40th, and nothing changes
    w = make_world(ppf, max_bytes=39 * COLOUR_BRICK + 128 * 8)
    empty = w.stats()
    assert empty["bytes"] == 64 * 8
    with pytest.raises(ppf.OslamError) as e:
        w.put(g, ones, cols)
    assert e.value.code == LIM and "max_bytes" in str(e.value) and w.stats() == empty
    w.put(g[:39], ones[:39], cols[:39])
    before = w.stats()
    assert before["bricks"] == 39 and before["bytes"] == 39 * COLOUR_BRICK + 128 * 8
    with pytest.raises(ppf.OslamError) as e:
        w.put(g[39:], ones[39:], cols[39:])
    assert e.value.code == LIM and w.stats() == before               # the stats and with them the table's size
    with pytest.raises(ppf.OslamError) as e:
        w.put(g[39:], ones[39:])                                    # the plain put of a colour store needs the larger brick too
    assert e.value.code == LIM and w.stats() == before
    w.close()
    # the bound of 39 plain bricks does not hold 39 colour bricks
    w = make_world(ppf, max_bytes=39 * BRICK + 128 * 8)
    with pytest.raises(ppf.OslamError) as e:
        w.put(g[:39], ones[:39], cols[:39])
    assert e.value.code == LIM and w.stats()["bricks"] == 0
    w.put(g[:19], ones[:19], cols[:19])                             # 19 * 4112 + 64 * 8 fits
    assert w.stats()["bytes"] == 19 * COLOUR_BRICK + 64 * 8
    w.close()


def stand_in_volume(ppf, ref, off=(0, 0, 0), colour=False):
    """test_shift_host.stand_in inside zeroed host memory that also covers the colour fields of struct oslam_volume;
    colour: the colour buffer's pointer is set (it is only compared with NULL before a device call)"""
    h = TH.stand_in(ppf, ref, off)
    buf = C.create_string_buffer(4096)
    C.memmove(buf, C.byref(h), C.sizeof(h))
    if colour:
        C.cast(C.byref(buf, C.sizeof(h)), C.POINTER(C.c_void_p))[0] = 0x1000
    return buf


def test_new_calls_reject_bad_arguments_before_touching_a_device(built_lib, ppf):
    L, INV = ppf.lib(), ppf.OSLAM_E_INVALID
    for name in ("oslam_world_has_colour", "oslam_world_put_colour", "oslam_world_box_colour", "oslam_volume_pack_colour",
                 "oslam_world_colours"):
        assert name in ppf._SIGNATURES
    assert C.sizeof(ppf.WorldParams) == 40 and ppf.WorldParams.reserved.offset == 24      # colour is the int at 24

    def err():
        return L.oslam_last_error().decode()

    ref = TH.exact_frame(S.blank(16, 16, 16), voxel=0.02, origin=(-0.0, 0.1, -1.28))
    frame = dict(voxel=0.02, origin0=(-0.0, 0.1, -1.28))
    cw, pw = make_world(ppf, **frame), make_world(ppf, colour=False, **frame)
    p = ppf.WorldParams(voxel=0.1)
    handle = C.c_void_p(0)
    for bad in (2, -1):
        p.colour = bad
        assert L.oslam_world_create(C.byref(p), C.byref(handle)) == INV and not handle.value
    assert L.oslam_world_has_colour(None) == 0 and L.oslam_world_has_colour(pw._h) == 0 and L.oslam_world_has_colour(cw._h) == 1
    # put_colour, box_colour
    g, ww, cc = np.array([[0, 0, 0]], np.int32), np.array([1 << 16], U), np.array([7], U)
    out, outc = np.zeros(8, U), np.zeros(8, U)
    lo, hi = np.zeros(3, np.int32), np.full(3, 2, np.int32)
    P = ppf._p
    assert L.oslam_world_put_colour(None, P(g), P(ww), P(cc), 1) == INV
    assert L.oslam_world_put_colour(cw._h, None, P(ww), P(cc), 1) == L.oslam_world_put_colour(cw._h, P(g), None, P(cc), 1) == INV
    assert L.oslam_world_put_colour(cw._h, P(g), P(ww), None, 1) == INV
    assert L.oslam_world_put_colour(pw._h, P(g), P(ww), P(cc), 1) == INV and "no colour" in err()
    big = np.array([[0, G_MAX + 2, 0]], np.int32)
    assert L.oslam_world_put_colour(cw._h, P(big), P(ww), P(cc), 1) == INV
    assert L.oslam_world_put_colour(cw._h, None, None, None, 0) == 0
    assert L.oslam_world_box_colour(None, P(lo), P(hi), P(out), P(outc), 0) == INV
    assert L.oslam_world_box_colour(pw._h, P(lo), P(hi), P(out), P(outc), 0) == INV and "no colour" in err()
    assert L.oslam_world_box_colour(cw._h, None, P(hi), P(out), P(outc), 0) == L.oslam_world_box_colour(cw._h, P(lo), None, P(out), P(outc), 0) == INV
    assert L.oslam_world_box_colour(cw._h, P(lo), P(hi), None, P(outc), 0) == L.oslam_world_box_colour(cw._h, P(lo), P(hi), P(out), None, 0) == INV
    assert L.oslam_world_box_colour(cw._h, P(hi), P(lo), P(out), P(outc), 0) == INV
    wide = np.array([512, 512, 513], np.int32)
    assert L.oslam_world_box_colour(cw._h, P(lo), P(wide), None, None, 0) == ppf.OSLAM_E_LIMIT and "2^27" in err()
    assert L.oslam_world_box_colour(cw._h, P(lo), P(lo), None, None, 0) == 0                # an empty box reads nothing
    assert cw.stats()["voxels"] == 0 and pw.stats()["voxels"] == 0
    # the shift: a colour store with a volume without colour, before any device call, with nothing changed
    plain_vol, col_vol = stand_in_volume(ppf, ref), stand_in_volume(ppf, ref, colour=True)
    res = ppf.ReloadResult()
    s = np.array([1, 0, 0], np.int32)
    cw.put([(100, 100, 100)], [7 << 16], [9])
    before = cw.stats()
    assert L.oslam_volume_shift_world(plain_vol, cw._h, P(s), C.byref(res)) == INV and "needs a volume with colour" in err()
    assert cw.stats() == before and bytes(plain_vol.raw) == bytes(stand_in_volume(ppf, ref).raw)
    zero = np.zeros(3, np.int32)
    res.launches = 9
    assert L.oslam_volume_shift_world(col_vol, cw._h, P(zero), C.byref(res)) == 0 and res.launches == 0      # a zero shift returns at once
    assert L.oslam_volume_shift_world(plain_vol, cw._h, P(zero), C.byref(res)) == INV       # but not past this refusal
    other = make_world(ppf, voxel=0.021, origin0=frame["origin0"])
    assert L.oslam_volume_shift_world(col_vol, other._h, P(s), C.byref(res)) == INV and "another voxel size" in err()
    # the tap
    n = C.c_size_t(9)
    buf = np.zeros(4, U)
    far = np.array([(1 << 20) + 1, 0, 0], np.int32)
    assert L.oslam_volume_pack_colour(None, P(s), None, None, None, 0, C.byref(n)) == INV
    assert L.oslam_volume_pack_colour(col_vol, None, None, None, None, 0, C.byref(n)) == INV
    assert L.oslam_volume_pack_colour(col_vol, P(s), None, None, None, 0, None) == INV
    assert L.oslam_volume_pack_colour(col_vol, P(far), None, None, None, 0, C.byref(n)) == INV
    for outs in ((None, P(buf), P(buf)), (P(buf), None, P(buf)), (P(buf), P(buf), None)):
        assert L.oslam_volume_pack_colour(col_vol, P(s), outs[0], outs[1], outs[2], 4, C.byref(n)) == INV
    assert L.oslam_volume_pack_colour(plain_vol, P(s), None, None, None, 0, C.byref(n)) == INV and "no colour" in err()
    assert L.oslam_volume_pack_colour(col_vol, P(zero), None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # the colour of the whole map
    pts = np.zeros((4, 3), np.float32)
    rgb, valid = np.full(12, 7, np.uint8), np.full(4, 7, np.uint8)
    n.value = 9

    def colours(w=cw._h, vol=None, sp=None, xyz=pts, count=4, stride=0, rgb_out=rgb, valid_out=valid):
        return L.oslam_world_colours(w, vol, C.byref(sp) if sp is not None else None, P(xyz) if xyz is not None else None, count,
                                     stride, P(rgb_out) if rgb_out is not None else None,
                                     P(valid_out) if valid_out is not None else None, C.byref(n))

    assert colours(w=None) == colours(xyz=None) == colours(rgb_out=None) == colours(valid_out=None) == INV
    for stride in (4, 8, 13, 18):
        assert colours(count=1, stride=stride) == INV and "stride_bytes" in err(), stride
    assert colours(count=1 << 31) == INV
    assert colours(w=pw._h) == INV and "keeps no colour" in err()
    assert colours(w=pw._h, count=0) == INV                                                 # n == 0 still needs a colour store
    assert colours(vol=plain_vol) == INV and "volume has no colour" in err()
    assert colours(w=other._h, vol=col_vol) == INV
    other.close()
    other = make_world(ppf, voxel=0.02, origin0=(0.0, 0.1, -1.28))                         # the sign of a zero counts
    assert colours(w=other._h, vol=col_vol) == INV and "another voxel size or origin" in err()
    for anchor in ((1 << 20) + 1, 0, 0), (0, -(1 << 20) - 1, 0):
        assert colours(sp=ppf.default_world_surface_params(anchor_set=1, anchor=anchor)) == INV and "anchor" in err()
    assert colours(sp=ppf.default_world_surface_params(min_weight=0)) == INV
    assert n.value == 9 and (rgb == 7).all() and (valid == 7).all()                         # nothing written by any refusal
    # n == 0, and an empty map with points, return zeros without a device call
    assert colours(xyz=None, count=0, rgb_out=None, valid_out=None) == 0 and n.value == 0
    cw.clear()
    n.value = 9
    assert colours() == 0 and n.value == 0 and not rgb.any() and not valid.any()
    got, ok = cw.colours(np.ones((5, 3), np.float32))
    assert got.shape == (5, 3) and ok.shape == (5,) and not got.any() and not ok.any()
    for w in (cw, pw, other):
        w.close()


# ---------------------------------------------------------------- pin (a) on the restatements alone
def blank_coloured(nx, ny, nz, voxel, origin):
    return CR.Volume(nx, ny, nz, voxel, origin, mu=4 * float(voxel))


def probe_points(rng, store_params, lo, hi, anchor, n=4000):
    """points all over the box lo .. hi and a voxel beyond it, in the frame of anchor, plus points on voxel borders and
    centres, where floor decides"""
    A, O, voxel = WS.frame(store_params, None, anchor)
    span = np.array(hi, np.float64) - np.array(lo, np.float64) + 2.0
    r = np.array(lo, np.float64) - 1.0 - np.array(A, np.float64) + rng.random((n, 3)) * span
    r[: n // 4] = np.round(r[: n // 4] * 2.0) / 2.0                 # borders and centres
    P = (O.astype(np.float64) + r * float(voxel)).astype(np.float32)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, -1e30, 0]], np.float32)
    return np.concatenate([P, odd])


def test_pin_a_a_dense_coloured_volume_gives_the_same_bytes():
    rng = np.random.default_rng(31)
    params = (np.float32(0.02), np.asarray((-0.0, 0.1, -1.28), np.float32))
    vol = TH.exact_frame(planted((16, 16, 16), 5), voxel=0.02, origin=(-0.0, 0.1, -1.28))
    vol.inv_voxel = np.float32(1.0) / vol.voxel
    store, cstore = {}, {}
    for s in [(8, -8, 8), (-3, 5, 9)]:                              # the window ends at (5, -3, 17) with a store around it
        vol, _, _ = RC.shift_world(vol, store, cstore, s)
    RC.put(store, cstore, [(6, -2, 18), (40, 3, 3)], [5 << 16, 6 << 16], [0x01ffffff, 0x09102030])    # one inside the window's box: ignored
    assert len(store) > 1000 and H.state(vol)[1] == (5, -3, 17)
    for with_vol in (vol, None):
        lo, hi = WC.coloured_bounds(store, cstore, with_vol)
        for anchor in (lo, None, (-7, 11, 2)):
            P = probe_points(rng, params, lo, hi, lo if anchor is None else anchor)
            got = WC.colour_at(store, cstore, params, P, with_vol, anchor)
            assert not got[-5:].any()                               # NaN, the infinities and 1e30 read nothing
            if anchor == lo:
                d = WC.dense(store, cstore, params, with_vol, lo, hi, blank_coloured)
                want = d.colour_at(P)
                assert got.tobytes() == want.tobytes()
                share = float((got != 0).mean())
                assert 0.1 < share < 0.98, share                     # the probes meet colour and its absence
                # the entry planted inside the window's box shows only without the window
                Pp = (WS.frame(params, None, lo)[1] + (np.array([[6, -2, 18]], np.float32) - np.array(lo, np.float32) + np.float32(0.5)) * params[0])
                one = WC.colour_at(store, cstore, params, Pp, with_vol, lo)
                assert int(one[0]) == int(d.colour_at(Pp)[0]) and (int(one[0]) == 0xffffffff) == (with_vol is None)
            else:
                # another anchor forms other floats; the probes still meet colour
                assert float((got != 0).mean()) > 0.1


# ---------------------------------------------------------------- the colour store alone under the sanitizers
def test_colour_store_alone_under_the_sanitizers():
    """csrc/oslam_world.c and tests/native/world_colour_check.c, nothing else, compiled with -fsanitize=address,undefined
    and run as a program of its own, as test_reload_host runs world_check.c.  A finding makes it exit with a status other
    than 0."""
    out = os.path.join(ROOT, "build", "world_colour_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "objective-slam_amd", "csrc")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-static-libasan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "native", "world_colour_check.c"), os.path.join(csrc, "oslam_world.c"), "-o", out,
                    "-lpthread", "-lm"], check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"world_colour_check ok" in r.stdout, (r.returncode, r.stderr.decode()[-2000:])


# ---------------------------------------------------------------- calibration
def test_the_whole_maps_colour_reaches_the_colour_function(synth):
    for seed in SEEDS:
        r = CAL.run(synth, seed)
        for name in ("colour", "plain"):
            print("seed %d, %s store: %d surface points of the whole map, %.4f with a colour, error median %.2f, 95th percentile "
                  "%.2f levels; %d shifts, %d stored, %d reloaded" % (seed, name, r[name]["points"], r[name]["share"], r[name]["median"],
                                                                     r[name]["p95"], r[name]["shifts"], r[name]["stored"], r[name]["reloaded"]))
        c, p = r["colour"], r["plain"]
        assert c["shifts"] >= 1 and c["stored"] > 0 and c["points"] == p["points"] > 1000
        assert c["share"] >= SHARE_MIN, (seed, c["share"])
        assert p["share"] < c["share"], (seed, p["share"], c["share"])
        assert c["median"] <= MEDIAN_BOUND and c["p95"] <= P95_BOUND, (seed, c["median"], c["p95"])
