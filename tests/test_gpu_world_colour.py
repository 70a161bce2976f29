"""GPU: colour through the voxel store (oslam_volume_shift_world with a colour store, oslam_volume_pack_colour) and the
colour of the whole map (oslam_world_colours, World.surface(colour=True), World.mesh_colour) against the numpy
restatements of tests/reload_colour_ref.py and tests/world_colour_ref.py, byte for byte: the words are 32-bit integers, the
colours bytes, and nothing here has a tolerance.

The volumes are 16^3 and 40 x 72 x 24 (test_gpu_shift's: 4 and 67.5 workgroups of the pack, rows of 40 so that a chunk
straddles rows and slabs).  TSDF words and colour words are random over all 32 bits, a fifth of the colour words with
wc == 0, with the planted seen-but-uncoloured and coloured-but-unseen voxels of tests/test_world_colour_host.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import colour_ref as CR  # noqa: E402
import edge_inputs  # noqa: E402
import reload_colour_ref as RC  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_calib as SC  # noqa: E402
import shift_ref as H  # noqa: E402
import test_colour_host as TCH  # noqa: E402
import test_gpu_colour as TGC  # noqa: E402
import test_gpu_reload as TGR  # noqa: E402
import test_gpu_shift as TG  # noqa: E402
import test_gpu_surface as TS  # noqa: E402
import test_gpu_world_surface as TGW  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import test_world_colour_host as TC  # noqa: E402
import test_world_surface_host as TW  # noqa: E402
import volume_ref as V  # noqa: E402
import world_colour_ref as WC  # noqa: E402
import world_surface_ref as WS  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint32
RAGGED = TG.RAGGED
SHAPES, IDS = TGR.SHAPES, TGR.IDS
CHAIN = TR.CHAIN


def frame(vol):
    return TH.exact_frame(vol, **TG.WORDS_FRAME)


def on_device(ppf, ref):
    """a coloured device volume with the restated volume's parameters, words and colour words"""
    dev = TS.on_device(ppf, ref)
    dev.enable_colour()
    dev.set_colour_words(ref.c)
    return dev


def reload(dev, ref):
    TG.reload(dev, ref)                                             # reset zeroes the colours too
    dev.set_colour_words(ref.c)


def same_colours(dev, ref):
    return dev.colour_words().tobytes() == np.asarray(ref.c, U).tobytes()


def same_store(world, store, cstore, lo, hi):
    got, gotc = world.box(lo, hi, colours=True)
    want, wantc = RC.box(store, cstore, lo, hi)
    return got.tobytes() == want.tobytes() and gotc.tobytes() == wantc.tobytes() and world.stats()["voxels"] == len(store)


def launches_of(s, stored, reloaded):
    """a coloured volume through a colour store (include/oslam.h): count and scan; emit and the colours' gather when
    something seen leaves; the two shifts; unpack and the colours' scatter when something comes back"""
    return 0 if not any(s) else 4 + 2 * (stored > 0) + 2 * (reloaded > 0)


def launches_plain(s, stored, reloaded):
    """the same volume through a plain store: what it was before colour stores"""
    return 0 if not any(s) else 4 + (stored > 0) + (reloaded > 0)


# ---------------------------------------------------------------- 1. the pack tap
@pytest.mark.parametrize("n", SHAPES, ids=IDS)
def test_pack_tap_with_colours_equals_the_restatement(built_lib, ppf, n):
    ref = frame(TC.planted(n, 11))
    nx, ny, nz = n
    dev = on_device(ppf, ref)
    for s in TGR.ten_shifts(n) + [(0, 0, 0)]:
        lin, words, cols = dev.packed(s, colours=True)
        wl, ww, wc = RC.packed(ref, s)
        print("%s, shift %s: %d records (restatement %d)" % (n, s, len(lin), len(wl)))
        assert len(lin) == len(wl) and lin.tobytes() == wl.tobytes() and words.tobytes() == ww.tobytes(), s
        assert cols.tobytes() == wc.tobytes(), (s, np.flatnonzero(cols != wc)[:8])
        assert (len(lin) == 0) == (not any(s))
        pl, pw = dev.packed(s)                                      # the plain tap is what it was
        assert pl.tobytes() == lin.tobytes() and pw.tobytes() == words.tobytes()
    assert TG.same_words(dev, ref) and same_colours(dev, ref) and dev.window()[0] == (0, 0, 0)     # the tap changes nothing
    # everything seen and everything leaves: one record per voxel, the ragged last workgroup included
    full = TC.coloured(frame(TH.full_range(n, 13)), 14)
    full.w[:] |= 1
    dev.set_voxels(full.q, full.w)
    dev.set_colour_words(full.c)
    lin, words, cols = dev.packed((nx, 0, 0), colours=True)
    assert len(lin) == nx * ny * nz and (n != RAGGED or len(lin) == 69120)
    assert lin.tobytes() == np.arange(nx * ny * nz, dtype=U).tobytes() and words.tobytes() == W.words_of(full).tobytes()
    assert cols.tobytes() == full.c.tobytes()
    # a volume without colour has no such tap
    plain = TS.on_device(ppf, ref)
    with pytest.raises(ppf.OslamError) as e:
        plain.packed((1, 0, 0), colours=True)
    assert e.value.code == ppf.OSLAM_E_INVALID
    plain.close()
    dev.close()


# ---------------------------------------------------------------- 2. out and back
@pytest.mark.parametrize("n", SHAPES, ids=IDS)
def test_out_and_back_restores_the_colours_of_seen_voxels(built_lib, ppf, n):
    ref = frame(TC.planted(n, 11))
    nx = n[0]
    dev, twin = on_device(ppf, ref), on_device(ppf, ref)            # twin: the same run through a plain store
    world, plain = ppf.World(dev, colour=True), ppf.World(twin)
    assert world.has_colour() and not plain.has_colour()
    seen = W.seen(W.words_of(ref))
    for path in ([(8, -8, 8), (-8, 8, -8)], CHAIN, [(nx + 5, -3, 0), (-nx - 5, 3, 0)]):
        reload(dev, ref)
        reload(twin, ref)
        cur, store, cstore = ref, {}, {}
        for s in path:
            res, tres = dev.shift(s, world), twin.shift(s, plain)
            cur, stored, reloaded = RC.shift_world(cur, store, cstore, s)
            bad = np.flatnonzero((dev.colour_words() != cur.c).ravel())
            print("%s, path %s, shift %s: stored %d, reloaded %d, %d launches (plain store %d), %d colour words differ" % (
                n, path, s, res["stored"], res["reloaded"], res["launches"], tres["launches"], bad.size))
            assert bad.size == 0, (path, s, bad[:8])
            assert TG.same_words(dev, cur) and TG.same_window(dev, cur), (path, s)
            assert (res["stored"], res["reloaded"], res["kept"]) == (stored, reloaded, H.kept(cur)), (path, s, res)
            # the TSDF side equals the run through a plain store
            assert TG.same_words(twin, cur) and {k: res[k] for k in ("kept", "stored", "reloaded", "offset")} == \
                {k: tres[k] for k in ("kept", "stored", "reloaded", "offset")}, (path, s, res, tres)
            assert res["launches"] == launches_of(s, stored, reloaded), (path, s, res)
            assert tres["launches"] == launches_plain(s, stored, reloaded), (path, s, tres)
            assert world.stats()["voxels"] == len(store) == plain.stats()["voxels"]
        want = RC.restored(ref, path)
        got = dev.colour_words()
        assert (got[seen] == ref.c[seen]).all() and got.tobytes() == want.tobytes(), path
        assert TGR.dev_words(dev).tobytes() == TR.restored(ref, path).tobytes()
        st = world.stats()
        assert reloaded > 0 and (st["voxels"], st["bricks"], st["lo"], st["hi"]) == (0, 0, (0, 0, 0), (0, 0, 0)) and store == cstore == {}
        # the plain store gave the words back and no colour: the difference is the feature
        lost = seen & (twin.colour_words() != ref.c)
        assert lost.any() and not twin.colour_words()[lost].any()
    for x in (world, plain, dev, twin):
        x.close()


# ---------------------------------------------------------------- 3. a seeded store
def test_a_seeded_colour_store_gives_back_exactly_the_entering_region(built_lib, ppf):
    ref = frame(TC.planted(RAGGED, 11))
    dev = on_device(ppf, ref)
    world = ppf.World(dev, colour=True)
    s = (3, -5, 2)                                                  # the new window is [3, 43) x [-5, 67) x [2, 26) in g
    inside = [(41, 10, 5), (42, 66, 25), (10, -5, 2), (3, -1, 25), (40, 0, 2), (20, 30, 24), (42, -5, 25)]
    outside = [(43, 10, 5), (2, -3, 5), (10, -6, 5), (10, 10, 26), (-1, -1, -1), (41, 67, 5), (10, -5, 1), (-40, -72, -24)]
    overlap = [(10, 10, 10)]                                        # inside both windows: it does not enter and stays stored
    leaving = [(1, 1, 1)]                                           # a voxel that leaves: its word and colour overwrite the seed
    g = inside + outside + overlap + leaving
    words = [(1000 + i) << 16 | i for i in range(len(g))]
    cols = [(i % 3) << 24 | 0x00100000 | i for i in range(len(g))]  # every third with wc == 0: stored and returned as it is
    world.put(g, words, cols)
    store, cstore = {}, {}
    RC.put(store, cstore, g, words, cols)
    res = dev.shift(s, world)
    want, stored, reloaded = RC.shift_world(ref, store, cstore, s)
    assert reloaded == len(inside) and (res["stored"], res["reloaded"]) == (stored, reloaded)
    assert res["kept"] == H.kept(want) and res["launches"] == 8
    got, gotc = TGR.dev_words(dev), dev.colour_words()
    assert got.tobytes() == W.words_of(want).tobytes() and gotc.tobytes() == want.c.tobytes() and TG.same_window(dev, want)
    for gg, word, col in zip(inside, words, cols):
        i, j, k = (gg[a] - s[a] for a in range(3))
        assert (int(got[k, j, i]), int(gotc[k, j, i])) == (word, col) and gg not in store, gg
        assert not any(x.any() for x in world.box(gg, [c + 1 for c in gg], colours=True)), gg
    for gg in outside + overlap:
        a, b = world.box(gg, [c + 1 for c in gg], colours=True)
        assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (store[gg], cstore[gg]) == (words[g.index(gg)], cols[g.index(gg)]), gg
    a, b = world.box((1, 1, 1), (2, 2, 2), colours=True)
    assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (int(W.words_of(ref)[1, 1, 1]), int(ref.c[1, 1, 1])) != (words[-1], cols[-1])
    assert same_store(world, store, cstore, (-48, -80, -32), (56, 88, 40))
    world.close()
    dev.close()


# ---------------------------------------------------------------- 4. with fusion in between
@pytest.fixture(scope="module")
def ragged_stream(synth):
    """two frames of seed 0 at the ragged 333 x 251 with a colour image each (tests/test_gpu_colour.py's)"""
    pts = E.make_world(synth, 0)
    traj = [T.astype(np.float32) for T in E.trajectory(synth, 0)[:2]]
    cam = edge_inputs.ragged_cam()
    imgs = [E.render(synth, pts, T, **edge_inputs.RAGGED) for T in traj]
    cols = [TGC.colour_image(synth, 251, 333, 910 + f) for f in range(2)]
    return dict(traj=traj, cam=cam, imgs=imgs, cols=cols)


def test_fusion_with_colour_between_the_shifts(built_lib, ppf, ragged_stream):
    st = ragged_stream
    spec, colour = TGC.RAGGED_VOL, TGC.COLOUR["ragged"]
    ref = TGC.ref_volume(spec, colour)
    dev = TGC.dev_volume(ppf, spec, colour)
    world = ppf.World(dev, colour=True)
    store, cstore = {}, {}

    def fuse(f):
        nonlocal ref
        v = TS.view_of(ppf, st["imgs"][f], st["cam"])
        v.set_colour(*st["cols"][f])
        got = dev.integrate(v, st["traj"][f], colour=v)
        v.close()
        want = ref.integrate_colour(V.z_image(st["imgs"][f], st["cam"]), CR.pack(*st["cols"][f]), st["cam"], st["traj"][f])
        assert (got["updated"], got["coloured"]) == want and want[1] > 0
        assert TG.same_words(dev, ref) and same_colours(dev, ref)

    fuse(0)
    res = dev.shift((8, -8, 0), world)
    ref, stored, reloaded = RC.shift_world(ref, store, cstore, (8, -8, 0))
    assert (res["stored"], res["reloaded"]) == (stored, 0) and stored > 0 and TG.same_words(dev, ref) and same_colours(dev, ref)
    assert sum(1 for c in cstore.values() if c >> 24) > 100          # colour did go into the store
    fuse(1)
    res = dev.shift((-8, 8, 0), world)
    ref, stored2, reloaded2 = RC.shift_world(ref, store, cstore, (-8, 8, 0))
    print("40x72x24 fused with colour: %d stored, then %d stored and %d reloaded, store %s" % (stored, stored2, reloaded2, world.stats()))
    assert (res["stored"], res["reloaded"], res["kept"]) == (stored2, reloaded2, H.kept(ref)) and reloaded2 == stored
    assert TG.same_words(dev, ref) and same_colours(dev, ref) and TG.same_window(dev, ref) and dev.window()[0] == (0, 0, 0)
    assert same_store(world, store, cstore, (-16, -16, -8), (56, 88, 32)) and len(store) == stored2 > 0
    world.close()
    dev.close()


# ---------------------------------------------------------------- 5. failure changes nothing
def test_a_refused_shift_changes_nothing(built_lib, ppf):
    ref = frame(TC.planted(RAGGED, 11))
    dev, bare = on_device(ppf, ref), TS.on_device(ppf, ref)
    s = (3, -5, 2)
    fits = ppf.World(dev, colour=True)
    other = TC.make_world(ppf, voxel=0.021, origin0=[float(x) for x in ref.origin])
    small = ppf.World(dev, max_bytes=64 * 8 + 2 * TC.COLOUR_BRICK, colour=True)      # the table and two colour bricks
    for w in (fits, other, small):
        w.put([(100, 100, 100)], [7 << 16], [0x05010203])
    INV, LIM = ppf.OSLAM_E_INVALID, ppf.OSLAM_E_LIMIT
    for vol, w, code in ((bare, fits, INV), (dev, other, INV), (dev, small, LIM)):
        before = w.stats()
        with pytest.raises(ppf.OslamError) as e:
            vol.shift(s, w)
        assert e.value.code == code, str(e.value)
        off, org = vol.window()
        assert TG.same_words(vol, ref) and off == (0, 0, 0) and org.tobytes() == ref.origin.tobytes()
        assert vol is bare or same_colours(vol, ref)
        assert w.stats() == before == dict(before, voxels=1, bricks=1)
        a, b = w.box((100, 100, 100), (101, 101, 101), colours=True)
        assert (int(a[0, 0, 0]), int(b[0, 0, 0])) == (7 << 16, 0x05010203)
    res = dev.shift(s, fits)                                        # and the shift through a store that fits still works
    want, stored, reloaded = RC.shift_world(ref, {}, {}, s)
    assert TG.same_words(dev, want) and same_colours(dev, want) and (res["stored"], res["reloaded"]) == (stored, 0)
    for x in (fits, other, small, dev, bare):
        x.close()


# ---------------------------------------------------------------- 6. the colour of the whole map
def coloured_dense_device(ppf, box):
    """test_gpu_world_surface.dense_device with the restated dense volume's colour words"""
    dev = TGW.dense_device(ppf, box)
    n = (dev.params.nz, dev.params.ny, dev.params.nx)
    c = np.zeros(n, U)
    c[:box.n[2], :box.n[1], :box.n[0]] = box.c
    dev.enable_colour()
    dev.set_colour_words(c)
    return dev


def constructed_points(sp, vol, store, cstore, anchor):
    """-> (P float32 [n, 3], what: a dict of index arrays).  Points at g + (0.8, 0.8, 0.8) voxels have the base corner g
    exactly where the floats are exact enough, which the caller does not rely on: the restatement decides.
      straddle   bases with local coordinate 7 on each of the seven non-empty sets of axes, inside the window and in the store
      faces      bases at off - 2, off - 1, off, off + n - 2, off + n - 1, off + n on every axis: both sides of every face
      negative   bases with negative g
      planted    the centre of the store entry planted inside the window's box
      odd        NaN, the infinities and 1e30"""
    A, O, voxel = WS.frame(sp, vol, anchor)
    off, n = np.array(H.state(vol)[1]), np.array(vol.n)
    bases, what = [], {}

    def add(name, gs):
        what[name] = np.arange(len(bases), len(bases) + len(gs))
        bases.extend(gs)

    strad = []
    for mask in range(1, 8):
        for centre in (off + n // 2, off - 12, off + n + 5):         # the window, and the store on either side
            g = (np.array(centre) >> 3 << 3) + 3
            for a in range(3):
                if mask >> a & 1:
                    g[a] = (g[a] >> 3 << 3) + 7
            strad.append(tuple(int(x) for x in g))
    add("straddle", strad)
    faces = []
    for a in range(3):
        for at in (off[a] - 2, off[a] - 1, off[a], off[a] + n[a] - 2, off[a] + n[a] - 1, off[a] + n[a]):
            for other in (off + n // 2, off + 1):
                g = np.array(other)
                g[a] = at
                faces.append(tuple(int(x) for x in g))
    add("faces", faces)
    add("negative", [(-3, -2, 5), (-9, -1, 4), (-1, -1, 3)])
    g = np.array(bases, np.float64) - np.array(A, np.float64)
    P = [(O.astype(np.float64) + (g + 0.5 + 0.3) * float(voxel)).astype(np.float32)]
    what["planted"] = np.array([len(bases)])
    P.append((O.astype(np.float64) + (np.array([PLANTED], np.float64) - np.array(A, np.float64) + 0.5) * float(voxel)).astype(np.float32))
    what["odd"] = np.arange(len(bases) + 1, len(bases) + 6)
    P.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, -1e30, 1e30]], np.float32))
    return np.concatenate(P), what


PLANTED = (0, 0, 10)            # inside the window's box after the first two shifts of the chain (offset (-4, -4, 3))


@pytest.fixture(scope="module")
def coloured_map():
    """the restated map after the first two shifts of the chain: a store on every side of the window, a seeded entry far
    out and one planted inside the window's box"""
    vol = TW.usual(RAGGED, 31)
    vol.c = TC.colour_words(RAGGED, 131)
    sp = TW.params_of(vol)
    store, cstore, cur = {}, {}, vol
    for s in CHAIN[:2]:
        cur, _, _ = RC.shift_world(cur, store, cstore, s)
    assert H.state(cur)[1] == (-4, -4, 3)
    RC.put(store, cstore, [PLANTED, (60, 3, 3)], [5 << 16, 6 << 16], [0x01fffefd, 0x09102030])
    lo, hi = WC.coloured_bounds(store, cstore, cur)
    lo = tuple(x - d for x, d in zip(lo, (5, 3, 2)))                # the dense volume's offset, and with it the anchor, is not 0
    return dict(start=vol, sp=sp, store=store, cstore=cstore, vol=cur, lo=lo, hi=hi)


def device_map(ppf, m):
    """-> (the coloured device volume at the map's window, the library's colour store with the map's entries)"""
    dev = on_device(ppf, m["start"])
    dev.shift(H.state(m["vol"])[1])
    dev.set_voxels(m["vol"].q, m["vol"].w)
    dev.set_colour_words(m["vol"].c)
    w = TC.make_world(ppf, voxel=float(m["sp"][0]), origin0=[float(x) for x in m["sp"][1]])
    g = list(m["store"].keys())
    w.put(np.array(g, np.int32), np.array([m["store"][k] for k in g], U), np.array([m["cstore"][k] for k in g], U))
    return dev, w


def check_colours(name, got, want, P):
    rgb, valid = got
    wrgb, wvalid = want
    bad = np.flatnonzero((rgb != wrgb).any(axis=1) | (valid != wvalid))
    print("%s: %d points, %d with a colour (restatement %d), %d differ" % (name, len(P), int(valid.sum()), int(wvalid.sum()), bad.size))
    assert bad.size == 0, (name, bad[:8], P[bad[:8]], rgb[bad[:8]], wrgb[bad[:8]])
    assert rgb.tobytes() == wrgb.tobytes() and not rgb[~valid].any()


def test_world_colours_equal_the_restatement_and_both_pins(built_lib, ppf, coloured_map):
    m = coloured_map
    store, cstore, sp, vol, lo, hi = m["store"], m["cstore"], m["sp"], m["vol"], m["lo"], m["hi"]
    dev, world = device_map(ppf, m)
    # pin (a): a dense coloured volume at offset lo that holds G and Gc over the box of everything coloured
    box = WC.dense(store, cstore, sp, vol, lo, hi, TC.blank_coloured)
    dense = coloured_dense_device(ppf, box)
    po, _ = world.surface(dev, anchor=lo)
    vx, _, _, _ = world.mesh(dev, anchor=lo, normals=False)
    extra, what = constructed_points(sp, vol, store, cstore, lo)
    P = np.concatenate([po, vx, extra])
    base = len(po) + len(vx)
    assert len(po) > 1000 and len(vx) >= len(po)
    want = WC.colours(store, cstore, sp, P, vol, lo)
    got = world.colours(P, dev, anchor=lo)
    check_colours("the map at anchor %s" % (lo,), got, want, P)
    check_colours("pin (a), Volume.colours of the dense volume", dense.colours(P), got, P)
    again = world.colours(P, dev, anchor=lo)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()      # two calls, the same bytes
    # what the constructed points are, from the map itself and not from the code under test
    valid = want[1]
    gc = WC.colour_map(store, cstore, vol)
    A = np.array(lo)
    O = WS.frame(sp, vol, lo)[1]
    u = (extra - O) * (np.float32(1.0) / np.float32(sp[0]))
    with np.errstate(all="ignore"):
        b = np.floor(u - np.float32(0.5))
    fin = np.isfinite(b).all(axis=1) & (np.abs(b) < 2 ** 22).all(axis=1)
    bg = np.where(fin[:, None], b, 0).astype(np.int64) + A
    near = np.where(fin[:, None], np.floor(np.where(fin[:, None], u, 0)), 0).astype(np.int64) + A
    corners = np.stack([gc.at(bg + np.array(d)) >> U(24) != 0 for d in np.ndindex(2, 2, 2)], axis=1)
    all8, near_ok = corners.all(axis=1) & fin, (gc.at(near) >> U(24) != 0) & fin
    local = bg & 7
    for mask in range(1, 8):                                        # the seven straddling patterns are all there
        pat = np.array([(mask >> a & 1) == 1 for a in range(3)])
        assert ((local[what["straddle"]] == 7) == pat).all(axis=1).any(), mask
    assert all8[what["straddle"]].any() and (~all8 & near_ok).any() and (~all8 & ~near_ok & fin).any()      # blend, nearest voxel, none
    assert (corners.any(axis=1) & ~all8 & near_ok).any()            # an uncoloured corner with a coloured nearest voxel
    off, n = np.array(H.state(vol)[1]), np.array(vol.n)
    inside = ((bg >= off) & (bg < off + n)).all(axis=1)
    assert inside[what["faces"]].any() and (~inside[what["faces"]]).any() and (bg[what["negative"]] < 0).any(axis=1).all()
    assert not valid[base + what["odd"]].any()
    # the entry planted inside the window's box is ignored: the point has the window's colour, or none, never the entry's
    pl = base + what["planted"][0]
    i, j, k = (PLANTED[a] - off[a] for a in range(3))
    assert tuple(got[0][pl]) != (0xfd, 0xfe, 0xff) and bool(valid[pl]) == bool(vol.c[k, j, i] >> U(24))
    # pin (b): the default anchor; a point whose corners and nearest voxel lie inside the window reads as Volume.colours
    Pb = np.concatenate([po, extra])
    gb = world.colours(Pb, dev)
    check_colours("the map at the default anchor", gb, WC.colours(store, cstore, sp, Pb, vol), Pb)
    Ob = WS.frame(sp, vol, None)[1]
    ub = (Pb - Ob) * (np.float32(1.0) / np.float32(sp[0]))
    with np.errstate(all="ignore"):
        bb, nb = np.floor(ub - np.float32(0.5)), np.floor(ub)
    within = ((bb >= 0) & (bb <= n - 2) & (nb >= 0) & (nb < n)).all(axis=1)
    vb = dev.colours(Pb)
    assert within.sum() > 500 and (~within).sum() > 100
    assert gb[0][within].tobytes() == vb[0][within].tobytes() and np.array_equal(gb[1][within], vb[1][within])
    assert (gb[1][~within] & ~vb[1][~within]).any()                 # beyond the window only the map has colour
    # the store alone, and a set anchor of its own
    for anchor in (None, (-7, 11, 2)):
        Ps = np.concatenate([world.surface(anchor=anchor)[0], extra])
        gs = world.colours(Ps, anchor=anchor)
        check_colours("the store alone, anchor %s" % (anchor,), gs, WC.colours(store, cstore, sp, Ps, None, anchor), Ps)
        assert gs[1].any()
    # there the planted entry shows
    one = world.colours(extra[what["planted"]], anchor=lo)
    assert tuple(one[0][0]) == (0xfd, 0xfe, 0xff) and one[1][0]
    # n == 0
    rgb0, valid0 = world.colours(np.zeros((0, 3), np.float32), dev)
    assert rgb0.shape == (0, 3) and valid0.shape == (0,)
    # a plain store, and a volume without colour, are refused
    bare, plain = TS.on_device(ppf, m["start"]), ppf.World(dev)
    for w, v in ((plain, dev), (world, bare)):
        with pytest.raises(ppf.OslamError) as e:
            w.colours(P[:4], v)
        assert e.value.code == ppf.OSLAM_E_INVALID
    for x in (bare, plain, dense, world, dev):
        x.close()


# ---------------------------------------------------------------- 7. the Python outputs
def test_surface_and_mesh_with_colour_and_the_ply(built_lib, ppf, coloured_map, tmp_path):
    m = coloured_map
    dev, world = device_map(ppf, m)
    po, no, rgb, valid = world.surface(dev, colour=True)
    po0, no0 = world.surface(dev)
    assert po.tobytes() == po0.tobytes() and no.tobytes() == no0.tobytes() and len(po) == world.last_surface["points"] > 1000
    assert rgb.shape == (len(po), 3) and rgb.dtype == np.uint8 and valid.shape == (len(po),) and valid.dtype == bool
    want = world.colours(po, dev)
    assert rgb.tobytes() == want[0].tobytes() and np.array_equal(valid, want[1]) and 0 < valid.sum() < len(valid)
    check_colours("World.surface(colour=True)", (rgb, valid), WC.colours(m["store"], m["cstore"], m["sp"], po, m["vol"]), po)
    out = world.surface(dev, keys=True, anchor=m["lo"], colour=True)
    assert len(out) == 5 and out[2].shape == (len(out[0]), 4) and out[3].tobytes() == world.colours(out[0], dev, anchor=m["lo"])[0].tobytes()
    xyz, nrm, tri, res, mrgb, mvalid = world.mesh_colour(dev)       # mesh() itself keeps its pinned parameter list
    xyz0, nrm0, tri0, res0 = world.mesh(dev)
    assert xyz.tobytes() == xyz0.tobytes() and tri.tobytes() == tri0.tobytes() and len(xyz) == res["vertices"] > 0
    wm = world.colours(xyz, dev)
    assert mrgb.shape == (len(xyz), 3) and mrgb.tobytes() == wm[0].tobytes() and np.array_equal(mvalid, wm[1]) and mvalid.any()
    assert len(world.mesh_colour(dev, keys=True)) == 7 and len(world.mesh_colour()) == 6
    # the coloured PLYs, read back
    f = str(tmp_path / "map_cloud.ply")
    ppf.ply_write(f, po, no, rgb=rgb)
    lines, v, rest = TCH.parse_ply(f)
    assert "property uchar red" in lines and len(rest) == 0
    assert np.stack([v["x"], v["y"], v["z"]], axis=1).tobytes() == po.tobytes() and np.stack([v["r"], v["g"], v["b"]], axis=1).tobytes() == rgb.tobytes()
    f = str(tmp_path / "map_mesh.ply")
    ppf.ply_write_mesh(f, xyz, nrm, tri, rgb=mrgb)
    p2, n2, t2 = ppf.ply_read_mesh(f)
    assert p2.tobytes() == xyz.tobytes() and n2.tobytes() == nrm.tobytes() and t2.tobytes() == tri.tobytes()
    lines, v, _ = TCH.parse_ply(f)
    assert "property uchar red" in lines and np.stack([v["r"], v["g"], v["b"]], axis=1).tobytes() == mrgb.tobytes()
    world.close()
    dev.close()


def test_step_with_follow_a_colour_store_and_colour(built_lib, ppf, synth):
    """Volume.step(view, follow=, world=w, colour=view) on the stream of tests/shift_calib.py: every shift moves the
    words and the colour words as the restatement moves the device's own state before it, the store holds what the
    restated store holds, colours included, and the whole map's surface has colour where the window no longer looks."""
    pts, traj = E.make_world(synth, 0), E.trajectory(synth, 0)
    cam = V.SMALL_CAM
    ep = ppf.default_egomotion_params(min_overlap=SC.MIN_OVERLAP)
    views = []
    for f, T in enumerate(traj[:5]):
        v = TS.view_of(ppf, E.render(synth, pts, T, **V.SMALL), cam)
        v.set_colour(*TGC.colour_image(synth, V.SMALL["height"], V.SMALL["width"], 920 + f))
        views.append(v)
    dev = ppf.Volume(**SC.VOLUME)
    dev.enable_colour()
    fp = ppf.default_follow_params(dev, **SC.FOLLOW)
    world = ppf.World(dev, colour=True)
    store, cstore, log = {}, {}, []
    shift = dev.shift

    def spy_shift(s, w=None):
        ref = TS.restated(dev, SC.VOLUME)                           # the words, colours and window before the shift
        ref.c = dev.colour_words()
        ref.origin0 = ref.origin.copy()
        ref.off, ref.origin = dev.window()
        res = shift(s, w)
        log.append((tuple(int(x) for x in s), w, ref, res))
        return res

    dev.shift = spy_shift
    dev.leaving = None                                              # with a store nothing is extracted: a call would fail
    for f, v in enumerate(views):
        n_log = len(log)
        T, r = dev.step(v, ep, follow=fp, world=world, colour=v)
        assert dev.last_integrate["coloured"] > 0
        for s, w, before, res in log[n_log:]:
            assert w is world
            want, stored, reloaded = RC.shift_world(before, store, cstore, s)
            assert TG.same_words(dev, want) and same_colours(dev, want) and TG.same_window(dev, want)
            assert (res["stored"], res["reloaded"], res["kept"]) == (stored, reloaded, H.kept(want))
            assert res["launches"] == launches_of(s, stored, reloaded)
        print("frame %d: ok %s, window %s, store %s" % (f, None if r is None else r["ok"], dev.window()[0], world.stats()))
        assert world.stats()["voxels"] == len(store) and dev.world == []
    assert len(log) >= 1 and len(store) > 0 and sum(1 for c in cstore.values() if c >> 24) > 100
    st = world.stats()
    assert same_store(world, store, cstore, st["lo"], st["hi"])
    po, no, rgb, valid = world.surface(dev, colour=True)
    inside = dev.colours(po)[1]
    print("the whole map: %d points, %d with a colour, %d of them beyond the window's reach" % (len(po), int(valid.sum()), int((valid & ~inside).sum())))
    assert (valid & ~inside).sum() > 100 and valid.mean() > 0.9
    for v in views:
        v.close()
    world.close()
    dev.close()
