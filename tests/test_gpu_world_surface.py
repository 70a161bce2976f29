"""GPU: the surface of the whole map, voxel store plus window (oslam_world_surface, oslam_scene_from_world, World.surface,
Scene.from_world), against the numpy restatement of tests/world_surface_ref.py, bit for bit: points, normals, their
order, their keys and the two counts.  Nothing here has a tolerance.

A workgroup owns one 8 x 8 x 8 brick.  The window of 40 x 72 x 24 at the offsets of the shift chain is not aligned to
the bricks on any axis, so bricks are shared between window and store and merged voxel by voxel; the words are random
over all 32 bits (test_world_surface_host.usual), so nearly every edge is a crossing and a word from a wrong index
shows.  The restated chain is computed once and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_calib as SC  # noqa: E402
import shift_ref as H  # noqa: E402
import surface_ref as S  # noqa: E402
import test_gpu_surface as TS  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import test_world_surface_host as TW  # noqa: E402
import volume_ref as V  # noqa: E402
import world_surface_ref as WS  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED, CHAIN, FRAME = TW.RAGGED, TW.CHAIN, TW.FRAME
G_FAR = (1 << 20) + 500


def same(name, got, want, res=None):
    """device (points, normals, keys) against the restatement's (points, normals, keys, crossings), as bits"""
    po, no, ko = got
    wx, wn, wk, wc = want
    if res is not None:
        print("%s: %d crossings, %d points (restatement %d, %d), %d bricks of which %d under the window, %d launches" % (
            name, res["crossings"], res["points"], wc, len(wx), res["bricks"], res["window_bricks"], res["launches"]))
        assert (res["crossings"], res["points"]) == (wc, len(wx)), name
    assert len(po) == len(wx) and ko.tobytes() == wk.tobytes(), name
    bad = np.flatnonzero((po.view(np.uint32) != wx.view(np.uint32)).any(axis=1) | (no.view(np.uint32) != wn.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (name, bad[:8], ko[bad[:4]], po[bad[:4]], wx[bad[:4]], no[bad[:4]], wn[bad[:4]])


def store_of(ppf, store, sp):
    """a library store with the restated store's entries"""
    w = TR.make_world(ppf, voxel=float(sp[0]), origin0=[float(x) for x in sp[1]])
    if store:
        w.put(np.array(list(store.keys()), np.int32), np.array(list(store.values()), np.uint32))
    return w


def dense_device(ppf, box):
    """a device volume with the restated dense volume's words, plain-shifted empty to its offset; its sides padded up to
    multiples of 8 (the padding is unseen and lies beyond the margin)"""
    n = [max(16, -(-x // 8) * 8) for x in box.n]
    assert max(n) <= 512
    origin0, off = H.state(box)
    dev = ppf.Volume(n[0], n[1], n[2], float(box.voxel), [float(x) for x in origin0])
    dev.shift(off)
    q, w = np.zeros((n[2], n[1], n[0]), np.int16), np.zeros((n[2], n[1], n[0]), np.uint16)
    q[:box.n[2], :box.n[1], :box.n[0]], w[:box.n[2], :box.n[1], :box.n[0]] = box.q, box.w
    dev.set_voxels(q, w)
    assert dev.window()[0] == tuple(off) and dev.window()[1].tobytes() == box.origin.tobytes()
    return dev


# ---------------------------------------------------------------- the shift chain
@pytest.fixture(scope="module")
def chain():
    """the restated chain: the window before it, and after every shift the store, the window and the restatement's
    surface for min_weight 1 and 3 with the default anchor"""
    vol = TW.usual(RAGGED, 31)
    sp = TW.params_of(vol)
    store, cur, steps = {}, vol, []
    for s in CHAIN:
        cur, _, _ = W.shift_world(cur, store, s)
        steps.append(dict(shift=s, store=dict(store), vol=cur, want={mw: WS.world_surface(store, sp, cur, mw) for mw in (1, 3)}))
    return dict(start=vol, sp=sp, steps=steps)


@pytest.mark.parametrize("mw", [1, 3])
def test_shift_chain(built_lib, ppf, chain, mw):
    dev = TS.on_device(ppf, chain["start"])
    world = ppf.World(dev)
    before = world.surface(dev, mw, keys=True)
    assert world.last_surface["bricks"] == world.last_surface["window_bricks"] == 5 * 9 * 3
    for step in chain["steps"]:
        dev.shift(step["shift"], world)
        got = world.surface(dev, mw, keys=True)
        res = world.last_surface
        same("40x72x24 after %s, min_weight %d" % (step["shift"], mw), got, step["want"][mw], res)
        assert res["anchor"] == dev.window()[0] and res["launches"] == 4 and res["bricks"] >= max(res["window_bricks"], world.stats()["bricks"])
    assert dev.window()[0] == (0, 0, 0) and world.stats()["bricks"] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, before))        # out and back: the map it was
    # against Volume.surface() of a dense volume that holds the same words, at a step with a store on every side of the
    # window and after the last shift
    for step in (chain["steps"][1], chain["steps"][-1]):
        lo, hi = WS.bounds(step["store"], step["vol"], margin=3)
        box = WS.dense(step["store"], chain["sp"], step["vol"], lo, hi, S.blank)
        dense = dense_device(ppf, box)
        dx, dn, dres = dense.surface(mw)
        cur, w2 = TS.on_device(ppf, chain["start"]), store_of(ppf, step["store"], chain["sp"])
        cur.shift(H.state(step["vol"])[1])
        cur.set_voxels(step["vol"].q, step["vol"].w)
        po, no, ko = w2.surface(cur, mw, anchor=lo, keys=True)
        order = WS.dense_order(ko)
        print("dense %s at %s: %d crossings, %d points; the map %d, %d" % (dense.params.nx, lo, dres["crossings"], dres["points"],
                                                                        w2.last_surface["crossings"], len(po)))
        assert w2.last_surface["crossings"] == dres["crossings"] > 0 and len(po) == len(dx) > 0 and w2.last_surface["anchor"] == tuple(lo)
        assert po[order].tobytes() == dx.tobytes() and no[order].tobytes() == dn.tobytes()
        for x in (dense, cur, w2):
            x.close()
    world.close()
    dev.close()


# ---------------------------------------------------------------- an empty store
def test_empty_store_equals_the_windows_surface(built_lib, ppf):
    ref = TW.usual(RAGGED, 32)
    rim = np.ones(ref.w.shape, bool)
    rim[3:-3, 3:-3, 3:-3] = False
    ref.w[rim] = 0
    for off in ((0, 0, 0), (3, -5, 2), (-16, 8, 64)):
        dev = TS.on_device(ppf, ref)
        dev.shift(off)
        dev.set_voxels(ref.q, ref.w)
        world = ppf.World(dev)
        po, no, ko = world.surface(dev, keys=True)
        vx, vn, vres = dev.surface()
        order = WS.dense_order(ko)
        print("rim of 3 at %s: %d points, %d bricks" % (off, len(po), world.last_surface["bricks"]))
        assert world.last_surface["crossings"] == vres["crossings"] and len(po) == vres["points"] > 1000
        assert po[order].tobytes() == vx.tobytes() and no[order].tobytes() == vn.tobytes()
        assert world.last_surface["bricks"] == world.last_surface["window_bricks"] == (135 if off != (3, -5, 2) else 6 * 10 * 4)
        world.close()
        dev.close()


# ---------------------------------------------------------------- the store alone
def ball(lo, centre, radius, side=12, weight=5, scale=4000.0):
    """{g: word} of a block of side^3 seen voxels from lo on whose q is the distance of the voxel's centre g + 0.5 from a
    sphere around centre: a smooth surface with normals wherever the stencil stays inside the block"""
    r = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.array(lo, np.int64)
    d = np.sqrt(((r + 0.5 - np.array(centre, np.float64)) ** 2).sum(axis=1)) - radius
    q = np.clip(np.rint(d * scale), -32767, 32767).astype(np.int16)
    words = q.view(np.uint16).astype(np.uint32) | np.uint32(weight << 16)
    return dict(zip(map(tuple, r.tolist()), words.tolist()))


CORNER = dict(lo=(2, 2, 2), centre=(6.0, 6.0, 6.0), radius=2.2)     # the sphere passes the corner (8, 8, 8) of eight bricks


def test_store_alone(built_lib, ppf):
    sp = (np.float32(0.05), np.array([-1.0, 0.5, 0.25], np.float32))
    store = ball(**CORNER)
    pair = {(100, 100, 100): 2 << 16 | 700, (101, 100, 100): 2 << 16 | (-700 & 0xffff)}      # next to absent bricks
    store.update(pair)
    w = store_of(ppf, store, sp)
    want = WS.world_surface(store, sp, None)
    got = w.surface(keys=True)
    same("the store alone, a ball at the corner (8, 8, 8)", got, want, w.last_surface)
    ko, first = got[2], w.last_surface
    assert first["window_bricks"] == 0 and first["bricks"] == w.stats()["bricks"] == 9 and first["anchor"] == (0, 0, 0)
    for a in range(3):                                              # a crossing on each axis whose two ends lie in different bricks
        assert ((ko[:, 3] == a) & (ko[:, a] == 7)).any(), a
    # one whose stencil, g - 2 .. g + 2 on every axis, spans the corner where the eight bricks meet
    assert ((ko[:, :3] >= 6) & (ko[:, :3] <= 7)).all(axis=1).any()
    # the pair at 100 is counted and has no normal
    assert not (ko[:, 0] >= 100).any()
    only = store_of(ppf, pair, sp)
    assert only.surface()[0].shape == (0, 3) and (only.last_surface["crossings"], only.last_surface["points"]) == (1, 0)
    without = store_of(ppf, ball(**CORNER), sp)
    without.surface()
    assert without.last_surface["crossings"] == first["crossings"] - 1 and without.last_surface["points"] == first["points"]
    # a plane through voxel centres: q = 0 at x = 40, negative below.  The crossing from 39 (i = 7 of its brick) has t = 1
    # exactly, so the read at P + voxel has its base at 41, outside the tile of 12: it goes through the table
    r = np.stack(np.meshgrid(np.arange(34, 46), np.arange(2, 14), np.arange(2, 14), indexing="ij"), -1).reshape(-1, 3)
    q = np.clip((r[:, 0] - 40) * 3000, -32767, 32767).astype(np.int16)
    plane = dict(zip(map(tuple, r.tolist()), (q.view(np.uint16).astype(np.uint32) | np.uint32(9 << 16)).tolist()))
    trace, exact = {}, (np.float32(TH.EXACT["voxel"]), np.array(TH.EXACT["origin"], np.float32))       # a frame without rounding
    want = WS.world_surface(plane, exact, None, trace=trace)
    flat = store_of(ppf, plane, exact)
    same("a plane at x = 40 (%d reads outside the tile)" % trace["outside_tile"], flat.surface(keys=True), want, flat.last_surface)
    assert trace["outside_tile"] >= 64 and len(want[0]) >= 64 and (want[2][:, 0] == 39).all()
    flat.close()
    # entries that a put placed inside the window's box are ignored: the window is unseen there
    ref = TH.exact_frame(S.blank(16, 16, 16), voxel=sp[0], origin=sp[1])
    dev = TS.on_device(ppf, ref)
    dev.shift((0, 0, 8))
    got = w.surface(dev, keys=True)
    want = WS.world_surface(store, sp, H.shifted(ref, (0, 0, 8)))
    same("the same store under an unseen 16^3 window at (0, 0, 8)", got, want, w.last_surface)
    assert 1 < w.last_surface["crossings"] < first["crossings"] and not (got[2][:, 2] >= 8).any()
    for x in (w, only, without, dev):
        x.close()


# ---------------------------------------------------------------- far from the origin
@pytest.mark.parametrize("voxel", [0.001, 0.05])
def test_far_from_the_origin(built_lib, ppf, voxel):
    """2^20 voxels from the origin one ulp of a coordinate is an eighth of a voxel of 1 mm: the trilinear bases that
    rounding puts outside a brick's tile are read through the table.  The restatement counts them."""
    sp = (np.float32(voxel), np.array([0.3, -0.2, 0.1], np.float32))
    for sign in (1, -1):
        c = (sign * (G_FAR - 6), -sign * (G_FAR - 6), sign * (G_FAR - 6))
        store = ball(tuple(x - 6 for x in c), c, 4.3)
        assert max(abs(x) for g in store for x in g) <= G_FAR
        w = store_of(ppf, store, sp)
        near = tuple(int(np.clip(x, -(1 << 20), 1 << 20)) for x in c)
        for anchor in ((0, 0, 0), near):
            trace = {}
            want = WS.world_surface(store, sp, None, 1, anchor, trace=trace)
            got = w.surface(anchor=anchor, keys=True)
            same("voxel %g at %s, anchor %s (%d reads outside the tile)" % (voxel, c, anchor, trace["outside_tile"]), got, want, w.last_surface)
            assert len(want[0]) > 100
            if voxel == 0.05 and anchor == (0, 0, 0):               # 52 428 m from the origin an ulp is 0.08 voxels
                assert trace["outside_tile"] > 0
        w.close()


# ---------------------------------------------------------------- an empty map, and the output conventions
def test_empty_map(built_lib, ppf):
    dev = TS.on_device(ppf, TH.exact_frame(S.blank(16, 24, 16), **FRAME))
    world = ppf.World(dev)
    po, no, ko = world.surface(dev, keys=True)
    assert po.shape == no.shape == (0, 3) and ko.shape == (0, 4)
    assert world.last_surface == dict(world.last_surface, crossings=0, points=0, bricks=12, window_bricks=12, launches=3)
    assert world.surface()[0].shape == (0, 3) and world.last_surface["bricks"] == 0
    world.close()
    dev.close()


def test_output_conventions(built_lib, ppf, chain):
    step = chain["steps"][1]
    dev, world = TS.on_device(ppf, chain["start"]), store_of(ppf, step["store"], chain["sp"])
    dev.shift(H.state(step["vol"])[1])
    dev.set_voxels(step["vol"].q, step["vol"].w)
    lo, hi = WS.bounds(step["store"], step["vol"], margin=3)
    words0, box0, stats0, window0 = dev.voxels(), world.box(lo, hi), world.stats(), dev.window()
    L, n, res = ppf.lib(), C.c_size_t(0), ppf.WorldSurfaceResult()
    want = step["want"][1]
    ppf._check(L.oslam_world_surface(world._h, dev._h, None, None, None, None, 0, C.byref(n), C.byref(res)))       # count only
    assert n.value == res.points == len(want[0]) and res.crossings == want[3] and res.launches == 3
    xyz = np.full((n.value, 3), 7.0, np.float32)
    nrm, key = xyz.copy(), np.full((n.value, 4), 7, np.int32)
    n2 = C.c_size_t(0)
    rc = L.oslam_world_surface(world._h, dev._h, None, ppf._p(xyz), ppf._p(nrm), ppf._p(key), n.value - 1, C.byref(n2), C.byref(res))
    assert rc == ppf.OSLAM_E_LIMIT and n2.value == n.value == res.points and (xyz == 7.0).all() and (nrm == 7.0).all() and (key == 7).all()
    ppf._check(L.oslam_world_surface(world._h, dev._h, None, ppf._p(xyz), ppf._p(nrm), ppf._p(key), n.value, C.byref(n2), C.byref(res)))
    same("through the C-ABI", (xyz, nrm, key), want)
    again = world.surface(dev, keys=True)                           # two calls give equal bits
    assert again[0].tobytes() == xyz.tobytes() and again[1].tobytes() == nrm.tobytes() and again[2].tobytes() == key.tobytes()
    without = world.surface(dev)                                    # key_out is optional
    assert without[0].tobytes() == xyz.tobytes() and without[1].tobytes() == nrm.tobytes()
    other = TR.make_world(ppf, voxel=0.021, origin0=FRAME["origin"])
    with pytest.raises(ppf.OslamError) as e:
        other.surface(dev)
    assert e.value.code == ppf.OSLAM_E_INVALID and "another voxel size or origin" in str(e.value)
    # neither the volume nor the store has changed
    words1 = dev.voxels()
    assert words1[0].tobytes() == words0[0].tobytes() and words1[1].tobytes() == words0[1].tobytes() and dev.window()[0] == window0[0]
    assert world.box(lo, hi).tobytes() == box0.tobytes() and world.stats() == stats0
    for x in (other, world, dev):
        x.close()


# ---------------------------------------------------------------- the scene of the map
def test_scene_from_world_equals_the_steps(built_lib, ppf, chain):
    step = chain["steps"][1]
    dev, both = TS.on_device(ppf, chain["start"]), store_of(ppf, step["store"], chain["sp"])
    dev.shift(H.state(step["vol"])[1])
    dev.set_voxels(step["vol"].q, step["vol"].w)
    alone = store_of(ppf, ball(**CORNER), chain["sp"])
    for world, vol, mw in ((both, dev, 1), (both, dev, 3), (alone, None, 1)):
        xyz, nrm = world.surface(vol, mw)
        assert len(xyz) > 90
        for leaf in (0.0, 0.05):
            got = ppf.Scene.from_world(world, vol, leaf, d_dist=0.04, min_weight=mw)
            want = ppf.Scene(xyz, nrm, d_dist=0.04) if leaf == 0.0 else ppf.Scene(*ppf.voxel_grid(xyz, nrm, leaf=leaf), d_dist=0.04)
            print("leaf %.2f: %d scene points of %d extracted" % (leaf, got.numPoints(), len(xyz)))
            assert got.numPoints() == want.numPoints() > 1 and (leaf == 0.0) == (got.numPoints() == len(xyz))
            for r in (0, got.numPoints() // 2, got.numPoints() - 1):
                assert np.array_equal(got.getHashKeys(r), want.getHashKeys(r)), (leaf, r)
            got.close()
            want.close()
    for x in (alone, both, dev):
        x.close()


# ---------------------------------------------------------------- a stream
def test_stream_with_follow_and_a_store(built_lib, ppf, synth):
    """Volume.step(view, follow=..., world=w) on the stream of tests/shift_calib.py, then the whole map: it has at least
    the window's points and, bit for bit, every point of Volume.surface() whose voxel lies 3 voxels inside the window."""
    pts, traj = E.make_world(synth, 0), E.trajectory(synth, 0)
    cam = V.SMALL_CAM
    ep = ppf.default_egomotion_params(min_overlap=SC.MIN_OVERLAP)
    dev = ppf.Volume(**SC.VOLUME)
    fp = ppf.default_follow_params(dev, **SC.FOLLOW)
    world = ppf.World(dev)
    for T in traj[:5]:
        v = TS.view_of(ppf, E.render(synth, pts, T, **V.SMALL), cam)
        dev.step(v, ep, follow=fp, world=world)
        v.close()
    off = dev.window()[0]
    assert any(off) and world.stats()["voxels"] > 0
    po, no, ko = world.surface(dev, keys=True)
    res = world.last_surface
    vx, vn, vres = dev.surface()
    ref = TS.restated(dev, SC.VOLUME)
    ref.origin0, ref.off = ref.origin.copy(), off
    ref.origin = dev.window()[1]
    wx, wn, wk, _ = TW.dense_points(ref)
    assert wx.tobytes() == vx.tobytes() and wn.tobytes() == vn.tobytes()      # the keys of Volume.surface()'s points
    print("window at %s: the map has %d points in %d bricks (%d of the store), the window %d" % (
        off, len(po), res["bricks"], world.stats()["bricks"], len(vx)))
    assert len(po) >= len(vx) > 0 and res["crossings"] >= vres["crossings"] and res["anchor"] == off
    order = WS.dense_order(ko)
    po, no, ko = po[order], no[order], ko[order]
    a, b = TW.inside(ko, ref), TW.inside(wk, ref)
    assert a.sum() == b.sum() > 100 and ko[a].tobytes() == wk[b].tobytes()
    assert po[a].tobytes() == vx[b].tobytes() and no[a].tobytes() == vn[b].tobytes()
    world.close()
    dev.close()
