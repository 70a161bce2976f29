"""GPU: the marching-cubes mesh of the whole map, voxel store plus window (oslam_world_mesh, World.mesh), against the
numpy restatement of tests/world_mesh_ref.py, bit for bit: vertices, normals, keys, triangle indices, their order and
the counts.  Nothing here has a tolerance.

A workgroup owns one 8 x 8 x 8 brick and finds a triangle corner's vertex in its own brick or in one of the seven
+x/+y/+z neighbours.  The first test puts one cube of every case across the corner where eight bricks meet, so every
corner of every row is looked up in another brick than the cube's; the last but two crosses the boundary between two
chunks of the scan (2^17 table entries)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as M  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_ref as H  # noqa: E402
import surface_ref as S  # noqa: E402
import test_gpu_surface as TS  # noqa: E402
import test_gpu_world_surface as TGW  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import test_world_mesh_host as TM  # noqa: E402
import test_world_surface_host as TW  # noqa: E402
import world_mesh_ref as WM  # noqa: E402
import world_surface_ref as WS  # noqa: E402
from test_gpu_world_surface import chain  # noqa: E402,F401  (the restated shift chain, computed once per module)

pytestmark = pytest.mark.gpu

RAGGED, CHAIN, FRAME = TW.RAGGED, TW.CHAIN, TW.FRAME
SP = (np.float32(0.05), np.array([-1.0, 0.5, 0.25], np.float32))
EXACT = (np.float32(TH.EXACT["voxel"]), np.array(TH.EXACT["origin"], np.float32))       # a frame without rounding
bits = TM.bits


def same(name, got, want, res=None):
    """device (vertices, normals or None, triangles, result, keys) against the restatement's dict, as bits"""
    xyz, nrm, tri, _, keys = got
    if res is not None:
        print("%s: %d vertices, %d triangles, %d cubes (restatement %d, %d, %d), %d bricks of which %d under the window, %d launches" % (
            name, res["vertices"], res["triangles"], res["cubes"], len(want["xyz"]), len(want["tri"]), want["cubes"], res["bricks"],
            res["window_bricks"], res["launches"]))
        assert (res["vertices"], res["triangles"], res["cubes"]) == (len(want["xyz"]), len(want["tri"]), want["cubes"]), name
    assert len(xyz) == len(want["xyz"]) and bits(keys) == bits(want["keys"]), name
    bad = np.flatnonzero((xyz.view(np.uint32) != want["xyz"].view(np.uint32)).any(axis=1))
    assert bad.size == 0, (name, bad[:8], keys[bad[:4]], xyz[bad[:4]], want["xyz"][bad[:4]])
    if nrm is not None:
        bad = np.flatnonzero((nrm.view(np.uint32) != want["nrm"].view(np.uint32)).any(axis=1))
        assert bad.size == 0, (name, bad[:8], keys[bad[:4]], nrm[bad[:4]], want["nrm"][bad[:4]])
    assert tri.dtype == np.uint32 and tri.shape == want["tri"].shape, name
    bad = np.flatnonzero((tri != want["tri"]).any(axis=1))
    assert bad.size == 0, (name, bad[:8], tri[bad[:4]], want["tri"][bad[:4]], want["cube"][bad[:4]])


# ---------------------------------------------------------------- one cube in eight bricks, every case
def case_map(shift=(0, 0, 0)):
    """{g: word}: case c's cube has its corner voxel at (16 * (c % 16) + 7, 16 * (c // 16) + 7, 7), so its eight voxels lie
    in the eight bricks that meet at (16 * (c % 16) + 8, 16 * (c // 16) + 8, 8); corner k is negative iff bit k of c is
    set.  Nothing else is seen.  shift moves the whole map."""
    store = {}
    for c in range(256):
        for k in range(8):
            g = (16 * (c % 16) + 7 + (k & 1) + shift[0], 16 * (c // 16) + 7 + (k >> 1 & 1) + shift[1], 7 + (k >> 2) + shift[2])
            q = -(900 + 37 * k) if c >> k & 1 else 1100 + 53 * k
            store[g] = (2 << 16) | (q & 0xffff)
    return store


def rows_of(mesh, shift=(0, 0, 0)):
    """the cube-edge numbers of every case's triangles, read off the triangles' vertex keys: {case: [(e0, e1, e2), ...]}"""
    keys, out = mesh["keys"].astype(np.int64), {c: [] for c in range(256)}
    for t, g in zip(mesh["tri"].astype(np.int64), mesh["cube"]):
        rel = g - np.array(shift, np.int64)
        c = int(rel[0] // 16 + 16 * (rel[1] // 16))
        assert tuple(rel % 16) == (7, 7, 7) and rel[2] == 7
        row = []
        for v in t:
            d, a = keys[v, :3] - g, int(keys[v, 3])
            lo, hi = [int(d[b]) for b in range(3) if b != a]
            assert d[a] == 0 and lo in (0, 1) and hi in (0, 1)
            row.append(4 * a + lo + 2 * hi)
        out[c].append(tuple(row))
    return out


def test_every_case_across_eight_bricks(built_lib, ppf):
    store = case_map()
    want = WM.world_mesh(store, SP, None)
    assert want["cubes"] == 254 and len(want["tri"]) == int(M.NTRI.sum())
    w = TGW.store_of(ppf, store, SP)
    got = w.mesh(keys=True)
    same("256 cubes, each in eight bricks, the store alone", got, want, w.last_mesh)
    assert w.last_mesh["bricks"] == w.stats()["bricks"] == 16 * 16 * 4 * 2 and w.last_mesh["window_bricks"] == 0
    rows = rows_of(dict(keys=got[4], tri=got[2], cube=want["cube"]))
    for c in range(256):
        assert rows[c] == ppf.mc_table_row(c), c
    # case 128: only corner (8, 8, 8) is negative; the cube's own brick holds no vertex, the three lie in three others
    t = got[2][[i for i, g in enumerate(want["cube"]) if tuple(g) == (7, 16 * 8 + 7, 7)]]
    assert len(t) == 1 and len({tuple(got[4][v, :3] >> 3) for v in t[0]}) == 3
    assert not (got[4][:, :3] >> 3 == np.array([0, 16, 0])).all(axis=1).any()
    # a window that holds the low half of every cube (z = 7), the store the high half
    ref = TH.exact_frame(S.blank(256, 256, 16), voxel=SP[0], origin=SP[1])
    win = H.shifted(ref, (0, 0, -8))
    words = np.zeros((16, 256, 256), np.uint32)
    for g, word in store.items():
        if g[2] == 7:
            words[15, g[1], g[0]] = word
    W.set_words(win, words)
    high = {g: word for g, word in store.items() if g[2] == 8}
    dev = TS.on_device(ppf, ref)
    dev.shift((0, 0, -8))
    dev.set_voxels(win.q, win.w)
    w2 = TGW.store_of(ppf, high, SP)
    want2 = WM.world_mesh(high, SP, win)
    same("the same cubes, low half in a window", w2.mesh(dev, keys=True), want2, w2.last_mesh)
    assert bits(want2["keys"]) == bits(want["keys"]) and bits(want2["tri"]) == bits(want["tri"])
    assert w2.last_mesh["anchor"] == (0, 0, -8) and w2.last_mesh["window_bricks"] == 32 * 32 * 2
    for x in (w, w2, dev):
        x.close()


# ---------------------------------------------------------------- negative and far coordinates
FAR = (1 << 20) + 488             # a brick corner; its brick reaches 2^20 + 495, the store's limit is 2^20 + 512


@pytest.mark.parametrize("shift", [(-8, -8, -8), (FAR - 248,) * 3, (-(FAR + 8),) * 3], ids=["across_zero", "far_positive", "far_negative"])
def test_negative_and_far_coordinates(built_lib, ppf, shift):
    """the map of every case moved so that its cubes straddle g = 0 (bricks -1 and 0), then to the far ends of the
    coordinate range: the cube of case 255 (or 0) stands on the brick corner +-(2^20 + 488)"""
    store = case_map(shift)
    far = max(abs(x) for g in store for x in g)
    assert far <= (1 << 20) + 496 and (shift[0] > -100 or far >= FAR)
    w = TGW.store_of(ppf, store, SP)
    near = tuple(int(np.clip(x, -(1 << 20), 1 << 20)) for x in shift)
    for anchor in ((0, 0, 0), near):
        want = WM.world_mesh(store, SP, None, 1, anchor)
        got = w.mesh(anchor=anchor, keys=True)
        same("every case moved by %s, anchor %s" % (shift, anchor), got, want, w.last_mesh)
        rows = rows_of(dict(keys=got[4], tri=got[2], cube=want["cube"]), shift)
        assert all(rows[c] == [tuple(r) for r in M.ROWS[c]] for c in range(256))
    w.close()


@pytest.mark.parametrize("sign", [1, -1])
def test_a_ball_far_from_the_origin(built_lib, ppf, sign):
    """the ball of the surface's far test, 2^20 + 494 voxels out with a voxel of 0.05: with anchor 0 an ulp of a coordinate
    is 0.08 voxels, so some trilinear bases of the normals fall outside the tile and are read through the table"""
    c = (sign * (TGW.G_FAR - 6), -sign * (TGW.G_FAR - 6), sign * (TGW.G_FAR - 6))
    store = TGW.ball(tuple(x - 6 for x in c), c, 4.3)
    w = TGW.store_of(ppf, store, SP)
    near = tuple(int(np.clip(x, -(1 << 20), 1 << 20)) for x in c)
    for anchor in ((0, 0, 0), near):
        want = WM.world_mesh(store, SP, None, 1, anchor)
        same("a ball at %s, anchor %s" % (c, anchor), w.mesh(anchor=anchor, keys=True), want, w.last_mesh)
        assert (want["nrm"] != 0).any(axis=1).sum() > 100 and len(want["tri"]) > 100
    w.close()


# ---------------------------------------------------------------- the shift chain
@pytest.mark.parametrize("mw,anchor", [(1, None), (3, None), (1, (-5, 9, 2)), (3, (-5, 9, 2))])
def test_shift_chain(built_lib, ppf, chain, mw, anchor):  # noqa: F811
    dev = TS.on_device(ppf, chain["start"])
    world = ppf.World(dev)
    for step in chain["steps"]:
        dev.shift(step["shift"], world)
        want = WM.world_mesh(step["store"], chain["sp"], step["vol"], mw, anchor)
        got = world.mesh(dev, mw, anchor=anchor, keys=True)
        res = world.last_mesh
        same("40x72x24 after %s, min_weight %d, anchor %s" % (step["shift"], mw, anchor), got, want, res)
        assert res["anchor"] == (dev.window()[0] if anchor is None else anchor) and res["launches"] == 6
        if anchor is None:                                          # the vertices with a normal are the surface's points
            wx, wn, wk, wc = step["want"][mw]
            has = (got[1] != 0).any(axis=1)
            assert res["vertices"] == wc and bits(got[0][has]) == bits(wx) and bits(got[1][has]) == bits(wn) and bits(got[4][has]) == bits(wk)
    world.close()
    dev.close()


# ---------------------------------------------------------------- seams, on the device's own triangles
def test_seams_on_the_devices_triangles(built_lib, ppf):
    whole = TGW.store_of(ppf, TM.ball_store(), TM.BALL_SP)
    xyz, nrm, tri, res = whole.mesh()
    TM.assert_closed(tri, len(xyz))
    assert res["bricks"] == whole.stats()["bricks"] == 64 and res["window_bricks"] == 0
    store, win = TM.ball_split()
    half = TGW.store_of(ppf, store, TM.BALL_SP)
    dev = ppf.Volume(16, 24, 24, float(TM.BALL_SP[0]), [float(x) for x in TM.BALL_SP[1]])
    dev.shift(TM.SPLIT_OFF)
    dev.set_voxels(win.q, win.w)
    got = half.mesh(dev, anchor=(0, 0, 0), keys=True)
    same("the ball split by a window face at x = 16", got, WM.world_mesh(store, TM.BALL_SP, win, anchor=(0, 0, 0)), half.last_mesh)
    assert bits(got[0]) == bits(xyz) and bits(got[1]) == bits(nrm) and bits(got[2]) == bits(tri)       # the same map
    TM.assert_closed(got[2], len(got[0]))
    holed_store = TM.without_brick(TM.ball_store())
    holed = TGW.store_of(ppf, holed_store, TM.BALL_SP)
    want = WM.world_mesh(holed_store, TM.BALL_SP, None)
    got = holed.mesh(keys=True)
    same("the ball without the brick %s" % (TM.ABSENT,), got, want, holed.last_mesh)
    n_open = TM.assert_open_only_at(got[2], want["cube"], len(got[0]))
    print("%d vertices, %d triangles closed; without a brick %d triangles with an open edge" % (len(xyz), len(tri), n_open))
    for x in (whole, half, holed, dev):
        x.close()


# ---------------------------------------------------------------- planes through voxel centres
def test_planes_through_voxel_centres(built_lib, ppf):
    """q = 0 at x = 40, negative below: every crossing from x = 39 has t = 1 exactly, so its read at P + voxel has its base
    outside the tile and goes through the table.  Then q = 0 on the plane x + y + z = 60, negative above: the three
    crossings of a zero voxel have t = 0 and coincide, so triangles between them have no area, and they are kept."""
    r = np.stack(np.meshgrid(np.arange(34, 46), np.arange(2, 14), np.arange(2, 14), indexing="ij"), -1).reshape(-1, 3)
    q = np.clip((r[:, 0] - 40) * 3000, -32767, 32767).astype(np.int16)
    plane = dict(zip(map(tuple, r.tolist()), (q.view(np.uint16).astype(np.uint32) | np.uint32(9 << 16)).tolist()))
    want = WM.world_mesh(plane, EXACT, None)
    flat = TGW.store_of(ppf, plane, EXACT)
    same("a plane at x = 40", flat.mesh(keys=True), want, flat.last_mesh)
    assert (want["keys"][:, 0] == 39).all() and (want["nrm"] != 0).any(axis=1).sum() >= 64 and len(want["tri"]) == 2 * 11 * 11
    r = np.stack(np.meshgrid(*[np.arange(14, 27)] * 3, indexing="ij"), -1).reshape(-1, 3)
    q = np.clip((60 - r.sum(axis=1)) * 2500, -32767, 32767).astype(np.int16)
    diag = dict(zip(map(tuple, r.tolist()), (q.view(np.uint16).astype(np.uint32) | np.uint32(9 << 16)).tolist()))
    want = WM.world_mesh(diag, EXACT, None)
    tilted = TGW.store_of(ppf, diag, EXACT)
    got = tilted.mesh(keys=True)
    same("a plane x + y + z = 60", got, want, tilted.last_mesh)
    p = got[0][got[2].astype(np.int64)].view(np.uint32)              # [nt, 3, 3]
    flatness = (p[:, 0] == p[:, 1]).all(axis=1) | (p[:, 1] == p[:, 2]).all(axis=1) | (p[:, 2] == p[:, 0]).all(axis=1)
    print("x + y + z = 60: %d of %d triangles have two equal corners" % (flatness.sum(), len(p)))
    assert flatness.sum() > 50 and not flatness.all()
    flat.close()
    tilted.close()


# ---------------------------------------------------------------- across the scan's chunk boundary
def test_across_the_scan_chunk_boundary(built_lib, ppf):
    """512 x 512 x 264 voxels are 64 x 64 x 33 = 135 168 table entries, more than the 2^17 one scan takes: the boundary
    between entry 2^17 - 1 and entry 2^17 lies between z = 255 and z = 256, through the second ball, so triangles of one
    chunk use vertices of the other.  About 0.6 GB of device memory."""
    t0 = time.time()
    n = (512, 512, 264)
    assert (n[0] // 8) * (n[1] // 8) * (n[2] // 8) == 135168 > 1 << 17
    store = TGW.ball((2, 2, 2), (10.0, 10.0, 10.0), 5.0, side=16)
    store.update(TGW.ball((248, 248, 248), (256.0, 256.0, 256.0), 5.0, side=16))
    g = np.array(list(store.keys()), np.int64)
    words = np.array(list(store.values()), np.uint32)
    q, w = np.zeros((n[2], n[1], n[0]), np.int16), np.zeros((n[2], n[1], n[0]), np.uint16)
    q[g[:, 2], g[:, 1], g[:, 0]] = (words & 0xffff).astype(np.uint16).view(np.int16)
    w[g[:, 2], g[:, 1], g[:, 0]] = (words >> 16).astype(np.uint16)
    dev = ppf.Volume(n[0], n[1], n[2], float(SP[0]), [float(x) for x in SP[1]])
    dev.set_voxels(q, w)
    del q, w
    world = ppf.World(dev)
    got = world.mesh(dev, keys=True)
    res = world.last_mesh
    want = WM.world_mesh(store, SP, None)                           # the same map: what the window does not see is nowhere
    same("two balls in 512 x 512 x 264", got, want, res)
    assert res["bricks"] == res["window_bricks"] == 135168 and res["launches"] == 1 + 1 + 4 + 2
    ez = got[4][:, 2] >> 3
    cz = want["cube"][:, 2] >> 3
    tz = ez[got[2].astype(np.int64)]
    assert (ez == 31).any() and (ez == 32).any() and ((cz == 31) & (tz == 32).any(axis=1)).any()       # a triangle across the boundary
    # Volume.mesh() of the same volume, remapped through the keys
    dx, dn, dtri, dres = dev.mesh()
    xyz, nrm, keys, tkeys = WM.in_dense_order(dict(want, xyz=got[0], nrm=got[1], keys=got[4], tri=got[2]))
    assert (dres["vertices"], dres["triangles"], dres["cubes"]) == (res["vertices"], res["triangles"], res["cubes"])
    assert bits(xyz) == bits(dx) and bits(nrm) == bits(dn) and bits(tkeys) == bits(keys[dtri.astype(np.int64)])
    # the surface of the same map: its counts are scanned in two chunks as well
    po, no, ko = world.surface(dev, keys=True)
    TGW.same("the surface of the same map", (po, no, ko), WS.world_surface(store, SP, None), world.last_surface)
    assert world.last_surface["crossings"] == res["vertices"] and world.last_surface["launches"] == 1 + 1 + 2 + 1
    world.close()
    dev.close()
    print("across the chunk boundary: %.2f s" % (time.time() - t0))


# ---------------------------------------------------------------- the output conventions
def test_output_conventions(built_lib, ppf, chain):  # noqa: F811
    step = chain["steps"][1]
    dev, world = TS.on_device(ppf, chain["start"]), TGW.store_of(ppf, step["store"], chain["sp"])
    dev.shift(H.state(step["vol"])[1])
    dev.set_voxels(step["vol"].q, step["vol"].w)
    lo, hi = WS.bounds(step["store"], step["vol"], margin=3)
    words0, box0, stats0, window0 = dev.voxels(), world.box(lo, hi), world.stats(), dev.window()
    L, nv, nt, res = ppf.lib(), C.c_size_t(0), C.c_size_t(0), ppf.WorldMeshResult()
    want = WM.world_mesh(step["store"], chain["sp"], step["vol"])

    def call(xyz, nrm, key, v_cap, tri, t_cap, n1, n2):
        ptr = lambda a: ppf._p(a) if a is not None else None      # noqa: E731
        return L.oslam_world_mesh(world._h, dev._h, None, ptr(xyz), ptr(nrm), ptr(key), v_cap, ptr(tri), t_cap, C.byref(n1), C.byref(n2),
                                  C.byref(res))

    ppf._check(call(None, None, None, 0, None, 0, nv, nt))          # counts only
    assert (nv.value, nt.value) == (res.vertices, res.triangles) == (len(want["xyz"]), len(want["tri"])) and res.cubes == want["cubes"]
    assert res.launches == 4
    world.surface(dev)
    assert res.vertices == world.last_surface["crossings"]
    xyz = np.full((nv.value, 3), 7.0, np.float32)
    nrm, key, tri = xyz.copy(), np.full((nv.value, 4), 7, np.int32), np.full((nt.value, 3), 7, np.uint32)
    for v_cap, t_cap in ((nv.value - 1, nt.value), (nv.value, nt.value - 1)):
        n1, n2 = C.c_size_t(0), C.c_size_t(0)
        res.vertices = res.triangles = res.cubes = 0
        assert call(xyz, nrm, key, v_cap, tri, t_cap, n1, n2) == ppf.OSLAM_E_LIMIT
        assert (n1.value, n2.value) == (nv.value, nt.value) == (res.vertices, res.triangles) and res.cubes == want["cubes"]
        assert (xyz == 7.0).all() and (nrm == 7.0).all() and (key == 7).all() and (tri == 7).all()
    ppf._check(call(xyz, nrm, key, nv.value, tri, nt.value, nv, nt))
    same("through the C-ABI", (xyz, nrm, tri, None, key), want)
    again = world.mesh(dev, keys=True)                              # two calls give equal bytes
    assert bits(again[0]) == bits(xyz) and bits(again[1]) == bits(nrm) and bits(again[2]) == bits(tri) and bits(again[4]) == bits(key)
    bare = world.mesh(dev, normals=False)                           # nrm_out and key_out are optional
    assert bare[1] is None and bits(bare[0]) == bits(xyz) and bits(bare[2]) == bits(tri) and bare[3]["launches"] == 6
    other = TR.make_world(ppf, voxel=0.021, origin0=FRAME["origin"])
    with pytest.raises(ppf.OslamError) as e:
        other.mesh(dev)
    assert e.value.code == ppf.OSLAM_E_INVALID and "another voxel size or origin" in str(e.value)
    # an empty map under a window, and an empty store alone
    blank = TS.on_device(ppf, TH.exact_frame(S.blank(16, 24, 16), **FRAME))
    nothing = ppf.World(blank)
    out = nothing.mesh(blank, keys=True)
    assert out[0].shape == out[1].shape == (0, 3) and out[2].shape == (0, 3) and out[4].shape == (0, 4)
    assert nothing.last_mesh == dict(nothing.last_mesh, vertices=0, triangles=0, cubes=0, bricks=12, window_bricks=12, launches=4)
    assert nothing.mesh()[2].shape == (0, 3) and nothing.last_mesh["bricks"] == 0 and nothing.last_mesh["launches"] == 0
    # neither the volume nor the store has changed
    words1 = dev.voxels()
    assert bits(words1[0]) == bits(words0[0]) and bits(words1[1]) == bits(words0[1]) and dev.window()[0] == window0[0]
    assert bits(world.box(lo, hi)) == bits(box0) and world.stats() == stats0
    for x in (other, nothing, blank, world, dev):
        x.close()


# ---------------------------------------------------------------- a PLY file
def test_ply_round_trip(built_lib, ppf, tmp_path):
    w = TGW.store_of(ppf, TM.ball_store(), TM.BALL_SP)
    xyz, nrm, tri, res = w.mesh()
    path = str(tmp_path / "world_mesh.ply")
    ppf.ply_write_mesh(path, xyz, nrm, tri)
    px, pn = ppf.ply_read(path)
    assert len(px) == res["vertices"] == len(xyz) > 0 and bits(px) == bits(xyz) and bits(pn) == bits(nrm)
    rx, rn, rt = ppf.ply_read_mesh(path)
    assert bits(rt) == bits(tri) and bits(rx) == bits(xyz)
    w.close()
