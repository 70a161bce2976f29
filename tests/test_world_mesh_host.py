"""CPU: the restatement of the whole map's mesh (tests/world_mesh_ref.py) against the rule of include/oslam.h at
oslam_world_mesh, which pins it to mesh_ref.mesh on a dense padded box and its vertices to world_surface_ref; the
closedness of the mesh across brick seams and a window face; and the symbol, the structure and every refusal of the new
entry point on stand-in handles.  Floats are compared as bits, triangles as key triples in their rotation and order.

No call in this file reaches a device."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as M  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_ref as H  # noqa: E402
import surface_ref as S  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import test_world_surface_host as TW  # noqa: E402
import world_mesh_ref as WM  # noqa: E402
import world_surface_ref as WS  # noqa: E402

RAGGED, CHAIN, FRAME = TW.RAGGED, TW.CHAIN, TW.FRAME


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def equals_dense(mesh, box, min_weight):
    """the map's mesh against mesh_ref.mesh of the dense padded box at the same anchor"""
    key, dx, dn = M.vertices(box, min_weight)
    _, _, dtri, dcubes = M.mesh(box, min_weight)
    dkeys = WM.dense_keys(box, key)
    xyz, nrm, keys, tkeys = WM.in_dense_order(mesh)
    assert len(xyz) == len(dx) > 0 and bits(keys) == bits(dkeys)
    assert bits(xyz) == bits(dx) and bits(nrm) == bits(dn)
    assert mesh["cubes"] == dcubes > 0 and len(tkeys) == len(dtri) > 0
    assert bits(tkeys) == bits(dkeys[dtri.astype(np.int64)])          # the same key triples, rotation and order


# ---------------------------------------------------------------- the restatement against the dense yardstick
def test_the_mesh_of_a_shift_chain_equals_the_dense_volume():
    vol = TW.usual(RAGGED, 31)
    sp = TW.params_of(vol)
    store, cur = {}, vol
    fixed = (-5, 9, 2)                                             # one frame for the whole chain
    first = WM.world_mesh(store, sp, cur, 1, fixed)
    assert len(first["xyz"]) > 50000 and len(first["tri"]) > 50000
    for step, s in enumerate(CHAIN):
        cur, stored, reloaded = W.shift_world(cur, store, s)
        assert stored > 0 or reloaded > 0
        again = WM.world_mesh(store, sp, cur, 1, fixed)            # the map is the same map wherever the window stands
        assert again["cubes"] == first["cubes"] and all(bits(again[k]) == bits(first[k]) for k in ("xyz", "nrm", "keys", "tri", "cube")), s
        lo, hi = WS.bounds(store, cur, margin=3)                   # A = the map's low corner
        box = WS.dense(store, sp, cur, lo, hi, S.blank)
        for mw in (1, 3):
            mesh = WM.world_mesh(store, sp, cur, mw, lo)
            print("after %s, min_weight %d, A = %s: %d vertices, %d triangles, %d cubes" % (s, mw, lo, len(mesh["xyz"]), len(mesh["tri"]),
                                                                                       mesh["cubes"]))
            equals_dense(mesh, box, mw)
    assert H.state(cur)[1] == (0, 0, 0) and not store


def test_vertices_against_the_surface_of_the_map():
    vol = TW.usual(RAGGED, 33)
    sp = TW.params_of(vol)
    store = {}
    cur, _, _ = W.shift_world(vol, store, CHAIN[0])
    cur, _, _ = W.shift_world(cur, store, CHAIN[1])
    for mw, anchor in ((1, None), (3, (-5, 9, 2))):
        mesh = WM.world_mesh(store, sp, cur, mw, anchor)
        wx, wn, wk, crossings = WS.world_surface(store, sp, cur, mw, anchor)
        has = (mesh["nrm"] != 0).any(axis=1)
        assert len(mesh["xyz"]) == crossings > has.sum() == len(wx) > 0
        assert bits(mesh["xyz"][has]) == bits(wx) and bits(mesh["nrm"][has]) == bits(wn) and bits(mesh["keys"][has]) == bits(wk)
        bare = WM.world_mesh(store, sp, cur, mw, anchor, normals=False)
        assert bare["nrm"] is None and all(bits(bare[k]) == bits(mesh[k]) for k in ("xyz", "keys", "tri"))


# ---------------------------------------------------------------- closed across seams
BALL_LO = (4, 4, 4)                                                # mesh_ref.sphere's 24^3 block from here: its centre, voxel
BALL = dict(n=24, voxel=0.05, centre=(0.6, 0.6, 0.6), r=0.33)      # coordinate 12, lies at g = 16, a corner of eight bricks
BALL_SP = (np.float32(0.05), np.array([-1.0, 0.5, 0.25], np.float32))
SPLIT_OFF = (0, 4, 4)                                              # the window of ball_split: its face x = 16 halves the ball
ABSENT = (2, 2, 2)                                                 # the brick 16 <= g < 24 on every axis


def ball_words():
    """uint32 [24, 24, 24] (z, y, x): the words of mesh_ref.sphere's ball"""
    ref = M.sphere(**BALL)
    return W.words_of(ref)


def ball_store(words=None, keep=None):
    """{g: word} of the ball's seen voxels at BALL_LO; keep: bool [24, 24, 24] of the voxels that go to the store"""
    words = ball_words() if words is None else words
    pick = W.seen(words) if keep is None else W.seen(words) & keep
    k, j, i = np.nonzero(pick)
    g = np.stack([i, j, k], axis=1) + np.array(BALL_LO, np.int64)
    return dict(zip(map(tuple, g.tolist()), words[k, j, i].tolist()))


def ball_split():
    """the ball with a window face through its middle: -> (store of x >= 16, window volume of 16 x 24 x 24 at SPLIT_OFF,
    which holds x < 16)"""
    words = ball_words()
    store = ball_store(words, np.broadcast_to(np.arange(24)[None, None, :] >= 12, words.shape))
    win = H.shifted(S.blank(16, 24, 24, voxel=BALL_SP[0], origin=BALL_SP[1]), SPLIT_OFF)
    low = np.zeros((24, 24, 16), np.uint32)
    low[:, :, 4:] = words[:, :, :12]
    W.set_words(win, low)
    return store, win


def without_brick(store, brick=ABSENT):
    return {g: w for g, w in store.items() if tuple(x >> 3 for x in g) != tuple(brick)}


def assert_closed(tri, n_vertices):
    """every directed edge once, its reverse once, and the sphere's Euler characteristic over the referenced vertices"""
    d, own, rev = M.edge_census(tri, n_vertices)
    assert len(tri) > 500 and (own == 1).all() and (rev == 1).all()
    v, e, f = len(np.unique(tri)), len(d) // 2, len(tri)
    assert v - e + f == 2, (v, e, f)


def assert_open_only_at(tri, cube, n_vertices, brick=ABSENT):
    """no directed edge twice; every edge without its reverse lies on a cube that touches the absent brick: the cube's
    corners g .. g + 1 reach the brick's voxels grown by one"""
    d, own, rev = M.edge_census(tri, n_vertices)
    assert (own == 1).all() and (rev <= 1).all()
    is_open = (rev == 0).reshape(3, -1).any(axis=0)                # directed_edges lists the triangles three times over
    lo = np.array(brick, np.int64) * 8
    touches = ((cube + 1 >= lo - 1) & (cube <= lo + 8)).all(axis=1)
    assert is_open.sum() > 8 and touches[is_open].all()
    return int(is_open.sum())


def test_closed_across_brick_seams_and_a_window_face():
    whole = WM.world_mesh(ball_store(), BALL_SP, None)
    b = whole["keys"][:, :3].astype(np.int64) >> 3
    assert len(np.unique(b, axis=0)) >= 8 and len(np.unique(whole["cube"] >> 3, axis=0)) >= 8
    assert_closed(whole["tri"], len(whole["xyz"]))
    store, win = ball_split()
    split = WM.world_mesh(store, BALL_SP, win, anchor=(0, 0, 0))
    assert all(bits(split[k]) == bits(whole[k]) for k in ("xyz", "nrm", "keys", "tri"))      # the same map
    assert_closed(WM.world_mesh(store, BALL_SP, win)["tri"], len(whole["xyz"]))
    holed = WM.world_mesh(without_brick(ball_store()), BALL_SP, None)
    assert 0 < len(holed["tri"]) < len(whole["tri"])
    n_open = assert_open_only_at(holed["tri"], holed["cube"], len(holed["xyz"]))
    print("the ball: %d vertices, %d triangles; without brick %s %d triangles with an open edge" % (
        len(whole["xyz"]), len(whole["tri"]), ABSENT, n_open))


# ---------------------------------------------------------------- ABI and refusals
def test_symbol_structure_and_defaults(built_lib, ppf):
    assert "oslam_world_mesh" in ppf._SIGNATURES and hasattr(ppf.lib(), "oslam_world_mesh")
    assert C.sizeof(ppf.WorldMeshResult) == 40 and C.sizeof(ppf.WorldSurfaceParams) == 48
    assert [f[0] for f in ppf.WorldMeshResult._fields_] == ["vertices", "triangles", "cubes", "bricks", "window_bricks", "launches",
                                                            "anchor", "ms_total"]
    import inspect
    sig = inspect.signature(ppf.World.mesh)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("vol", None), ("min_weight", 1), ("normals", True),
                                                                       ("anchor", None), ("keys", False), ("dev", 0)]


def test_refusals_before_any_device_call(built_lib, ppf):
    L, INV = ppf.lib(), ppf.OSLAM_E_INVALID
    ref = TH.exact_frame(S.blank(16, 16, 16), **FRAME)
    h = TH.stand_in(ppf, ref, off=(8, 0, -8))
    vol = C.byref(h)
    nv, nt, res = C.c_size_t(9), C.c_size_t(9), ppf.WorldMeshResult()
    buf, kbuf, tbuf = np.full((4, 3), 7.0, np.float32), np.full((4, 4), 7, np.int32), np.full((4, 3), 7, np.uint32)
    ok = ppf.default_world_surface_params()
    big = (1 << 20) + 1
    others = [TR.make_world(ppf, **kw) for kw in (dict(voxel=0.021, origin0=FRAME["origin"]), dict(voxel=0.02, origin0=(0.0, 0.1, -1.28)),
                                                  dict(voxel=0.02, origin0=(-0.0, 0.1, -1.2800001)))]
    w = TR.make_world(ppf, voxel=FRAME["voxel"], origin0=FRAME["origin"])
    w.put([(1, 2, 3)], [7 << 16])

    def mesh(wo=w._h, vo=None, sp=ok, xyz=buf, nrm=buf, key=None, v_cap=4, tri=tbuf, t_cap=4, nv_out=C.byref(nv), nt_out=C.byref(nt)):
        ptr = lambda a: ppf._p(a) if a is not None else None      # noqa: E731
        return L.oslam_world_mesh(wo, vo, C.byref(sp) if sp is not None else None, ptr(xyz), ptr(nrm), ptr(key), v_cap, ptr(tri), t_cap,
                                  nv_out, nt_out, C.byref(res))

    assert mesh(wo=None) == mesh(nv_out=None) == mesh(nt_out=None) == INV
    assert mesh(xyz=None) == mesh(tri=None) == INV                  # one of the two without the other
    assert mesh(xyz=None, nrm=None, tri=None, v_cap=4, t_cap=0) == mesh(xyz=None, nrm=None, tri=None, v_cap=0, t_cap=4) == INV
    assert mesh(xyz=None, tri=None, v_cap=0, t_cap=0) == INV        # nrm_out needs the outputs
    assert mesh(xyz=None, nrm=None, tri=None, key=kbuf, v_cap=0, t_cap=0) == INV
    for mw in (0, 65536):
        assert mesh(sp=ppf.default_world_surface_params(min_weight=mw)) == INV
    for a in range(3):
        for bad in (big, -big):
            anchor = [0, 0, 0]
            anchor[a] = bad
            assert mesh(sp=ppf.default_world_surface_params(anchor_set=1, anchor=anchor)) == INV
            assert "2^20" in L.oslam_last_error().decode()
    for other in others:
        assert mesh(wo=other._h, vo=vol) == INV and "another voxel size or origin" in L.oslam_last_error().decode()
    assert nv.value in (0, 9) and nt.value in (0, 9)                # a refused call reports no counts
    assert (buf == 7.0).all() and (tbuf == 7).all() and w.stats()["voxels"] == 1 and tuple(h.off) == (8, 0, -8)
    # an empty store alone is an empty map: no device is asked for anything
    empty = TR.make_world(ppf)
    res.launches = 9
    assert mesh(wo=empty._h, xyz=None, nrm=None, tri=None, v_cap=0, t_cap=0) == 0 and nv.value == nt.value == 0
    assert (res.vertices, res.triangles, res.cubes, res.bricks, res.window_bricks, res.launches, tuple(res.anchor)) == (0, 0, 0, 0, 0, 0, (0, 0, 0))
    assert mesh(wo=empty._h, key=kbuf, sp=ppf.default_world_surface_params(anchor_set=1, anchor=(3, 4, -5))) == 0
    assert nv.value == nt.value == 0 and tuple(res.anchor) == (3, 4, -5) and (buf == 7.0).all() and (kbuf == 7).all() and (tbuf == 7).all()
    out = empty.mesh(keys=True)
    assert out[0].shape == out[1].shape == (0, 3) and out[2].shape == (0, 3) and out[2].dtype == np.uint32 and out[4].shape == (0, 4)
    assert out[3] == empty.last_mesh and empty.last_mesh["vertices"] == 0 and empty.mesh(normals=False)[1] is None
    for x in others + [w, empty]:
        x.close()
