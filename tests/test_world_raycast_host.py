"""CPU: the restatement of the whole map's ray cast (tests/world_raycast_ref.py) against the rule of include/oslam.h at
oslam_world_raycast, which pins it to volume_ref.Volume.raycast: (a) on a dense volume that holds the map over the box,
(b) on the window itself with an empty store, (c) on the volume kept from before a shift through a store.  The inputs are
tests/world_raycast_inputs.py's, shared with tests/test_gpu_world_raycast.py; this file also asserts that they reach the
branches the device test relies on, so that no comparison there is empty.  Then the Python entry points, the structures
and every refusal that comes before a device call, on stand-in handles.  Floats are compared as bytes; nothing here has a
tolerance, and no call reaches a device."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reload_ref as W  # noqa: E402
import shift_ref as H  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import test_world_colour_host as TC  # noqa: E402
import volume_ref as V  # noqa: E402
import world_colour_ref as WC  # noqa: E402
import world_raycast_inputs as I  # noqa: E402
import world_raycast_ref as R  # noqa: E402


def same_view(name, got, want):
    """(z, (V, N, has), counts) twice: the same bytes and the same two counts"""
    (gz, gm, gr), (wz, wm, wr) = got, want
    bad = np.argwhere(gz.view(np.uint32) != wz.view(np.uint32))
    assert bad.size == 0, (name, bad[:4], gz[tuple(bad[0])], wz[tuple(bad[0])])
    assert V.records(gm).tobytes() == V.records(wm).tobytes(), name
    assert (gr["hits"], gr["normals"]) == (wr["hits"], wr["normals"]), (name, gr, wr)


def cast(m, case, store=None, vol="window", **kw):
    name, T, spec, anchor, box = case
    kw.setdefault("anchor", anchor)
    kw.setdefault("box", box)
    return R.raycast(m["store"] if store is None else store, m["sp"], T, I.cam_of(spec), spec["width"], spec["height"],
                     m["vol"] if isinstance(vol, str) else vol, **kw)


@pytest.fixture(scope="module")
def maps():
    """the analytic maps with their planted entries, and the random map"""
    out = {}
    for name in I.SHAPES:
        m = I.analytic(name)
        m["planted_store"], m["planted_g"], m["planted_word"] = I.with_planted(m)
        out[name] = m
    out["random"] = I.random_map()
    return out


# ---------------------------------------------------------------- the inputs reach their branches
def test_the_inputs_reach_every_branch(maps):
    tot = {}
    for name in I.SHAPES:
        m = maps[name]
        off = H.state(m["vol"])[1]
        assert any(x < 0 for x in off) and all(x % 8 for x in off)             # negative keys, and >> 3 is not / 8
        assert (np.array(list(m["store"].keys())) < 0).any()
        for case in I.cases(m):
            tr = {}
            _, _, res = cast(m, case, store=m["planted_store"], trace=tr)
            ex = tr.pop("exit")
            print("%s %s: %d hits, %d normals, %s" % (name, case[0], res["hits"], res["normals"], {k: v for k, v in tr.items() if v}))
            for k, v in tr.items():
                tot[k] = max(tot.get(k, -1), v) if k == "max_step" else tot.get(k, 0) + v
            tot["hits"], tot["normals"] = tot.get("hits", 0) + res["hits"], tot.get("normals", 0) + res["normals"]
            spec = case[2]
            if case[0].startswith("identity"):                        # one column with D_x == 0, one row with D_y == 0
                assert tr["zero_inside"] + tr.get("zero_miss", 0) >= spec["width"] + spec["height"] - 1
            if case[0] == "identity_outside":
                assert tr["zero_miss"] >= 1 and (ex[:, int(spec["cx"])] == "zero_miss").all()
            if case[0] == "identity_inside":
                assert tr.get("zero_miss", 0) == 0 and tr["zero_marched"] >= spec["width"]
            if case[0] == "plus_z":
                assert tr["exhausted"] >= 20
            if case[0] == "behind":
                assert tr["back_face"] >= 100
    print("together:", tot)
    assert tot["hits"] >= 200 and tot["normals"] >= 150
    for reason in ("zero_miss", "empty", "exhausted", "back_face", "trilinear", "hit", "no_normal"):
        assert tot[reason] >= 1, reason
    assert tot["mixed_stencil"] >= 20 and tot["cross_brick"] >= 20 and tot["absent_after_present"] >= 50 and tot["gap_then_hit"] >= 1
    assert tot["max_step"] < 1024                                     # the dense rule's bound is not what ends a ray either
    # the random map: almost every ray ends without a normal, every kind of read is made
    m = maps["random"]
    for case in I.random_cases(m):
        tr = {}
        _, _, res = cast(m, case, trace=tr)
        n_pix = case[2]["width"] * case[2]["height"]
        print("random %s: %s" % (case[0], {k: v for k, v in tr.items() if k != "exit" and v}))
        assert 0 < res["normals"] < n_pix // 10 and tr["cross_brick"] >= 20 and tr["back_face"] >= 20 and tr["trilinear"] >= 20


def test_whole_bricks_are_absent_along_rays(maps):
    for name in I.SHAPES:
        m = maps[name]
        lo, hi = R.default_box(m["planted_store"], m["vol"])
        n_box = np.prod([(hi[a] - lo[a]) // 8 for a in range(3)])
        n_tab = len(R.table(m["planted_store"], m["vol"]))
        print("%s: %d bricks in a bounding box of %d" % (name, n_tab, n_box))
        assert n_tab < 0.7 * n_box


# ---------------------------------------------------------------- pin (a): the dense volume
@pytest.mark.parametrize("name", list(I.SHAPES) + ["random"])
def test_pin_a_a_dense_volume_gives_the_same_bytes(maps, name):
    m = maps[name]
    store = m.get("planted_store", m["store"])
    lo, hi = I.pin_box(store, m["vol"])
    dense = I.dense_of(store, m["sp"], m["vol"], lo, hi, m["vol"].mu)
    assert H.state(dense)[1] == lo and all((hi[a] - lo[a]) % 8 == 0 and 16 <= hi[a] - lo[a] <= 512 for a in range(3))
    hits = 0
    for case in (I.cases(m) if name != "random" else I.random_cases(m)):
        cname, T, spec, _, _ = case
        want = dense.raycast(T, I.cam_of(spec), spec["width"], spec["height"])
        got = cast(m, case, store=store, anchor=lo, box=(lo, hi))
        same_view("%s %s" % (name, cname), got, want)
        assert got[2]["box_lo"] == lo and got[2]["box_hi"] == hi and got[2]["anchor"] == lo
        hits += want[2]["hits"]
    assert hits > 100


# ---------------------------------------------------------------- pin (b): the window alone
@pytest.mark.parametrize("name", list(I.SHAPES) + ["random"])
def test_pin_b_an_empty_store_and_the_windows_box_give_the_windows_ray_cast(maps, name):
    m = maps[name]
    vol = m["vol"]
    wbox = W.window_box(vol)
    hits = 0
    for case in (I.cases(m) if name != "random" else I.random_cases(m)):
        cname, T, spec, _, _ = case
        want = vol.raycast(T, I.cam_of(spec), spec["width"], spec["height"])
        got = cast(m, case, store={}, anchor=None, box=wbox)
        same_view("%s %s" % (name, cname), got, want)
        assert got[2]["anchor"] == H.state(vol)[1]
        hits += want[2]["hits"]
    assert hits > 20


# ---------------------------------------------------------------- the planted entry
def test_the_store_entry_inside_the_window_is_ignored_and_would_matter(maps):
    for name in I.SHAPES:
        m = maps[name]
        g, word = m["planted_g"], m["planted_word"]
        off, n = H.state(m["vol"])[1], m["vol"].n
        assert all(off[a] <= g[a] < off[a] + n[a] for a in range(3)) and g not in m["store"]
        case = I.cases(m)[1]
        with_it, without = cast(m, case, store=m["planted_store"]), cast(m, case)
        same_view(name, with_it, without)
        # in the window itself the same word changes the view: the entry lies where rays read
        changed = W.set_words(H.shifted(m["vol"], (0, 0, 0)), W.words_of(m["vol"]))
        i, j, k = (g[a] - off[a] for a in range(3))
        assert int(W.words_of(changed)[k, j, i]) != word
        words = W.words_of(changed)
        words[k, j, i] = word
        W.set_words(changed, words)
        other = cast(m, case, vol=changed)
        assert other[0].tobytes() != without[0].tobytes() or V.records(other[1]).tobytes() != V.records(without[1]).tobytes()


# ---------------------------------------------------------------- pin (c): the walk
def test_pin_c_the_kept_ray_cast_comes_back_after_a_shift_through_a_store(synth):
    vol = V.Volume(**I.WALK_VOL)
    frames = I.walk_frames(synth)
    for img, T in frames:
        assert vol.integrate(V.z_image(img, V.SMALL_CAM), V.SMALL_CAM, T) > 0
    spec = I.WALK_CAM
    cam = I.cam_of(spec)
    T0 = frames[0][1]
    kept = vol.raycast(T0, cam, spec["width"], spec["height"])
    assert kept[2]["normals"] > 1000
    store = {}
    sp = (vol.voxel, H.state(vol)[0])
    moved, stored, reloaded = W.shift_world(vol, store, I.WALK_SHIFT)
    assert stored > 1000 and reloaded == 0 and H.state(moved)[1] == I.WALK_SHIFT
    got = R.raycast(store, sp, T0, cam, spec["width"], spec["height"], moved, anchor=(0, 0, 0), box=((0, 0, 0), vol.n))
    same_view("the walk", got, kept)
    alone = moved.raycast(T0, cam, spec["width"], spec["height"])         # the moved window alone sees less
    print("the walk: %d hits kept and back, %d from the moved window alone" % (kept[2]["hits"], alone[2]["hits"]))
    assert alone[2]["hits"] < kept[2]["hits"]


# ---------------------------------------------------------------- paint and track
def test_paint_equals_the_dense_coloured_volume(maps):
    m = maps["16^3"]
    vol = TC.coloured(copy.copy(m["vol"]), 7)
    cstore = {g: int(x) for g, x in zip(m["store"], TC.colour_words((len(m["store"]), 1, 1), 8).ravel())}
    case = I.cases(m)[1]
    _, T, spec, anchor, _ = case
    z = cast(m, case)[0]
    lo, hi = WC.coloured_bounds(m["store"], cstore, vol)
    dense = WC.dense(m["store"], cstore, m["sp"], vol, lo, hi, TC.blank_coloured)
    want = dense.paint(z, I.cam_of(spec), T)
    got = R.paint(m["store"], cstore, m["sp"], z, I.cam_of(spec), T, vol, anchor=lo)
    assert got.tobytes() == want.tobytes() and (got >> 24 != 0).sum() > 100 and not got[z == 0].any()


def test_track_is_the_volumes_glue_under_pin_b(maps):
    m = maps["16^3"]
    _, T, spec, _, _ = I.cases(m)[0]
    cam = I.cam_of(spec)
    frame = m["vol"].raycast(T, cam, spec["width"], spec["height"])[1]
    want = m["vol"].track(frame, cam, T)
    got = R.track({}, m["sp"], frame, cam, T, m["vol"], box=W.window_box(m["vol"]))
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]


# ---------------------------------------------------------------- the library: entry points, structures, refusals
def test_structures_signatures_and_python_surface(built_lib, ppf):
    import inspect
    assert C.sizeof(ppf.WorldRaycastParams) == 76 and C.sizeof(ppf.WorldRaycastResult) == 60
    p = ppf.WorldRaycastParams()
    p.mu = 3.0
    assert ppf.lib().oslam_world_raycast_params_default(C.byref(p)) == 0
    assert (p.anchor_set, p.box_set, p.mu, p.dev, list(p.reserved)) == (0, 0, 0.0, 0, [0] * 6)
    assert ppf.lib().oslam_world_raycast_params_default(None) == ppf.OSLAM_E_INVALID
    for name in ("oslam_world_raycast", "oslam_world_track", "oslam_world_paint_view", "oslam_world_raycast_params_default"):
        assert name in ppf._SIGNATURES
    assert list(inspect.signature(ppf.World.raycast).parameters) == [
        "self", "T_vol_cam", "fx", "fy", "cx", "cy", "width", "height", "vol", "anchor", "box", "mu", "z_min", "z_max", "max_jump",
        "dev"]
    assert list(inspect.signature(ppf.World.track).parameters)[:5] == ["self", "view", "T_prev", "vol", "params"]
    assert list(inspect.signature(ppf.World.paint).parameters) == ["self", "view", "T_vol_cam", "vol", "anchor"]


def test_refusals_before_any_device_call(built_lib, ppf):
    L, INV, LIM = ppf.lib(), ppf.OSLAM_E_INVALID, ppf.OSLAM_E_LIMIT
    frame = dict(voxel=0.02, origin=(-0.0, 0.1, -1.28))
    ref = TH.exact_frame(V.Volume(16, 16, 16, 0.02, [0.0, 0.0, 0.0], mu=0.08), **frame)
    h = TH.stand_in(ppf, ref, off=(8, 0, -8))
    vol = C.byref(h)
    w = TR.make_world(ppf, voxel=frame["voxel"], origin0=frame["origin"])
    w.put([(1, 2, 3)], [7 << 16])
    others = [TR.make_world(ppf, **kw) for kw in (dict(voxel=0.021, origin0=frame["origin"]), dict(voxel=0.02, origin0=(0.0, 0.1, -1.28)))]
    eye = np.eye(4, dtype=np.float32)
    skew = eye.copy()
    skew[0, 1] = 0.3
    good = ppf.Camera(30.0, 30.0, 18.0, 10.0, 1.0, 0.1, 10.0, 0.05)
    out, res = C.c_void_p(0), ppf.WorldRaycastResult()

    def params(**kw):
        p = ppf.World._raycast_params(kw.pop("anchor", None), kw.pop("box", None), kw.pop("mu", 0.0), 0)
        assert not kw
        return p

    def ray(wo=w._h, vo=vol, rp=None, T=eye, cam=good, width=37, height=21, o=C.byref(out)):
        rp = params() if rp is None else rp
        return L.oslam_world_raycast(wo, vo, C.byref(rp), ppf._p(T) if T is not None else None, C.byref(cam) if cam is not None else None,
                                     width, height, o, C.byref(res))

    assert ray(wo=None) == ray(T=None) == ray(cam=None) == ray(o=None) == INV
    assert ray(T=skew) == INV
    for bad in (ppf.Camera(0.0, 30.0, 18.0, 10.0, 1.0, 0.1, 10.0, 0.05), ppf.Camera(30.0, 30.0, 18.0, 10.0, 1.0, 0.0, 10.0, 0.05),
                ppf.Camera(30.0, 30.0, 18.0, 10.0, 1.0, 2.0, 1.0, 0.05), ppf.Camera(30.0, 30.0, float("nan"), 10.0, 1.0, 0.1, 10.0, 0.05)):
        assert ray(cam=bad) == INV
    assert ray(width=0) == ray(height=0) == ray(width=16385) == ray(height=16385) == INV
    big = (1 << 20) + 1
    for a in range(3):
        for bad in (big, -big):
            anchor = [0, 0, 0]
            anchor[a] = bad
            assert ray(rp=params(anchor=anchor)) == INV and "2^20" in L.oslam_last_error().decode()
        lo, hi = [0, 0, 0], [16, 16, 16]
        hi[a] = 1
        assert ray(rp=params(box=(lo, hi))) == INV and "2 voxels" in L.oslam_last_error().decode()
        hi[a] = 0
        assert ray(rp=params(box=(lo, hi))) == INV
        for corner in (R.BOX_MAX + 1, -R.BOX_MAX - 1):
            lo, hi = [0, 0, 0], [16, 16, 16]
            (lo if corner < 0 else hi)[a] = corner
            assert ray(rp=params(box=(lo, hi))) == INV and "520" in L.oslam_last_error().decode()
    for mu in (float("nan"), float("inf"), -0.1, 0.039):             # 2 voxels are 0.04
        assert ray(rp=params(mu=mu)) == INV, mu
    assert ray(vo=None) == INV and "mu" in L.oslam_last_error().decode()          # mu == 0 without a volume
    assert ray(vo=None, rp=params(mu=0.039)) == INV
    for other in others:
        assert ray(wo=other._h) == INV and "another voxel size or origin" in L.oslam_last_error().decode()
    # the step bound: (z_max - z_min) / (mu / 2) >= 65535 is OSLAM_E_LIMIT, by the volume's mu and by a set one
    far = ppf.Camera(30.0, 30.0, 18.0, 10.0, 1.0, 0.1, 0.1 + 0.04 * 65535.0 * 1.001, 0.05)
    assert ray(cam=far) == LIM and "65535" in L.oslam_last_error().decode()
    assert ray(cam=far, vo=None, rp=params(mu=0.08)) == LIM
    assert R.steps_refused(dict(z_min=0.1, z_max=0.1 + 0.04 * 65535.0 * 1.001), 0.08) and not R.steps_refused(I.BASE, 0.08)
    assert not out.value and w.stats()["voxels"] == 1 and tuple(h.off) == (8, 0, -8)

    # track: the view is a zeroed stand-in with the camera of a view in it
    class KView(C.Structure):
        _fields_ = [("z", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                    ("cy", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float)]

    class ViewHandle(C.Structure):
        _fields_ = [("dev", C.c_int), ("k", KView), ("d_z", C.c_void_p), ("max_jump", C.c_float), ("d_maps", C.c_void_p),
                    ("d_colour", C.c_void_p)]

    v = ViewHandle()
    v.k.w, v.k.h, v.k.fx, v.k.fy, v.k.cx, v.k.cy, v.k.z_min, v.k.z_max, v.max_jump = 37, 21, 30.0, 30.0, 18.0, 10.0, 0.1, 10.0, 0.05
    To, ego = np.full(16, 7.0, np.float32), ppf.EgomotionResult()

    def trk(wo=w._h, vo=vol, rp=None, view=C.byref(v), T=eye, To=To):
        rp = params() if rp is None else rp
        return L.oslam_world_track(wo, vo, C.byref(rp), view, ppf._p(T) if T is not None else None, None,
                                   ppf._p(To) if To is not None else None, C.byref(ego))

    assert trk(wo=None) == trk(view=None) == trk(T=None) == trk(To=None) == trk(T=skew) == INV
    assert trk(rp=params(anchor=(big, 0, 0))) == trk(rp=params(mu=0.01)) == trk(vo=None) == trk(wo=others[0]._h) == INV
    h.dev = 1
    assert trk() == INV and "different devices" in L.oslam_last_error().decode()
    h.dev = 0
    assert (To == 7.0).all()

    # paint: oslam_world_colours' refusals and oslam_volume_paint_view's
    painted = C.c_uint32(9)
    cw = TC.make_world(ppf, voxel=frame["voxel"], origin0=frame["origin"])
    cvol = TC.stand_in_volume(ppf, ref, off=(8, 0, -8), colour=True)
    bare = TC.stand_in_volume(ppf, ref, off=(8, 0, -8))
    cother = TC.make_world(ppf, voxel=0.021, origin0=frame["origin"])

    def paint(wo=cw._h, vo=cvol, sp=None, T=eye, view=C.byref(v)):
        return L.oslam_world_paint_view(wo, vo, C.byref(sp) if sp is not None else None, ppf._p(T) if T is not None else None, view,
                                        C.byref(painted))

    assert paint(wo=None) == paint(T=None) == paint(view=None) == paint(T=skew) == INV
    assert paint(sp=ppf.default_world_surface_params(anchor_set=1, anchor=(0, -big, 0))) == INV
    assert paint(sp=ppf.default_world_surface_params(min_weight=0)) == INV
    assert paint(wo=w._h) == INV and "keeps no colour" in L.oslam_last_error().decode()
    assert paint(vo=bare) == INV and "has no colour" in L.oslam_last_error().decode()
    assert paint(wo=cother._h) == INV and "another voxel size or origin" in L.oslam_last_error().decode()
    for x in others + [w, cw, cother]:
        x.close()
