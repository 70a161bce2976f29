"""GPU: the whole map ray-cast back into a view (oslam_world_raycast, oslam_world_track, oslam_world_paint_view;
World.raycast, World.track, World.paint) against the numpy restatement of tests/world_raycast_ref.py, byte for byte: the z
image, the maps, hits, normals, the anchor and the box in force, and the launches.  Nothing here has a tolerance.

The inputs are tests/world_raycast_inputs.py's, and tests/test_world_raycast_host.py asserts on the CPU that they reach
every exit reason of the march, stencils that mix store and window, bases with a local coordinate of 7, samples in absent
bricks that follow samples in present ones and gaps before hits.  Windows of 16^3 and 40 x 72 x 24 at offsets that are no
multiples of 8 and negative on one axis; images of 37 x 21 (a ragged tile edge) and 64 x 16 (exact tiles).

One-line mutations, each built into a scratch copy of the library and this file run against it on an MI355X; every one
stays inside the map's memory.  The tests that then fail:
  the lane's cache never refreshed when the brick changes (wray_find keeps its first answer)
      all fourteen tests of this file
  / 8 for >> 3 in the key of a sample (wray_nearest)
      test_every_case_equals_the_restatement[16^3] and [40x72x24], test_the_store_alone_and_the_empty_map,
      test_pin_a (all three maps), test_pin_b[16^3], test_refusals_change_nothing (its last call)
  r_hi for r_hi - 1 in the slab (wray_march)
      test_every_case_equals_the_restatement (all three maps: "behind" and "random_inside" enter or end at a far face),
      test_pin_a[16^3] and [40x72x24], test_pin_b[16^3] and [40x72x24]
  the store entry inside the window's box not ignored (k_brick_window leaves a voxel whose brick word is seen)
      test_every_case_equals_the_restatement[16^3] and [40x72x24] ("inside_out" reads the planted voxel), test_pin_a[16^3]
      and [40x72x24], test_paint_equals_its_restatement_and_the_volumes_under_pin_b, test_refusals_change_nothing
  the first corner of the trilinear read seen from w >= 2 instead of w > 0 (wray_trilinear; weights here are 1..3)
      all fourteen tests of this file
"""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_ref as H  # noqa: E402
import test_gpu_shift as TG  # noqa: E402
import test_gpu_surface as TS  # noqa: E402
import test_gpu_volume as TV  # noqa: E402
import test_gpu_world_surface as TGW  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_world_colour_host as TC  # noqa: E402
import track_ref as K  # noqa: E402
import volume_ref as V  # noqa: E402
import world_raycast_inputs as I  # noqa: E402
import world_raycast_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint32
MIN_OVERLAP = 0.4               # tests/shift_calib.py's: the window is narrower than the view
NAMES = list(I.SHAPES) + ["random"]


@pytest.fixture(scope="module")
def maps():
    """the analytic maps with their planted entries, and the random map: restated once, never changed"""
    out = {}
    for name in I.SHAPES:
        m = I.analytic(name)
        m["store"], m["planted_g"], m["planted_word"] = I.with_planted(m)
        out[name] = m
    out["random"] = I.random_map()
    return out


def cases_of(m):
    return I.random_cases(m) if m["name"] == "random" else I.cases(m)


def device_volume(ppf, vol):
    """a device volume with the restated window's parameters, offset and words"""
    origin0, off = H.state(vol)
    dev = ppf.Volume(vol.n[0], vol.n[1], vol.n[2], float(vol.voxel), [float(x) for x in origin0], mu=float(vol.mu),
                     max_weight=vol.max_weight)
    dev.shift(off)
    dev.set_voxels(vol.q, vol.w)
    assert dev.window()[0] == tuple(off) and dev.window()[1].tobytes() == vol.origin.tobytes()
    return dev


def device_map(ppf, m, store=None):
    return device_volume(ppf, m["vol"]), TGW.store_of(ppf, m["store"] if store is None else store, m["sp"])


def dev_words(dev):
    q, w = dev.voxels()
    return q.view(np.uint16).astype(U) | (w.astype(U) << U(16))


def cast(ppf, world, dev, case, **kw):
    """World.raycast of a case -> (view, (z, maps [h, w, 8], result dict))"""
    name, T, spec, anchor, box = case
    kw.setdefault("anchor", anchor)
    kw.setdefault("box", box)
    v, res = world.raycast(T, spec["fx"], spec["fy"], spec["cx"], spec["cy"], spec["width"], spec["height"], vol=dev,
                           z_min=I.BASE["z_min"], z_max=I.BASE["z_max"], max_jump=I.BASE["max_jump"], **kw)
    maps, z = ppf.view_maps(v)
    return v, (z, maps, res)


def dense_cast(ppf, dev, case):
    name, T, spec, _, _ = case
    v, res = dev.raycast(T, spec["fx"], spec["fy"], spec["cx"], spec["cy"], spec["width"], spec["height"], z_min=I.BASE["z_min"],
                         z_max=I.BASE["z_max"], max_jump=I.BASE["max_jump"])
    maps, z = ppf.view_maps(v)
    v.close()
    return z, maps, res


def same_bytes(name, got, want):
    """two device results (z, maps, result dict): the same bytes, hits and normals"""
    (gz, gm, gr), (wz, wm, wr) = got, want
    bad = np.argwhere(gz.view(U) != wz.view(U))
    print("%s: %d hits, %d normals (the other %d, %d), %d pixels of z differ" % (name, gr["hits"], gr["normals"], wr["hits"],
                                                                               wr["normals"], len(bad)))
    assert len(bad) == 0, (name, bad[:4], gz[tuple(bad[0])], wz[tuple(bad[0])])
    assert gm.tobytes() == wm.tobytes(), (name, np.argwhere((gm.view(U) != wm.view(U)).any(axis=-1))[:4])
    assert (gr["hits"], gr["normals"]) == (wr["hits"], wr["normals"]), name


def same_as_restatement(name, got, want, launches):
    z, maps, res = got
    wz, wm, wr = want
    same_bytes(name, got, (wz, V.records(wm), wr))
    assert (res["anchor"], res["box_lo"], res["box_hi"]) == (tuple(wr["anchor"]), tuple(wr["box_lo"]), tuple(wr["box_hi"])), (name, res, wr)
    assert res["launches"] == launches, (name, res)


def restated(m, case, store=None, vol="window", **kw):
    name, T, spec, anchor, box = case
    kw.setdefault("anchor", anchor)
    kw.setdefault("box", box)
    return R.raycast(m["store"] if store is None else store, m["sp"], T, I.cam_of(spec), spec["width"], spec["height"],
                     m["vol"] if isinstance(vol, str) else vol, **kw)


# ---------------------------------------------------------------- 1. every case against the restatement
@pytest.mark.parametrize("name", NAMES)
def test_every_case_equals_the_restatement(built_lib, ppf, maps, name):
    m = maps[name]
    dev, world = device_map(ppf, m)
    words, stats = dev_words(dev), world.stats()
    n_table = len(R.table(m["store"], m["vol"]))
    hits = 0
    for case in cases_of(m):
        v, got = cast(ppf, world, dev, case)
        same_as_restatement("%s %s" % (name, case[0]), got, restated(m, case), launches=2)
        assert got[2]["bricks"] == n_table and got[2]["window_bricks"] == int(np.prod(R.window_bricks(m["vol"])[1]))
        v2, again = cast(ppf, world, dev, case)                       # two calls, the same bytes
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
        # a ray-cast view of the map is a view: oslam_view_to_cloud compacts its normals
        po, no = ppf.view_to_cloud(v)
        has = got[1][..., 3] == 1.0
        assert len(po) == got[2]["normals"] == int(has.sum()) and po.tobytes() == got[1][..., :3][has].tobytes()
        assert no.tobytes() == got[1][..., 4:7][has].tobytes()
        hits += got[2]["hits"]
        v.close()
        v2.close()
    assert hits > 100
    assert dev_words(dev).tobytes() == words.tobytes() and world.stats() == stats      # neither changes
    world.close()
    dev.close()


# ---------------------------------------------------------------- 2. the store alone, and the empty map
def test_the_store_alone_and_the_empty_map(built_lib, ppf, maps):
    m = maps["16^3"]
    store = dict(m["store"])
    store.update(W.window_entries(m["vol"]))                          # the whole analytic region as a store
    world = TGW.store_of(ppf, store, m["sp"])
    for case in I.cases(m)[:3]:
        for anchor in (None, (-7, 11, 2)):
            v, got = cast(ppf, world, None, case, anchor=anchor, box=None, mu=I.MU)
            same_as_restatement("the store alone, %s, anchor %s" % (case[0], anchor), got,
                                restated(m, case, store=store, vol=None, anchor=anchor, box=None, mu=I.MU), launches=1)
            assert got[2]["window_bricks"] == 0 and got[2]["bricks"] == world.stats()["bricks"] and got[2]["hits"] > 20
            v.close()
    world.close()
    empty = TR.make_world(ppf, voxel=I.VOXEL, origin0=I.ORIGIN0)
    case = I.cases(m)[0]
    v, (z, mp, res) = cast(ppf, empty, None, case, mu=I.MU, anchor=(3, 4, -5))
    assert not z.any() and not mp.any() and z.shape == (case[2]["height"], case[2]["width"])
    assert (res["hits"], res["normals"], res["bricks"], res["launches"], res["anchor"]) == (0, 0, 0, 0, (3, 4, -5))
    assert ppf.view_to_cloud(v)[0].shape == (0, 3)
    v.close()
    empty.close()


# ---------------------------------------------------------------- 3. pin (a): the dense volume on the device
@pytest.mark.parametrize("name", NAMES)
def test_pin_a_the_dense_volume_gives_the_same_bytes(built_lib, ppf, maps, name):
    m = maps[name]
    lo, hi = I.pin_box(m["store"], m["vol"])
    box = I.dense_of(m["store"], m["sp"], m["vol"], lo, hi, m["vol"].mu)
    dense = device_volume(ppf, box)                                 # the map's voxel, created origin and mu, at offset lo
    assert (dense.params.nx, dense.params.ny, dense.params.nz) == tuple(hi[a] - lo[a] for a in range(3))
    dev, world = device_map(ppf, m)
    hits = 0
    for case in cases_of(m):
        want = dense_cast(ppf, dense, case)
        v, got = cast(ppf, world, dev, case, anchor=lo, box=(lo, hi))
        same_bytes("pin (a), %s %s" % (name, case[0]), got, want)
        assert (got[2]["anchor"], got[2]["box_lo"], got[2]["box_hi"]) == (lo, lo, hi)
        hits += want[2]["hits"]
        v.close()
    assert hits > 100
    for x in (dense, world, dev):
        x.close()


# ---------------------------------------------------------------- 4. pin (b): the window alone; track and paint under it
@pytest.mark.parametrize("name", NAMES)
def test_pin_b_the_window_alone(built_lib, ppf, maps, name):
    m = maps[name]
    dev = device_volume(ppf, m["vol"])
    world = ppf.World(dev)
    wbox = W.window_box(m["vol"])
    hits = 0
    for case in cases_of(m):
        want = dense_cast(ppf, dev, case)
        v, got = cast(ppf, world, dev, case, anchor=None, box=wbox)
        same_bytes("pin (b), %s %s" % (name, case[0]), got, want)
        assert got[2]["anchor"] == H.state(m["vol"])[1] and got[2]["bricks"] == got[2]["window_bricks"]
        hits += want[2]["hits"]
        v.close()
    assert hits > 20
    world.close()
    dev.close()


# ---------------------------------------------------------------- 5. pin (c): the walk, and tracking against the map
@pytest.fixture(scope="module")
def walk(synth):
    """the restated walk: the fused volume, the ray cast kept from it, the store and the window after the shift"""
    vol = V.Volume(**I.WALK_VOL)
    frames = I.walk_frames(synth)
    for img, T in frames:
        vol.integrate(V.z_image(img, V.SMALL_CAM), V.SMALL_CAM, T)
    spec = I.WALK_CAM
    cam = dict(I.cam_of(spec), max_jump=E.MAX_JUMP)
    store = {}
    moved, _, _ = W.shift_world(vol, store, I.WALK_SHIFT)
    world, traj = E.make_world(synth, 0), E.trajectory(synth, 0)
    small = E.render(synth, world, traj[1], **spec)                   # frame 1 at the small camera: what is tracked
    return dict(vol=vol, frames=frames, spec=spec, cam=cam, store=store, moved=moved, sp=(vol.voxel, H.state(vol)[0]), small=small)


def test_pin_c_the_walk_and_tracking_against_the_map(built_lib, ppf, walk):
    s, spec, cam = walk, walk["spec"], walk["cam"]
    dev = ppf.Volume(**I.WALK_VOL)
    for img, T in s["frames"]:
        v = TS.view_of(ppf, img, V.SMALL_CAM)
        assert dev.integrate(v, T)["updated"] > 0
        v.close()
    assert TG.same_words(dev, s["vol"])
    T0 = s["frames"][0][1]
    args = (T0, spec["fx"], spec["fy"], spec["cx"], spec["cy"], spec["width"], spec["height"])
    kw = dict(z_min=cam["z_min"], z_max=cam["z_max"], max_jump=cam["max_jump"])
    kv, kres = dev.raycast(*args, **kw)
    kept = ppf.view_maps(kv)[::-1] + (kres,)
    frame = ppf.View(s["small"], spec["fx"], spec["fy"], spec["cx"], spec["cy"], depth_scale=cam["depth_scale"], **kw)
    ep = ppf.default_egomotion_params(min_overlap=MIN_OVERLAP)
    ppf.egomotion(frame, kv, params=ep)                               # builds the frame's maps
    Tv, rv = dev.track(frame, T0, ep)                                 # the volume's own tracking, before the shift
    world = ppf.World(dev)
    res = dev.shift(I.WALK_SHIFT, world)
    assert res["stored"] > 1000 and TG.same_words(dev, s["moved"])
    box = ((0, 0, 0), s["vol"].n)
    gv, gres = world.raycast(*args, vol=dev, anchor=(0, 0, 0), box=box, **kw)
    got = ppf.view_maps(gv)[::-1] + (gres,)
    same_bytes("pin (c), the walk", got, kept)
    assert kres["normals"] > 1000
    want = R.raycast(s["store"], s["sp"], T0, cam, spec["width"], spec["height"], s["moved"], anchor=(0, 0, 0), box=box)
    same_as_restatement("the walk", got, want, launches=2)
    # oslam_world_track: its glue, bit for bit; the volume's tracking from before the shift; the restatement
    Te, re_ = ppf.egomotion(frame, gv, params=ep)
    Tt, rt = world.track(frame, T0, vol=dev, params=ep, anchor=(0, 0, 0), box=box)
    assert Tt.tobytes() == V.compose(T0, Te).tobytes() and TV.plain(rt) == TV.plain(re_) and rt["launches"] == re_["launches"] + 2
    assert Tt.tobytes() == Tv.tobytes() and TV.plain(rt) == TV.plain(rv) and rt["launches"] == rv["launches"] + 1
    fmaps = K.view_maps(s["small"], cam, cam["max_jump"])
    T32, r32 = R.track(s["store"], s["sp"], fmaps, cam, T0, s["moved"], anchor=(0, 0, 0), box=box, sums="f32",
                     min_overlap=MIN_OVERLAP)
    print("oslam_world_track: %s; the restatement %s" % (TV.plain(rt), r32))
    assert Tt.tobytes() == T32.tobytes() and rt["correspondences"] == r32["correspondences"] > 500 and rt["iterations"] == r32["iterations"]
    assert rt["ok"] == r32["ok"] == 1
    # under pin (b) it is oslam_volume_track: the moved window alone
    Tw, rw = world_of_nothing_track(ppf, dev, frame, T0, ep)
    Tvol, rvol = dev.track(frame, T0, ep)
    assert Tw.tobytes() == Tvol.tobytes() and TV.plain(rw) == TV.plain(rvol)
    # the moved window alone sees less than the map
    av, ares = dev.raycast(*args, **kw)
    assert ares["hits"] < gres["hits"]
    for x in (av, gv, kv, frame, world, dev):
        x.close()


def world_of_nothing_track(ppf, dev, frame, T, ep):
    empty = ppf.World(dev)
    lo, n = dev.window()[0], (dev.params.nx, dev.params.ny, dev.params.nz)
    out = empty.track(frame, T, vol=dev, params=ep, box=(lo, tuple(lo[a] + n[a] for a in range(3))))
    empty.close()
    return out


# ---------------------------------------------------------------- 6. paint
def test_paint_equals_its_restatement_and_the_volumes_under_pin_b(built_lib, ppf, maps):
    m = maps["40x72x24"]
    vol = TC.coloured(copy.copy(m["vol"]), 7)
    keys = list(m["store"].keys())
    cols = TC.colour_words((len(keys), 1, 1), 8).ravel()
    cstore = dict(zip(keys, (int(x) for x in cols)))
    dev = device_volume(ppf, vol)
    dev.enable_colour()
    dev.set_colour_words(vol.c)
    world = TC.make_world(ppf, voxel=float(m["sp"][0]), origin0=[float(x) for x in m["sp"][1]])
    world.put(np.array(keys, np.int32), np.array([m["store"][k] for k in keys], U), cols)
    painted = 0
    for case in I.cases(m)[:3]:
        name, T, spec, anchor, box = case
        v, (z, _, res) = cast(ppf, world, dev, case)
        n = world.paint(v, T, vol=dev, anchor=anchor)
        want = R.paint(m["store"], cstore, m["sp"], z, I.cam_of(spec), T, vol, anchor)
        got = v.colour()
        print("paint %s: %d pixels painted of %d hits" % (name, n, res["hits"]))
        assert got.tobytes() == want.tobytes() and n == int((want != 0).sum()) and not got[z == 0].any()
        painted += n
        # pin (b): an empty colour store and the default anchor paint what the volume paints
        lone = ppf.World(dev, colour=True)
        n_map = lone.paint(v, T, vol=dev)
        a = v.colour()
        assert dev.paint(v, T) == n_map > 0 and a.tobytes() == v.colour().tobytes()
        lone.close()
        v.close()
    assert painted > 300
    world.close()
    dev.close()


# ---------------------------------------------------------------- 7. refusals leave everything as it was
def test_refusals_change_nothing(built_lib, ppf, maps):
    m = maps["16^3"]
    dev, world = device_map(ppf, m)
    words, stats = dev_words(dev), world.stats()
    case = I.cases(m)[0]
    name, T, spec, _, _ = case
    INV, LIM = ppf.OSLAM_E_INVALID, ppf.OSLAM_E_LIMIT
    skew = T.copy()
    skew[0, 1] += 0.3
    big = (1 << 20) + 1
    other = TR.make_world(ppf, voxel=0.051, origin0=I.ORIGIN0)
    other.put([(1, 2, 3)], [7 << 16])

    def call(w=world, vol=dev, T=T, width=spec["width"], height=spec["height"], fx=spec["fx"], z_min=0.1, z_max=10.0, **kw):
        return w.raycast(T, fx, spec["fy"], spec["cx"], spec["cy"], width, height, vol=vol, z_min=z_min, z_max=z_max, **kw)

    for code, kw in ((INV, dict(T=skew)), (INV, dict(fx=0.0)), (INV, dict(z_min=0.0)), (INV, dict(width=0)), (INV, dict(height=16385)),
                     (INV, dict(anchor=(0, big, 0))), (INV, dict(box=((0, 0, 0), (16, 1, 16)))),
                     (INV, dict(box=((0, 0, 0), (16, 16, R.BOX_MAX + 1)))), (INV, dict(box=((-R.BOX_MAX - 1, 0, 0), (16, 16, 16)))),
                     (INV, dict(mu=float("nan"))), (INV, dict(mu=-1.0)), (INV, dict(mu=1.9 * I.VOXEL)), (INV, dict(vol=None)),
                     (INV, dict(w=other)), (LIM, dict(z_max=0.1 + 0.5 * I.MU * 65535.0 * 1.001))):
        with pytest.raises(ppf.OslamError) as e:
            call(**kw)
        assert e.value.code == code, (kw, str(e.value))
    frame = ppf.View(np.full((spec["height"], spec["width"]), 1.0, np.float32), spec["fx"], spec["fy"], spec["cx"], spec["cy"],
                     depth_scale=1.0)
    for kw in (dict(anchor=(big, 0, 0)), dict(mu=0.01), dict(box=((0, 0, 0), (1, 16, 16)))):
        with pytest.raises(ppf.OslamError) as e:
            world.track(frame, T, vol=dev, **kw)
        assert e.value.code == INV
    with pytest.raises(ppf.OslamError) as e:
        world.track(frame, skew, vol=dev)
    assert e.value.code == INV
    for w_, v_ in ((world, dev),):                                    # a plain store and a volume without colour cannot paint
        with pytest.raises(ppf.OslamError) as e:
            w_.paint(frame, T, vol=v_)
        assert e.value.code == INV and not frame.has_colour()
    assert dev_words(dev).tobytes() == words.tobytes() and world.stats() == stats and dev.window()[0] == H.state(m["vol"])[1]
    v, got = cast(ppf, world, dev, case)                              # and the call still works
    same_as_restatement("after the refusals", got, restated(m, case), launches=2)
    for x in (v, frame, other, world, dev):
        x.close()


# ---------------------------------------------------------------- 8. a ray-cast view of the map is a view
def test_a_view_of_the_map_is_taken_by_egomotion_and_view_to_cloud(built_lib, ppf, maps):
    m = maps["40x72x24"]
    dev, world = device_map(ppf, m)
    case = I.cases(m)[1]
    va, a = cast(ppf, world, dev, case)
    vb, b = cast(ppf, world, dev, case)
    T, r = ppf.egomotion(va, vb)
    print("egomotion of a view of the map against itself: %s" % (TV.plain(r),))
    assert 200 < r["correspondences"] <= a[2]["normals"] and np.isfinite(T).all()
    po, no = ppf.view_to_cloud(va)
    assert len(po) == a[2]["normals"]
    for x in (va, vb, world, dev):
        x.close()
