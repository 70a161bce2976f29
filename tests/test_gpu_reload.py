"""GPU: the shift through the voxel store (oslam_volume_shift_world, oslam_volume_pack, Volume.shift(s, world),
Volume.packed and Volume.step(..., world=...)) against the numpy restatement of tests/reload_ref.py, bit for bit: words
are 32-bit integers and nothing here has a tolerance.

The pack kernels give a workgroup 1024 consecutive linear indices: 16^3 is 4 workgroups, 40 x 72 x 24 is 67.5, so the
last run is ragged and, with rows of 40, a chunk straddles rows and slabs.  The words are random over all 32 bits
(test_shift_host.full_range) with a few planted w == 0, q != 0 ones, so a word from a wrong index shows.  Shapes, shifts
and helpers are those of tests/test_gpu_shift.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_calib as SC  # noqa: E402
import shift_ref as H  # noqa: E402
import test_gpu_shift as TG  # noqa: E402
import test_gpu_surface as TS  # noqa: E402
import test_reload_host as TR  # noqa: E402
import test_shift_host as TH  # noqa: E402
import volume_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED = TG.RAGGED
SHAPES = [(16, 16, 16), RAGGED]
IDS = ["16^3", "40x72x24"]


def ten_shifts(n):
    """the shifts of test_gpu_shift.test_words_follow_the_restatement"""
    nx, ny, nz = n
    return [(1, 0, 0), (-1, 0, 0), (4, 0, 0), (3, -5, 2), (0, 8, 0), (0, 0, -(nz - 1)), (nx - 1, 0, 0), (nx, 0, 0),
            (nx + 5, -3, 0), (0, 0, 0)]


def frame(vol):
    return TH.exact_frame(vol, **TG.WORDS_FRAME)


def dev_words(dev):
    q, w = dev.voxels()
    return q.view(np.uint16).astype(np.uint32) | (w.astype(np.uint32) << np.uint32(16))


def same_store(world, store, lo, hi):
    """the device's store equals the restated one inside the box, and holds nothing outside it"""
    return world.box(lo, hi).tobytes() == W.box(store, lo, hi).tobytes() and world.stats()["voxels"] == len(store)


def launches_of(s, stored, reloaded):
    """count and scan, emit when something seen leaves, shift, unpack when something comes back (include/oslam.h)"""
    return 0 if not any(s) else 3 + (stored > 0) + (reloaded > 0)


# ---------------------------------------------------------------- the pack tap
@pytest.mark.parametrize("n", SHAPES, ids=IDS)
def test_pack_tap_equals_the_restatement(built_lib, ppf, n):
    ref = frame(TR.planted(n, 11))
    nx, ny, nz = n
    dev = TS.on_device(ppf, ref)
    for s in ten_shifts(n):
        lin, words = dev.packed(s)
        wl, ww = W.packed(ref, s)
        print("%s, shift %s: %d records (restatement %d)" % (n, s, len(lin), len(wl)))
        assert len(lin) == len(wl) and lin.tobytes() == wl.tobytes() and words.tobytes() == ww.tobytes(), s
        assert (len(lin) == 0) == (not any(s))
    assert TG.same_words(dev, ref) and dev.window()[0] == (0, 0, 0)         # the tap changes nothing
    # nothing seen: q over all of int16, w == 0
    unseen = frame(TH.full_range(n, 12))
    unseen.w[:] = 0
    dev.set_voxels(unseen.q, unseen.w)
    for s in [(3, -5, 2), (nx, 0, 0)]:
        lin, words = dev.packed(s)
        assert len(lin) == len(words) == 0, s
    # everything seen and everything leaves: one record per voxel, the ragged last workgroup included
    full = frame(TH.full_range(n, 13))
    full.w[:] |= 1
    dev.set_voxels(full.q, full.w)
    lin, words = dev.packed((nx, 0, 0))
    assert lin.tobytes() == np.arange(nx * ny * nz, dtype=np.uint32).tobytes() and words.tobytes() == W.words_of(full).tobytes()
    dev.close()


# ---------------------------------------------------------------- an empty store
@pytest.mark.parametrize("n", SHAPES, ids=IDS)
def test_with_an_empty_store_the_window_is_the_plain_shifts(built_lib, ppf, n):
    ref = frame(TR.planted(n, 11))
    dev = TS.on_device(ppf, ref)
    lo, hi = W.window_box(ref)
    for s in ten_shifts(n):
        TG.reload(dev, ref)
        world = ppf.World(dev)
        res = dev.shift(s, world)
        store = {}
        want, stored, reloaded = W.shift_world(ref, store, s)
        plain = H.shifted(ref, s)
        got = dev_words(dev)
        bad = np.flatnonzero((got != W.words_of(plain)).ravel())
        print("%s shifted by %s through an empty store: stored %d (restatement %d), kept %d, %d launches, %d words differ" % (
            n, s, res["stored"], stored, res["kept"], res["launches"], bad.size))
        assert bad.size == 0 and got.tobytes() == W.words_of(want).tobytes(), (s, bad[:8])
        assert TG.same_window(dev, plain) and res["offset"] == plain.off, (s, dev.window())
        assert reloaded == 0 and (res["stored"], res["reloaded"]) == (stored, 0), (s, res)
        assert res["kept"] == (H.kept(want) if any(s) else 0) and res["launches"] == launches_of(s, stored, 0), (s, res)
        assert same_store(world, store, lo, hi), s
        world.close()
    dev.close()


# ---------------------------------------------------------------- out and back
@pytest.mark.parametrize("n", SHAPES, ids=IDS)
def test_out_and_back_restores_the_window_and_empties_the_store(built_lib, ppf, n):
    """The issue's wording is "the original with the unseen words zeroed".  That holds where a voxel left at some point of
    the path; an unseen word with q != 0 that stays in the window all the way moves with it as under oslam_volume_shift
    (rule 2 of the header) and is still there.  test_reload_host.restored states both; a planted word of each kind is in
    the volume."""
    ref = frame(TR.planted(n, 11))
    nx = n[0]
    dev = TS.on_device(ppf, ref)
    world = ppf.World(dev)
    seen = int(W.seen(W.words_of(ref)).sum())
    for path in ([(3, -5, 2), (-3, 5, -2)], TR.CHAIN, [(nx + 5, -3, 0), (-nx - 5, 3, 0)]):
        TG.reload(dev, ref)
        cur, store = ref, {}
        for s in path:
            res = dev.shift(s, world)
            cur, stored, reloaded = W.shift_world(cur, store, s)
            assert dev_words(dev).tobytes() == W.words_of(cur).tobytes() and TG.same_window(dev, cur), (path, s)
            assert (res["stored"], res["reloaded"], res["kept"]) == (stored, reloaded, H.kept(cur)), (path, s, res)
            assert res["launches"] == launches_of(s, stored, reloaded) and world.stats()["voxels"] == len(store), (path, s, res)
        want = TR.restored(ref, path)
        assert dev_words(dev).tobytes() == want.tobytes(), path
        off, org = dev.window()
        assert off == (0, 0, 0) and org.tobytes() == ref.origin.tobytes() and np.signbit(org[0])
        st = world.stats()
        print("%s, path %s: %d of %d seen words back, store %s" % (n, path, res["kept"], seen, st))
        assert res["kept"] == seen and reloaded > 0 and (st["voxels"], st["bricks"], st["lo"], st["hi"]) == (0, 0, (0, 0, 0), (0, 0, 0))
        assert store == {}
    # everything left: every unseen word came back as 0
    assert want.tobytes() == np.where(W.seen(W.words_of(ref)), W.words_of(ref), 0).tobytes()
    world.close()
    dev.close()


# ---------------------------------------------------------------- a seeded store
def test_a_seeded_store_gives_back_exactly_the_entering_region(built_lib, ppf):
    ref = frame(TR.planted(RAGGED, 11))
    dev = TS.on_device(ppf, ref)
    world = ppf.World(dev)
    s = (3, -5, 2)                                                  # the new window is [3, 43) x [-5, 67) x [2, 26) in g
    inside = [(41, 10, 5), (42, 66, 25), (10, -5, 2), (3, -1, 25), (40, 0, 2), (20, 30, 24), (42, -5, 25)]
    outside = [(43, 10, 5), (2, -3, 5), (10, -6, 5), (10, 10, 26), (-1, -1, -1), (41, 67, 5), (10, -5, 1), (-40, -72, -24)]
    overlap = [(10, 10, 10)]                                        # inside both windows: it does not enter and stays stored
    leaving = [(1, 1, 1)]                                           # a voxel that leaves: the leaving word overwrites the seed
    g = inside + outside + overlap + leaving
    words = [(1000 + i) << 16 | i for i in range(len(g))]
    world.put(g, words)
    store = dict(zip(g, words))
    res = dev.shift(s, world)
    want, stored, reloaded = W.shift_world(ref, store, s)
    assert reloaded == len(inside) and (res["stored"], res["reloaded"]) == (stored, reloaded)
    assert res["kept"] == H.kept(want) and res["launches"] == 5
    got = dev_words(dev)
    assert got.tobytes() == W.words_of(want).tobytes() and TG.same_window(dev, want)
    for gg, word in zip(inside, words):
        i, j, k = (gg[a] - s[a] for a in range(3))
        assert int(got[k, j, i]) == word and gg not in store and not world.box(gg, [c + 1 for c in gg]).any(), gg
    for gg in outside + overlap:
        assert int(world.box(gg, [c + 1 for c in gg])[0, 0, 0]) == store[gg] == words[g.index(gg)], gg
    assert int(world.box((1, 1, 1), (2, 2, 2))[0, 0, 0]) == int(W.words_of(ref)[1, 1, 1]) != words[-1]
    assert same_store(world, store, (-48, -80, -32), (56, 88, 40))
    world.close()
    dev.close()


# ---------------------------------------------------------------- with fusion in between
@pytest.fixture(scope="module")
def world_scene(synth):
    return E.make_world(synth, 0), E.trajectory(synth, 0)


def test_fusion_between_the_shifts(built_lib, ppf, synth, world_scene):
    pts, traj = world_scene
    cam = edge_inputs.ragged_cam()
    imgs = [E.render(synth, pts, T, **edge_inputs.RAGGED) for T in traj[:2]]
    dev = TS.fused(ppf, TS.RAGGED_VOL, [(imgs[0], cam)], traj[:1])
    ref = TS.restated(dev, TS.RAGGED_VOL)
    world = ppf.World(dev)
    store = {}
    res = dev.shift((8, -8, 0), world)
    ref, stored, reloaded = W.shift_world(ref, store, (8, -8, 0))
    assert (res["stored"], res["reloaded"]) == (stored, reloaded) == (stored, 0) and TG.same_words(dev, ref)
    T1 = traj[1].astype(np.float32)
    v = TS.view_of(ppf, imgs[1], cam)
    got = dev.integrate(v, T1)["updated"]
    v.close()
    assert got == ref.integrate(V.z_image(imgs[1], cam), cam, T1) > 0 and TG.same_words(dev, ref)
    res = dev.shift((-8, 8, 0), world)
    ref, stored2, reloaded2 = W.shift_world(ref, store, (-8, 8, 0))
    print("40x72x24 fused: %d stored, then %d stored and %d reloaded, store %s" % (stored, stored2, reloaded2, world.stats()))
    assert (res["stored"], res["reloaded"], res["kept"]) == (stored2, reloaded2, H.kept(ref))
    assert TG.same_words(dev, ref) and TG.same_window(dev, ref) and dev.window()[0] == (0, 0, 0)
    assert reloaded2 == stored > 0 and world.stats()["voxels"] == len(store) == stored2
    _, _, sres = TS.check("40x72x24 fused, shifted out and back through the store", dev, ref)
    assert sres["points"] > 100
    world.close()
    dev.close()


# ---------------------------------------------------------------- failure changes nothing
def test_a_refused_shift_changes_nothing(built_lib, ppf):
    ref = frame(TR.planted(RAGGED, 11))
    dev = TS.on_device(ppf, ref)
    s = (3, -5, 2)
    other = TR.make_world(ppf, voxel=0.021, origin0=[float(x) for x in ref.origin])
    small = ppf.World(dev, max_bytes=4096)                          # the table and one brick
    for w in (other, small):
        w.put([(100, 100, 100)], [7 << 16])
    for w, code in ((other, ppf.OSLAM_E_INVALID), (small, ppf.OSLAM_E_LIMIT)):
        before = w.stats()
        with pytest.raises(ppf.OslamError) as e:
            dev.shift(s, w)
        assert e.value.code == code, str(e.value)
        off, org = dev.window()
        assert TG.same_words(dev, ref) and off == (0, 0, 0) and org.tobytes() == ref.origin.tobytes()
        assert w.stats() == before == dict(before, voxels=1, bricks=1)
        assert int(w.box((100, 100, 100), (101, 101, 101))[0, 0, 0]) == 7 << 16
    res = dev.shift(s)                                              # and the plain shift still works
    want = H.shifted(ref, s)
    assert TG.same_words(dev, want) and TG.same_window(dev, want) and res["kept"] == H.kept(want)
    res = dev.shift((-3, 5, -2), ppf.World(dev))                    # as does the one through a store that fits
    assert res["reloaded"] == 0 and res["offset"] == (0, 0, 0)
    other.close()
    small.close()
    dev.close()


# ---------------------------------------------------------------- step
def test_step_with_follow_and_a_store(built_lib, ppf, synth, world_scene):
    """Volume.step(view, follow=..., world=w) on the stream of tests/shift_calib.py next to the same stream without a
    store: the window moves after the same frames as the follow rule restated on the device's own poses, every shift
    moves the words as the restatement does, nothing is appended to Volume.world, and the store holds what the restated
    store holds.  Without world the same stream fills Volume.world as before."""
    pts, traj = world_scene
    cam = V.SMALL_CAM
    ep = ppf.default_egomotion_params(min_overlap=SC.MIN_OVERLAP)
    views = [TS.view_of(ppf, E.render(synth, pts, T, **V.SMALL), cam) for T in traj[:5]]
    plain = ppf.Volume(**SC.VOLUME)
    dev = ppf.Volume(**SC.VOLUME)
    fp = ppf.default_follow_params(dev, **SC.FOLLOW)
    world = ppf.World(dev)
    store, log = {}, []
    shift = dev.shift

    def spy_shift(s, w=None):
        ref = TS.restated(dev, SC.VOLUME)                           # the words and the window before the shift
        ref.origin0 = ref.origin.copy()
        ref.off, ref.origin = dev.window()
        res = shift(s, w)
        log.append((tuple(int(x) for x in s), w, ref, res))
        return res

    dev.shift = spy_shift
    dev.leaving = None                                              # with a store nothing is extracted: a call would fail
    state = V.Volume(**SC.VOLUME)                                   # the window alone: follow reads only its origin
    shifts = 0
    for f, v in enumerate(views):
        n_log = len(log)
        T, r = dev.step(v, ep, follow=fp, world=world)
        Tp, _ = plain.step(v, ep, follow=fp)
        new = log[n_log:]
        s = H.follow(state, T, **SC.FOLLOW) if r is not None and r["ok"] else (0, 0, 0)
        print("frame %d: ok %s, shift %s, window %s, store %s" % (f, None if r is None else r["ok"], s, dev.window()[0], world.stats()))
        if any(s):
            assert len(new) == 1 and new[0][0] == s and new[0][1] is world, (f, s, new)
            before, res = new[0][2], new[0][3]
            want, stored, reloaded = W.shift_world(before, store, s)
            assert TG.same_words(dev, want) and TG.same_window(dev, want)
            assert (res["stored"], res["reloaded"], res["kept"]) == (stored, reloaded, H.kept(want))
            state = H.shifted(state, s)
            shifts += 1
        else:
            assert not new, (f, new)
        assert dev.window()[0] == tuple(getattr(state, "off", (0, 0, 0))) and dev.world == []
        assert world.stats()["voxels"] == len(store)
        if not any(x[3]["reloaded"] for x in log):                 # nothing came back yet: the two volumes hold the same words
            assert T.tobytes() == Tp.tobytes() and plain.window()[0] == dev.window()[0] and len(plain.world) == shifts, f
    assert shifts >= 1 and len(store) > 0 and dev.world == []
    assert len(plain.world) >= 1 and sum(len(p) for p, _ in plain.world) > 0
    dev.reset()                                                     # does not touch the store
    assert dev.window()[0] == (0, 0, 0) and world.stats()["voxels"] == len(store)
    for v in views:
        v.close()
    world.close()
    plain.close()
    dev.close()
