"""GPU: the shifting window (oslam_volume_shift, oslam_volume_window, oslam_volume_leaving, oslam_volume_follow and
Volume.step(..., follow=...)) against the numpy restatement of tests/shift_ref.py, bit for bit.

k_tsdf_shift gives a thread four consecutive words of a row: 16^3 has rows of 4 threads, 40 x 72 x 24 rows of 10, no
multiple of a wave, and 17 280 quads, 67.5 workgroups.  The words are random over all 32 bits, so a load from a wrong
index shows, a row's end that reads the next row's start included.  The extraction's shapes are those of
tests/test_gpu_surface.py, whose helpers are used here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import mesh_ref as M  # noqa: E402
import shift_calib as SC  # noqa: E402
import shift_ref as H  # noqa: E402
import surface_ref as S  # noqa: E402
import test_gpu_mesh as TM  # noqa: E402
import test_gpu_surface as TS  # noqa: E402
import test_shift_host as TH  # noqa: E402
import volume_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
RAGGED = (40, 72, 24)
WORDS_FRAME = dict(voxel=0.02, origin=(-0.0, 0.1, -1.28))          # a -0.0 that has to come back with its sign


def same_window(dev, ref):
    off, org = dev.window()
    return off == tuple(ref.off) and org.tobytes() == ref.origin.tobytes()


def same_words(dev, ref):
    q, w = dev.voxels()
    return q.tobytes() == ref.q.tobytes() and w.tobytes() == ref.w.tobytes()


def reload(dev, ref):
    dev.reset()
    dev.set_voxels(ref.q, ref.w)


# ---------------------------------------------------------------- words
@pytest.mark.parametrize("n", [(16, 16, 16), RAGGED], ids=["16^3", "40x72x24"])
def test_words_follow_the_restatement(built_lib, ppf, n):
    ref = TH.exact_frame(TH.full_range(n, 11), **WORDS_FRAME)
    nx, ny, nz = n
    dev = TS.on_device(ppf, ref)
    assert dev.window()[0] == (0, 0, 0) and dev.window()[1].tobytes() == ref.origin.tobytes()
    for s in [(1, 0, 0), (-1, 0, 0), (4, 0, 0), (3, -5, 2), (0, 8, 0), (0, 0, -(nz - 1)), (nx - 1, 0, 0), (nx, 0, 0),
              (nx + 5, -3, 0), (0, 0, 0)]:
        reload(dev, ref)
        res = dev.shift(s)
        want = H.shifted(ref, s)
        q, w = dev.voxels()
        bad = np.flatnonzero((q != want.q).ravel() | (w != want.w).ravel())
        print("%s shifted by %s: kept %d (restatement %d), %d words differ" % (n, s, res["kept"], H.kept(want), bad.size))
        assert bad.size == 0, (s, bad[:8])
        assert same_window(dev, want) and res["offset"] == want.off, (s, dev.window())
        if any(s):
            assert (res["kept"], res["launches"]) == (H.kept(want), 1), (s, res)
        else:
            assert (res["kept"], res["launches"]) == (0, 0), res
    # two shifts in a row are the restatement applied twice: the second reads what the first wrote into the other buffer
    reload(dev, ref)
    want = ref
    for s in [(3, -5, 2), (-7, 1, 1), (4, 8, -2)]:
        res = dev.shift(s)
        want = H.shifted(want, s)
        assert same_words(dev, want) and same_window(dev, want) and res["kept"] == H.kept(want), s
    # out and back: offset 0, the created origin's bits (the sign of -0.0 included), only the overlap survives
    reload(dev, ref)
    dev.shift((3, -5, 2))
    res = dev.shift((-3, 5, -2))
    want = H.shifted(H.shifted(ref, (3, -5, 2)), (-3, 5, -2))
    off, org = dev.window()
    assert off == (0, 0, 0) == res["offset"] and org.tobytes() == ref.origin.tobytes() and np.signbit(org[0])
    assert same_words(dev, want) and 0 < res["kept"] == H.kept(want) < H.kept(ref)
    # the offset's limit on a live volume: nothing changes
    dev.shift((1 << 20, 0, 0))
    assert dev.window()[0] == (1 << 20, 0, 0) and not dev.voxels()[1].any()
    dev.set_voxels(ref.q, ref.w)
    with pytest.raises(ppf.OslamError) as e:
        dev.shift((1, 0, 0))
    assert e.value.code == ppf.OSLAM_E_INVALID and dev.window()[0] == (1 << 20, 0, 0) and same_words(dev, ref)
    dev.reset()
    assert dev.window()[0] == (0, 0, 0) and dev.window()[1].tobytes() == ref.origin.tobytes() and not dev.voxels()[1].any()
    dev.close()


# ---------------------------------------------------------------- the stages after a shift
@pytest.fixture(scope="module")
def world(synth):
    return E.make_world(synth, 0), E.trajectory(synth, 0)


def test_the_stages_follow_the_moved_origin(built_lib, ppf, synth, world):
    """integrate, raycast, surface and mesh on a shifted volume against their restatements on the shifted restated
    volume: the kernels read the origin from the volume and are not edited"""
    pts, traj = world
    cam = edge_inputs.ragged_cam()
    imgs = [E.render(synth, pts, T, **edge_inputs.RAGGED) for T in traj[:4]]
    dev = TS.fused(ppf, TS.RAGGED_VOL, [(im, cam) for im in imgs[:3]], traj[:3])
    ref = H.shifted(TS.restated(dev, TS.RAGGED_VOL), (8, -8, 0))
    res = dev.shift((8, -8, 0))
    assert same_words(dev, ref) and same_window(dev, ref) and res["kept"] == H.kept(ref) > 0
    T3 = traj[3].astype(np.float32)
    v = TS.view_of(ppf, imgs[3], cam)
    got = dev.integrate(v, T3)["updated"]
    assert got == ref.integrate(V.z_image(imgs[3], cam), cam, T3) > 0 and same_words(dev, ref)
    v.close()
    h, w = imgs[0].shape
    rv, rres = dev.raycast(T3, cam["fx"], cam["fy"], cam["cx"], cam["cy"], w, h, z_min=cam["z_min"], z_max=cam["z_max"],
                           max_jump=E.MAX_JUMP)
    maps, z = ppf.view_maps(rv)
    wz, wmaps, wcnt = ref.raycast(T3, cam, w, h)
    print("shifted 40x72x24: %d voxels updated, ray cast %d hits %d normals" % (got, rres["hits"], rres["normals"]))
    assert z.tobytes() == wz.tobytes() and maps.tobytes() == V.records(wmaps).tobytes()
    assert (rres["hits"], rres["normals"]) == (wcnt["hits"], wcnt["normals"]) and rres["hits"] > 0
    rv.close()
    _, _, sres = TS.check("shifted 40x72x24", dev, ref)
    TM.check("shifted 40x72x24", dev, ref)
    assert sres["points"] > 100
    dev.close()


# ---------------------------------------------------------------- what leaves
def check_leaving(ppf, name, dev, ref, s, min_weight=1, verts=None):
    """leaving against the restatement, twice, and the partition of the device's own crossings by the shift itself;
    the volume comes back as it was.  verts: mesh_ref.vertices(ref, min_weight), computed once per volume"""
    xyz, nrm, res = dev.leaving(s, min_weight)
    wx, wn, wc = H.leaving(ref, s, min_weight, verts)
    print("%s, shift %s, min_weight %d: %d crossings and %d points leave (restatement %d, %d)" % (
        name, s, min_weight, res["crossings"], res["points"], wc, len(wx)))
    assert (res["crossings"], res["points"]) == (wc, len(wx)) and len(xyz) == len(wx), (name, s)
    assert xyz.tobytes() == wx.tobytes() and nrm.tobytes() == wn.tobytes(), (name, s)
    xyz2, nrm2, res2 = dev.leaving(s, min_weight)
    assert xyz2.tobytes() == xyz.tobytes() and nrm2.tobytes() == nrm.tobytes() and res2["crossings"] == res["crossings"]
    assert same_words(dev, ref)                                     # leaving changes nothing
    before = dev.surface(min_weight)[2]["crossings"]
    dev.shift(s)
    after = dev.surface(min_weight)[2]["crossings"]
    print("    %d crossings before = %d leaving + %d after" % (before, res["crossings"], after))
    assert before == res["crossings"] + after, (name, s, before, res["crossings"], after)
    reload(dev, ref)
    return xyz, nrm, res


SMALL_SHIFTS = [(3, -5, 2), (1, 0, 0), (0, 0, -23), (-8, 8, 0), (40, 0, 0)]


@pytest.mark.parametrize("unseen", [0.0, 0.02])
def test_leaving_of_random_signs(built_lib, ppf, unseen):
    ref = M.random_signs(*RAGGED, 5, unseen)
    dev = TS.on_device(ppf, ref)
    for mw in (1, 3):
        sx, sn, sres = dev.surface(mw)
        verts = M.vertices(ref, mw)
        for s in SMALL_SHIFTS:
            xyz, nrm, res = check_leaving(ppf, "40x72x24 random signs, %.0f %% unseen" % (100 * unseen), dev, ref, s, mw, verts)
            assert 0 < res["crossings"] and res["points"] <= res["crossings"] and (s != (3, -5, 2) or res["points"] > 0)
            if s == (40, 0, 0):                                     # the whole volume: the surface itself, byte for byte
                assert xyz.tobytes() == sx.tobytes() and nrm.tobytes() == sn.tobytes()
                assert (res["crossings"], res["points"]) == (sres["crossings"], sres["points"])
        xyz, _, res = dev.leaving((0, 0, 0), mw)
        assert len(xyz) == 0 and (res["crossings"], res["points"]) == (0, 0)
    # cap one below the count and cap 0 with outputs: OSLAM_E_LIMIT, the count in n_out, nothing written; NULL outputs count
    L = ppf.lib()
    s = np.array([3, -5, 2], np.int32)
    _, _, res = dev.leaving(s)
    for cap in (res["points"] - 1, 0):
        po = np.full((res["points"], 3), 7.0, np.float32)
        no, n, r = po.copy(), C.c_size_t(0), ppf.SurfaceResult()
        rc = L.oslam_volume_leaving(dev._h, ppf._p(s), None, ppf._p(po), ppf._p(no), cap, C.byref(n), C.byref(r))
        assert rc == ppf.OSLAM_E_LIMIT and n.value == res["points"] == r.points and r.crossings == res["crossings"]
        assert (po == 7.0).all() and (no == 7.0).all()
    n = C.c_size_t(0)
    ppf._check(L.oslam_volume_leaving(dev._h, ppf._p(s), None, None, None, 0, C.byref(n), None))
    assert n.value == res["points"]
    dev.close()


def test_leaving_of_the_checkerboard(built_lib, ppf):
    ref = S.checkerboard()
    dev = TS.on_device(ppf, ref)
    verts = M.vertices(ref)
    for s in SMALL_SHIFTS + [(0, 0, -15), (16, 0, 0)]:             # (0, 0, -23) and (40, 0, 0) clear 16^3 as (16, 0, 0) does
        _, _, res = check_leaving(ppf, "16^3 checkerboard", dev, ref, s, verts=verts)
        if s == (1, 0, 0):                                          # the plane i = 0 goes: its y and z edges and the x edges out of it
            assert res["crossings"] == 2 * 16 * 15 + 16 * 16
        if s in ((16, 0, 0), (40, 0, 0), (0, 0, -23)):
            assert res["crossings"] == 11520
    dev.close()


def test_leaving_of_a_fused_volume_with_more_workgroups_than_a_scan_tile(built_lib, ppf, synth, world):
    pts, traj = world
    dev = TS.fused(ppf, TS.BIG, [(E.render(synth, pts, traj[0]), E.CAM)], traj[:1])
    ref = TS.restated(dev, TS.BIG)
    xyz, nrm, res = dev.leaving((8, -16, 24))
    wx, wn, wc = H.leaving(ref, (8, -16, 24))
    print("128^3 fused from a 640x480 frame, shift (8, -16, 24): %d crossings and %d points leave" % (res["crossings"], res["points"]))
    assert (res["crossings"], res["points"]) == (wc, len(wx)) and res["points"] > 0
    assert xyz.tobytes() == wx.tobytes() and nrm.tobytes() == wn.tobytes()
    before = dev.surface()[2]["crossings"]
    dev.shift((8, -16, 24))
    assert before == res["crossings"] + dev.surface()[2]["crossings"]
    dev.close()


def test_positions_that_stay_are_the_same_bytes(built_lib, ppf):
    """voxel 1/16 and an origin on its grid: every voxel centre is exact in float32 before and after the shift, so the
    mesh's vertices (every crossing, in order) minus the leaving ones are the vertices after it, byte for byte.  With
    voxel 0.05 the counts partition in the same way and the positions may differ in the last bit: counts only."""
    s = (3, -5, 2)
    for exact in (True, False):
        ref = M.random_signs(*RAGGED, 5, 0.02)
        if exact:
            TH.exact_frame(ref)
        dev = TS.on_device(ppf, ref)
        before = dev.mesh(normals=False)[0]
        key = M.vertices(ref, 1, normals=False)[0]
        gone = H.leaving_keys(ref, key, s)
        _, _, res = dev.leaving(s)
        dev.shift(s)
        after = dev.mesh(normals=False)[0]
        print("voxel %s: %d vertices = %d leaving + %d after" % (float(ref.voxel), len(before), res["crossings"], len(after)))
        assert len(before) == len(key) and res["crossings"] == int(gone.sum()) and len(after) == len(before) - res["crossings"]
        if exact:
            assert (len(before), res["crossings"], len(after)) == (96489, 20601, 75888)
            assert before[~gone].tobytes() == after.tobytes()
        dev.close()


# ---------------------------------------------------------------- follow and step
FOLLOW_VOL = dict(nx=96, ny=64, nz=80, voxel=0.1, origin=[-4.8, -3.2, 0.3], mu=0.4, max_weight=128)
FOLLOW = dict(lookahead=4.3, threshold=2.0, granule=2)              # d = 0 at the identity; 3 degrees a frame are 2.25 voxels there


def test_follow_equals_the_restatement(built_lib, ppf):
    dev = ppf.Volume(**FOLLOW_VOL)
    ref = V.Volume(**FOLLOW_VOL)
    eye = np.eye(4, dtype=np.float32)
    assert dev.follow(eye, ppf.default_follow_params(dev, **FOLLOW)) == (0, 0, 0)
    d = ppf.default_follow_params(dev)
    w = H.follow_defaults(ref)
    assert (d.lookahead, d.threshold, d.granule) == (w["lookahead"], w["threshold"], w["granule"])
    at = eye.copy()
    at[1, 3] = F(16.0) * F(0.1)                                     # the default threshold of 16 voxels on y ...
    over = at.copy()
    over[1, 3] = np.nextafter(at[1, 3], F(9.0))
    turn = np.array([[0, 0, 1, 0.2], [0, 1, 0, -0.1], [-1, 0, 0, 0.4], [0, 0, 0, 1]], np.float32)
    far = eye.copy()
    far[:3, 3] = [100.0, -0.3, -50.0]
    poses = [eye, at, over, turn, far]
    # exactly at the threshold: 32 * 0.1f is 3.2f and 16 * 0.1f is exact, so centre_y = 0 and d_y = 16 without rounding
    assert dev.follow(at) == (0, 0, 0) and dev.follow(over) == (0, 16, 0)
    for shift in ((0, 0, 0), (8, -16, 4)):
        if any(shift):
            dev.shift(shift)
            ref = H.shifted(ref, shift)
        for T in poses:
            for kw in (dict(), FOLLOW, dict(lookahead=0.0, threshold=0.0, granule=1), dict(granule=64)):
                got = dev.follow(T, ppf.default_follow_params(dev, **kw) if kw else None)
                assert got == H.follow(ref, T, **kw), (shift, T[:3, 3], kw, got)
    assert same_window(dev, ref)                                    # follow moves nothing
    dev.close()


def test_step_with_follow(built_lib, ppf, synth, world):
    """Volume.step(view, follow=...) over five frames of the small stream of tests/volume_ref.py against a run without
    follow: the same poses up to the first shift; every shift moves the words as the restatement does, what left is in
    Volume.world, and the offsets are the follow rule applied to the device's own poses.  No tracking quality here.
    The volume, the follow parameters and the overlap gate are those of tests/shift_calib.py, whose restated loop moves
    the window at frames 2 and 4."""
    pts, traj = world
    cam = V.SMALL_CAM
    FOLLOW_VOL, FOLLOW = SC.VOLUME, SC.FOLLOW
    ep = ppf.default_egomotion_params(min_overlap=SC.MIN_OVERLAP)
    views = [TS.view_of(ppf, E.render(synth, pts, T, **V.SMALL), cam) for T in traj[:5]]
    plain = ppf.Volume(**FOLLOW_VOL)
    dev = ppf.Volume(**FOLLOW_VOL)
    fp = ppf.default_follow_params(dev, **FOLLOW)
    log = []
    shift, leaving = dev.shift, dev.leaving

    def spy_shift(s):
        ref = TS.restated(dev, FOLLOW_VOL)                          # the words and the window before the shift
        ref.origin0 = ref.origin.copy()
        ref.off, ref.origin = dev.window()
        res = shift(s)
        log.append(("shift", tuple(s), ref, res))
        return res

    def spy_leaving(s, min_weight=1):
        out = leaving(s, min_weight)
        log.append(("leaving", tuple(s), out))
        return out

    dev.shift, dev.leaving = spy_shift, spy_leaving
    state = V.Volume(**FOLLOW_VOL)                                  # the window alone: follow reads only its origin
    shifts, first = 0, None
    for f, v in enumerate(views):
        Tp, rp = plain.step(v, ep)
        n_log = len(log)
        T, r = dev.step(v, ep, follow=fp)
        if first is None:
            assert T.tobytes() == Tp.tobytes() and (r is None) == (rp is None), f
        new = log[n_log:]
        s = H.follow(state, T, **FOLLOW) if r is not None and r["ok"] else (0, 0, 0)
        print("frame %d: ok %s, shift %s, window %s" % (f, None if r is None else r["ok"], s, dev.window()[0]))
        if any(s):
            assert [e[0] for e in new] == ["leaving", "shift"] and new[0][1] == new[1][1] == s, (f, s, new)
            before, res = new[1][2], new[1][3]
            want = H.shifted(before, s)
            assert same_words(dev, want) and same_window(dev, want) and res["kept"] == H.kept(want)
            po, no, lres = new[0][2]
            wx, wn, wc = H.leaving(before, s)
            assert po.tobytes() == wx.tobytes() and no.tobytes() == wn.tobytes() and lres["crossings"] == wc
            assert dev.world[-1][0].tobytes() == po.tobytes() and dev.world[-1][1].tobytes() == no.tobytes()
            state = H.shifted(state, s)
            shifts += 1
            first = f if first is None else first
        else:
            assert not new, (f, new)
        assert dev.window()[0] == tuple(getattr(state, "off", (0, 0, 0))) and len(dev.world) == shifts
    assert shifts >= 1 and sum(len(p) for p, _ in dev.world) > 0 and plain.window()[0] == (0, 0, 0) and plain.world == []
    dev.reset()
    assert dev.world == [] and dev.window()[0] == (0, 0, 0)
    for v in views:
        v.close()
    plain.close()
    dev.close()
