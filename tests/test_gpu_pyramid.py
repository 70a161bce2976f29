"""GPU: the image pyramid (k_pyr_down, oslam_pyramid_create / _level), coarse-to-fine camera motion over two pyramids
(oslam_pyramid_egomotion) and frame-to-model tracking over them (oslam_volume_track_pyramid) against the numpy
restatement of tests/pyramid_ref.py and against the public single-level calls, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import edge_inputs  # noqa: E402
import pyramid_ref as P  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402
import volume_ref as V  # noqa: E402
from test_pyramid_host import CAM as HAND_CAM, hand_made_cases  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
DYN = ("launches", "ms_total")
SIZES = [(1, 1), (2, 2), (5, 3), (65, 17), (333, 251), (640, 480)]          # (w, h)
TRACK_VOL = dict(nx=64, ny=64, nz=64, voxel=0.1, origin=[-3.2, -4.4, 1.5], mu=0.4, max_weight=2)


def view_of(ppf, img, cam, max_jump):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=max_jump)


def plain(d):
    return {k: v for k, v in d.items() if k not in DYN}


def random_depth(w, h, cam, seed):
    """Seeded float depth in metres: a slanted surface with steps of about the band (0.05 .. 0.13 m) between blocks,
    uniform noise of 2 cm, holes, and pixels exactly at z_min and z_max."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    z = 2.0 + 0.002 * u + 0.001 * v + rng.uniform(0.05, 0.13, (h // 6 + 1, w // 6 + 1)).cumsum(axis=1)[v // 6, u // 6] * 0.5
    z = (z + rng.uniform(-0.02, 0.02, (h, w))).astype(np.float32)
    z[rng.uniform(size=(h, w)) < 0.08] = 0.0
    z[rng.uniform(size=(h, w)) < 0.02] = cam["z_min"]
    z[rng.uniform(size=(h, w)) < 0.02] = cam["z_max"]
    z[rng.uniform(size=(h, w)) < 0.01] = np.nan          # oslam_view_create turns these into holes
    return z


def device_levels(ppf, pyr):
    """-> [(maps [h,w,8], z [h,w])] of every level of a device pyramid"""
    return [ppf.view_maps(pyr.level(k)) for k in range(pyr.levels)]


def assert_level_equals(name, k, got, want):
    """got: (maps, z) of the device; want: a level of pyramid_ref.pyramid.  z bit for bit, and the maps against
    track_ref.view_maps of the restated z with the restated camera and max_jump: the check that the level's camera and
    max_jump are the rule's, since every vertex and normal depends on them."""
    maps, z = got
    assert z.shape == want["z"].shape, (name, k, z.shape, want["z"].shape)
    bad = np.flatnonzero(z.view(np.uint32).ravel() != want["z"].view(np.uint32).ravel())
    assert bad.size == 0, (name, k, bad[:8], z.ravel()[bad[:8]], want["z"].ravel()[bad[:8]])
    Vr, Nr, ok = P.level_maps(want)
    assert np.array_equal(maps[..., 3] != 0, ok), (name, k)
    assert maps[..., :3].tobytes() == Vr.tobytes() and maps[..., 4:7].tobytes() == Nr.tobytes(), (name, k)


def test_pyr_down_equals_restatement_at_every_size(built_lib, ppf):
    cam = dict(fx=525.0, fy=520.0, cx=319.5, cy=239.25, depth_scale=1.0, z_min=0.5, z_max=6.0)
    for w, h in SIZES:
        c = dict(cam, cx=0.5 * (w - 1), cy=0.5 * (h - 1) + 0.25)
        img = random_depth(w, h, c, 100 + w)
        want = P.pyramid(img, c, 0.08, levels=3)
        v = view_of(ppf, img, c, 0.08)
        pyr = ppf.Pyramid(v)
        assert pyr.levels == 3
        got = device_levels(ppf, pyr)
        valid = [int((z > 0).sum()) for _, z in got]
        print("%dx%d: levels %s, valid pixels %s" % (w, h, [z.shape[::-1] for _, z in got], valid))
        for k in range(3):
            assert_level_equals("%dx%d" % (w, h), k, got[k], want[k])
        if w >= 65:
            assert valid[2] > 0
        # another band and two levels; the base is the caller's view itself
        p2 = ppf.Pyramid(v, levels=2, depth_band=0.03)
        w2 = P.pyramid(img, c, 0.08, levels=2, depth_band=0.03)
        assert_level_equals("%dx%d band 0.03" % (w, h), 1, ppf.view_maps(p2.level(1)), w2[1])
        assert p2.level(0)._h.value == v._h.value
        with pytest.raises(ppf.OslamError):
            p2.level(2)
        p2.close()
        pyr.close()
        v.close()


def test_hand_made_cases_on_the_device(built_lib, ppf):
    for name, (z, band, want) in hand_made_cases().items():
        v = view_of(ppf, z, HAND_CAM, 0.05)
        pyr = ppf.Pyramid(v, levels=2, depth_band=float(band))
        _, got = ppf.view_maps(pyr.level(1))
        assert got.tobytes() == want.tobytes(), (name, got, want)
        pyr.close()
        v.close()


def test_a_level_outlives_its_pyramid_object(built_lib, ppf):
    """level(k) keeps the pyramid and the base alive: dropping every other reference must not free what it reads."""
    z = np.full((9, 12), 2.5, np.float32)
    lv = ppf.Pyramid(view_of(ppf, z, HAND_CAM, 0.05)).level(1)
    _, got = ppf.view_maps(lv)
    assert np.array_equal(got, np.full((5, 6), 2.5, np.float32)) and (lv.width, lv.height) == (6, 5)
    lv.close()                                            # closing a borrowed view gives nothing back
    assert not lv._h


@pytest.fixture(scope="module")
def pairs(ppf, synth):
    """Frames 0, 1, 4, 5 of seed 0 of tests/test_camera_host.py at 640x480 and at the ragged 333x251: the images and the
    restated pyramids with their maps."""
    world = E.make_world(synth, 0)
    traj = E.trajectory(synth, 0)
    out = {}
    for name, size, cam in (("640x480", {}, E.CAM), ("333x251", edge_inputs.RAGGED, edge_inputs.ragged_cam())):
        imgs = {f: E.render(synth, world, traj[f], **size) for f in (0, 1, 4, 5)}
        out[name] = dict(cam=cam, imgs=imgs, ref={f: P.with_maps(P.pyramid(im, cam, E.MAX_JUMP)) for f, im in imgs.items()})
    return out


def test_coarse_levels_of_the_stream_are_views(built_lib, ppf, pairs):
    for name, c in pairs.items():
        v = view_of(ppf, c["imgs"][1], c["cam"], E.MAX_JUMP)
        pyr = ppf.Pyramid(v)
        for k in (1, 2):
            got = ppf.view_maps(pyr.level(k))
            assert_level_equals(name, k, got, c["ref"][1][k])
            print("%s level %d: %d of %d pixels have a normal" % (name, k, int((got[0][..., 3] != 0).sum()), got[1].size))
            assert (got[0][..., 3] != 0).sum() > got[1].size // 2
        pyr.close()
        v.close()


def test_pyramid_egomotion_equals_chain_and_restatement(built_lib, ppf, pairs):
    sched = E.default_params()["levels"]
    for name, c in pairs.items():
        for f in (1, 5):
            va, vb = view_of(ppf, c["imgs"][f - 1], c["cam"], E.MAX_JUMP), view_of(ppf, c["imgs"][f], c["cam"], E.MAX_JUMP)
            pa, pb = ppf.Pyramid(va), ppf.Pyramid(vb)
            T, r = ppf.egomotion_pyramid(pa, pb)
            # cost: the scheduled iterations plus the maps of the six level views, which a second call does not build
            assert r["launches"] == 19 + 6, r
            T2, r2 = ppf.egomotion_pyramid(pa, pb)
            assert r2["launches"] == 19 and T2.tobytes() == T.tobytes() and plain(r2) == plain(r)
            # the chain of single-level calls on the levels' views
            Tc, its, last = None, [], None
            for stride, n in sched:
                k = {4: 2, 2: 1, 1: 0}[stride]
                Tc, last = ppf.egomotion(pa.level(k), pb.level(k), Tc, ppf.default_egomotion_params(levels=[(1, n)]))
                its.append(last["iterations"][0])
            assert T.tobytes() == Tc.tobytes(), (name, f, refine_ref.pose_error(T, Tc))
            assert r["iterations"] == its and r["correspondences"] == last["correspondences"], (name, f, r, its, last)
            assert (r["rmse"], r["overlap"], r["converged"], r["ok"]) == \
                (last["rmse"], last["overlap"], last["converged"], last["ok"]), (name, f, r, last)
            # the restatement in the pinned float32 order
            W, w = P.egomotion_pyramid(c["ref"][f - 1], c["ref"][f], sums="f32")
            ang, dt = refine_ref.pose_error(T, W)
            print("%s frame %d: iterations %s, correspondences %d, overlap %.3f; device vs restatement (f32 order) %.3e deg "
                  "%.3e m, equal bits: %s" % (name, f, r["iterations"], r["correspondences"], r["overlap"], ang, dt,
                                              T.tobytes() == W.tobytes()))
            assert r["iterations"] == w["iterations"] and r["correspondences"] == w["correspondences"], (name, f, r, w)
            assert T.tobytes() == W.tobytes(), (name, f, ang, dt)
            if f == 1:
                # a schedule that names a level the pyramid lacks is refused
                q = ppf.Pyramid(vb, levels=2)
                with pytest.raises(ppf.OslamError) as e:
                    ppf.egomotion_pyramid(pa, q)
                assert e.value.code == ppf.OSLAM_E_INVALID
                assert ppf.egomotion_pyramid(pa, q, levels=[(2, 2), (1, 2)])[1]["iterations"][0] > 0
                q.close()
                # {1, 10} on one-level pyramids is oslam_view_egomotion with {1, 10}
                oa, ob = ppf.Pyramid(va, levels=1), ppf.Pyramid(vb, levels=1)
                T1, r1 = ppf.egomotion_pyramid(oa, ob, levels=[(1, 10)])
                T0, r0 = ppf.egomotion(va, vb, None, ppf.default_egomotion_params(levels=[(1, 10)]))
                assert T1.tobytes() == T0.tobytes() and plain(r1) == plain(r0) and r1["launches"] == 10
                # the same handle twice: the identity at once
                Ts, rs = ppf.egomotion_pyramid(oa, oa)
                assert np.array_equal(Ts, np.eye(4, dtype=np.float32)) and rs["launches"] == 0 and rs["ok"] == 1
                oa.close()
                ob.close()
            for x in (pa, pb, va, vb):
                x.close()


def test_volume_track_pyramid_equals_its_parts(built_lib, ppf, pairs):
    c = pairs["333x251"]
    cam = c["cam"]
    vol = ppf.Volume(**TRACK_VOL)
    views = {f: view_of(ppf, c["imgs"][f], cam, E.MAX_JUMP) for f in (0, 1)}
    eye = np.eye(4, dtype=np.float32)
    vol.integrate(views[0], eye)
    vol.integrate(views[0], eye)
    frame = ppf.Pyramid(views[1])
    for k in range(3):
        ppf.view_maps(frame.level(k))                     # the frame's maps exist before the calls that are compared
    for levels, band, sched in ((3, 0.09, None), (2, 0.05, [(2, 3), (1, 4)])):
        p = ppf.default_egomotion_params() if sched is None else ppf.default_egomotion_params(levels=sched)
        T, r = vol.track_pyramid(frame, eye, p, levels=levels, depth_band=band)
        # by hand through the public calls: ray cast, pyramid, pyramid egomotion, the pose product
        model, _ = vol.raycast(eye, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 333, 251, z_min=cam["z_min"],
                               z_max=cam["z_max"], max_jump=E.MAX_JUMP)
        mp = ppf.Pyramid(model, levels=levels, depth_band=band)
        Te, re_ = ppf.egomotion_pyramid(frame, mp, None, p)
        print("levels %d band %.2f: %s" % (levels, band, plain(r)))
        assert T.tobytes() == V.compose(eye, Te).tobytes()
        assert plain(r) == plain(re_), (r, re_)
        # the ray cast and the down-sampling launches are counted; the frame's maps exist by now in both calls, the
        # model's coarse levels build theirs in both
        assert r["launches"] == re_["launches"] + 1 + (levels - 1), (r, re_)
        assert r["correspondences"] > 1000 and sum(r["iterations"]) > 0
        mp.close()
        model.close()
    # from a pose that is not the identity the product is formed in double and rounded once
    Tp = np.eye(4, dtype=np.float32)
    Tp[:3, :3] = K.axis_rotation((0.1, 1.0, 0.05), 1.0).astype(np.float32)
    Tp[:3, 3] = [0.01, -0.02, 0.015]
    T, r = vol.track_pyramid(frame, Tp)
    model, _ = vol.raycast(Tp, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 333, 251, z_min=cam["z_min"], z_max=cam["z_max"],
                           max_jump=E.MAX_JUMP)
    mp = ppf.Pyramid(model)
    Te, re_ = ppf.egomotion_pyramid(frame, mp)
    assert T.tobytes() == V.compose(Tp, Te).tobytes() and plain(r) == plain(re_)
    mp.close()
    model.close()
    frame.close()
    for v in views.values():
        v.close()
    vol.close()
