"""GPU: the bilateral depth filter (k_bilateral, oslam_view_bilateral) against the numpy restatement of
tests/bilateral_ref.py bit for bit, its output as a genuine view (maps, egomotion, pyramid, integration), Volume.step's
smooth= wiring against the hand-written sequence, and the noisy stream of the calibration end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilateral_calib as BC  # noqa: E402
import bilateral_ref as B  # noqa: E402
import camera_ref as E  # noqa: E402
import pyramid_ref as P  # noqa: E402
import track_ref as K  # noqa: E402
import view_ref  # noqa: E402
import volume_ref as V  # noqa: E402
from test_bilateral_host import exact_gate_image  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
DYN = ("launches", "ms_total")
SIZES = [(1, 1), (2, 2), (5, 3), (33, 9), (65, 17), (333, 251)]             # (w, h); 33 x 9 is one past a tile both ways
RADII = (1, 6, 8)
SIGMAS = ((4.5, 0.03), (3.3, 0.017))
CAM = dict(fx=525.0, fy=520.0, cx=319.5, cy=239.25, depth_scale=1.0, z_min=0.5, z_max=6.0)
MAX_JUMP = 0.08
TINY = dict(width=160, height=120, fx=131.25, fy=131.25, cx=79.5, cy=59.5)
TINY_CAM = dict(E.CAM, fx=131.25, fy=131.25, cx=79.5, cy=59.5)
STEP_VOL = dict(nx=64, ny=64, nz=64, voxel=0.15, origin=[-2.9, -4.3, 0.3], mu=0.6, max_weight=2)    # the whole room
# voxels of 15 cm under pixels of 2 to 5 cm: the ray cast's normals pass the normal gate on 0.63 and 0.58 of the frame
# (tests/volume_ref.py on these frames), so the step's acceptance is asked at 0.5
STEP_MIN_OVERLAP = 0.5


def view_of(ppf, img, cam, max_jump=MAX_JUMP):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=max_jump)


def plain(d):
    return {k: v for k, v in d.items() if k not in DYN and k != "smooth"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_depth(w, h, cam, seed):
    """Seeded float depth in metres: a slanted surface with steps of 0.05 .. 0.13 m between blocks of 6 pixels, so that the
    3-sigma gate of sigma_depth 0.03 and of 0.017 falls on both sides, uniform noise of 2 cm, 8 % holes, pixels exactly at
    z_min and z_max, NaNs."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    z = 2.0 + 0.002 * u + 0.001 * v + rng.uniform(0.05, 0.13, (h // 6 + 1, w // 6 + 1)).cumsum(axis=1)[v // 6, u // 6]
    z = (z + rng.uniform(-0.02, 0.02, (h, w))).astype(np.float32)
    z[rng.uniform(size=(h, w)) < 0.08] = 0.0
    z[rng.uniform(size=(h, w)) < 0.02] = cam["z_min"]
    z[rng.uniform(size=(h, w)) < 0.02] = cam["z_max"]
    z[rng.uniform(size=(h, w)) < 0.01] = np.nan          # oslam_view_create turns these into holes
    return z


def assert_filter_equals(ppf, name, img, cam, **kw):
    """one call on a fresh view of img against the restatement: z bit for bit, valid, taps, launches -> the restated z"""
    want, valid, taps = B.bilateral_depth(img, cam, **kw)
    v = view_of(ppf, img, cam)
    f, r = ppf.bilateral_view(v, **kw)
    _, got = ppf.view_maps(f)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    print("%s %s: valid %d (restatement %d), taps %d (%d), %d pixels differ" % (name, kw, r["valid"], valid, r["taps"], taps,
                                                                            bad.size))
    assert got.shape == want.shape and bad.size == 0, (name, kw, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])
    assert (r["valid"], r["taps"], r["launches"]) == (valid, taps, 1), (name, kw, r, valid, taps)
    assert (f.width, f.height) == (v.width, v.height)
    f.close()
    v.close()
    return want


@pytest.mark.parametrize("w,h", SIZES)
def test_filter_equals_restatement(built_lib, ppf, w, h):
    c = dict(CAM, cx=0.5 * (w - 1), cy=0.5 * (h - 1) + 0.25)
    img = random_depth(w, h, c, 300 + w)
    for R in RADII:
        for ss, sd in SIGMAS:
            want = assert_filter_equals(ppf, "%dx%d" % (w, h), img, c, radius=R, sigma_space=ss, sigma_depth=sd)
    if w >= 65:
        z = view_ref.view_z(img, 1.0, c["z_min"], c["z_max"])
        assert (want != z).sum() > z.size // 2 and np.array_equal(want == 0, z == 0)


def test_hand_made_images_on_the_device(built_lib, ppf):
    z, kw = exact_gate_image()
    want = assert_filter_equals(ppf, "exact gate", z, CAM, **kw)
    assert int(bits(want)[4, 4]) == 0x4000FEE1
    hole = np.zeros((11, 37), np.float32)
    hole[3, 5] = np.nan
    v = view_of(ppf, hole, CAM)
    f, r = ppf.bilateral_view(v)
    assert (r["valid"], r["taps"], r["launches"]) == (0, 0, 1) and not ppf.view_maps(f)[1].any()
    f.close()
    v.close()
    assert_filter_equals(ppf, "constant", np.full((19, 40), 2.5, np.float32), CAM, radius=8)


def test_repeatable_and_refusals_leave_the_device_usable(built_lib, ppf):
    img = random_depth(65, 17, CAM, 9)
    want, valid, taps = B.bilateral_depth(img, CAM)
    v = view_of(ppf, img, CAM)
    outs = []
    for k in range(2):
        f, r = ppf.bilateral_view(v)
        outs.append((ppf.view_maps(f)[1].tobytes(), r["valid"], r["taps"]))
        f.close()
        for bad in (dict(radius=0), dict(radius=9), dict(sigma_space=0.0), dict(sigma_depth=float("nan")),
                    dict(sigma_depth=float("inf"))):
            with pytest.raises(ppf.OslamError) as e:
                ppf.bilateral_view(v, **bad)
            assert e.value.code == ppf.OSLAM_E_INVALID, bad
    assert outs[0] == outs[1] == (want.tobytes(), valid, taps)
    # params= replaces the keywords
    f, r = ppf.bilateral_view(v, params=ppf.default_bilateral_params(radius=2, sigma_depth=0.05))
    assert ppf.view_maps(f)[1].tobytes() == B.bilateral_depth(img, CAM, radius=2, sigma_depth=0.05)[0].tobytes()
    f.close()
    v.close()


@pytest.fixture(scope="module")
def tiny(synth):
    """Frames 0, 1, 2 of seed 0 of tests/test_camera_host.py at 160 x 120, with 3 mm of seeded depth noise."""
    world = E.make_world(synth, 0)
    traj = E.trajectory(synth, 0)
    rng = np.random.default_rng(3)
    return [BC.add_noise(E.render(synth, world, traj[f], **TINY), rng, 3.0) for f in range(3)]


def test_filtered_view_is_a_view(built_lib, ppf, tiny):
    cam1 = dict(TINY_CAM, depth_scale=1.0)
    raw = [view_of(ppf, im, TINY_CAM, E.MAX_JUMP) for im in tiny[:2]]
    zr = [B.bilateral_depth(im, TINY_CAM)[0] for im in tiny[:2]]
    filt = [ppf.bilateral_view(v)[0] for v in raw]
    twin = [view_of(ppf, z, cam1, E.MAX_JUMP) for z in zr]            # plain views of the restated z
    # the maps: built on first use from the filtered z with the input's camera and max_jump
    for k in range(2):
        maps, z = ppf.view_maps(filt[k])
        Vr, Nr, ok = K.view_maps(zr[k], cam1, E.MAX_JUMP)
        assert z.tobytes() == zr[k].tobytes()
        assert np.array_equal(maps[..., 3] != 0, ok) and ok.sum() > z.size // 2
        assert maps[..., :3].tobytes() == Vr.tobytes() and maps[..., 4:7].tobytes() == Nr.tobytes()
        cam, w, h = ppf.view_camera(filt[k])
        assert (w, h) == (160, 120) and cam.max_jump == F(E.MAX_JUMP) and cam.fx == F(TINY_CAM["fx"])
    # egomotion
    T, r = ppf.egomotion(filt[1], filt[0])
    Tw, rw = ppf.egomotion(twin[1], twin[0])
    print("egomotion on filtered views: %s" % plain(r))
    assert T.tobytes() == Tw.tobytes() and plain(r) == plain(rw) and r["correspondences"] > 1000
    # pyramid
    pyr = ppf.Pyramid(filt[0])
    want = P.pyramid(zr[0], cam1, E.MAX_JUMP)
    for k in range(3):
        assert ppf.view_maps(pyr.level(k))[1].tobytes() == want[k]["z"].tobytes(), k
    pyr.close()
    # integration
    eye = np.eye(4, dtype=np.float32)
    va, vb = ppf.Volume(**STEP_VOL), ppf.Volume(**STEP_VOL)
    ra, rb = va.integrate(filt[0], eye), vb.integrate(twin[0], eye)
    assert plain(ra) == plain(rb) and ra["updated"] > 0
    for x, y in zip(va.voxels(), vb.voxels()):
        assert np.array_equal(x, y)
    # a ray-cast view filters too, and its filtered copy takes its normals from z
    cast, _ = va.raycast(eye, TINY_CAM["fx"], TINY_CAM["fy"], TINY_CAM["cx"], TINY_CAM["cy"], 160, 120,
                         z_min=TINY_CAM["z_min"], z_max=TINY_CAM["z_max"], max_jump=E.MAX_JUMP)
    zc = ppf.view_maps(cast)[1]
    fc, rc = ppf.bilateral_view(cast)
    wc, valid, taps = B.bilateral(zc, TINY_CAM["z_min"], TINY_CAM["z_max"])
    maps, z = ppf.view_maps(fc)
    Vr, Nr, ok = K.view_maps(wc, cam1, E.MAX_JUMP)
    assert z.tobytes() == wc.tobytes() and (rc["valid"], rc["taps"]) == (valid, taps) and valid > 1000
    assert maps[..., :3].tobytes() == Vr.tobytes() and maps[..., 4:7].tobytes() == Nr.tobytes()
    for x in [fc, cast, va, vb] + filt + twin + raw:
        x.close()


def test_volume_step_smooth_equals_the_hand_written_sequence(built_lib, ppf, tiny):
    views = [view_of(ppf, im, TINY_CAM, E.MAX_JUMP) for im in tiny]
    p = ppf.default_bilateral_params(radius=4, sigma_depth=0.02)
    ep = ppf.default_egomotion_params(min_overlap=STEP_MIN_OVERLAP)
    a, b = ppf.Volume(**STEP_VOL), ppf.Volume(**STEP_VOL)
    Tb = np.eye(4, dtype=np.float32)
    for f, v in enumerate(views):
        T, r = a.step(v, ep, smooth=p)
        if f == 0:
            assert r is None and T.tobytes() == Tb.tobytes()
            want_int = b.integrate(v, Tb)                              # the first frame: raw, unfiltered
        else:
            filt, sres = ppf.bilateral_view(v, params=p)
            Tt, rt = b.track(filt, Tb, ep)
            filt.close()
            print("frame %d: %s, smooth %s" % (f, plain(r), {k: x for k, x in r["smooth"].items() if k not in DYN}))
            assert plain(r) == plain(rt) and T.tobytes() == (Tt if rt["ok"] else Tb).tobytes(), (f, r, rt)
            assert {k: x for k, x in r["smooth"].items() if k not in DYN} == {k: x for k, x in sres.items() if k not in DYN}
            assert r["smooth"]["launches"] == 1 and r["smooth"]["valid"] == int((tiny[f] > 0).sum())
            assert rt["ok"] == 1, (f, rt)
            Tb = Tt
            want_int = b.integrate(v, Tb)                              # integrated from the raw view
        assert plain(a.last_integrate) == plain(want_int), (f, a.last_integrate, want_int)
        for x, y in zip(a.voxels(), b.voxels()):
            assert np.array_equal(x, y), f
    # without smooth nothing changes: the plain step differs from the smoothed one only through the tracked view
    c = ppf.Volume(**STEP_VOL)
    c.step(views[0])
    T1, r1 = c.step(views[1])
    assert "smooth" not in r1
    for x in views + [a, b, c]:
        x.close()


def test_noisy_stream_end_to_end(built_lib, ppf):
    """The 6 mm rows of the calibration's motion table on the device: the raw pairs miss min_overlap, the filtered ones
    follow with a translation error below 5 mm."""
    traj, imgs = BC.noisy_frames(6.0)
    raw = [view_of(ppf, im, V.SMALL_CAM, E.MAX_JUMP) for im in imgs]
    filt = [ppf.bilateral_view(v)[0] for v in raw]
    for a, b in BC.MOTION_PAIRS:
        truth = E.truth(traj[a], traj[b])[:3, 3]
        Tr, rr = ppf.egomotion(raw[a], raw[b])
        Tf, rf = ppf.egomotion(filt[a], filt[b])
        err = float(np.linalg.norm(Tf[:3, 3].astype(np.float64) - truth))
        print("%d -> %d: raw overlap %.3f ok %d, filtered overlap %.3f ok %d, translation error %.1f mm"
              % (a, b, rr["overlap"], rr["ok"], rf["overlap"], rf["ok"], 1000 * err))
        assert not rr["ok"], rr
        assert rf["ok"] and err < 0.005, (rf, err)
    for x in filt + raw:
        x.close()
