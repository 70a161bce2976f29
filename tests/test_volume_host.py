"""CPU: the fusion stage's yardstick (tests/volume_ref.py) against the truth, its calibration, and the arguments
(include/oslam.h at oslam_volume_integrate, oslam_volume_raycast and oslam_volume_track).

The world and the motion are tests/test_camera_host.py's (camera_ref.make_world / trajectory: 3 degrees and 3 cm per
frame, 10 frames, seeds 0, 1, 2), rendered at 320 x 240, fused into a volume of 5 cm voxels around the room
(volume_ref.room_volume: 184 x 128 x 128 .. 144 voxels).

mu.  With the default mu of 4 voxels (0.20 m) a frame ray-cast back from its own pose hits 77 % of its valid pixels and
has a normal on 71 % of the pixels that had one: the floor and the side wall are seen at a grazing angle, the projective
band |z_o - p'z| <= mu is there only mu * cos thick across the surface (1.5 voxels on the floor at 4 m), voxels behind it
are never seen, and a trilinear read needs all 8 corners seen.  Frame-to-model tracking then stays below the default
min_overlap of 0.75 (0.65 at the first step).  With mu = 8 voxels (0.40 m, volume_ref.ROOM_MU) 88 % of the valid pixels
are hit and every step of the loop below is ok.  Measured with the restatement on the CPU:

  Fusion of the 10 frames at their true poses, ray cast from a true pose between frames 4 and 5, against the rendering
  of that pose on the pixels both have:
    seed   median |dz|   95th percentile   hits / valid pixels of the rendering
    0      0.0017 m      0.0086 m          0.878
    1      0.0015 m      0.0088 m          0.877
    2      0.0017 m      0.0091 m          0.863
  (mu = 4 voxels, seed 0: 0.0016 m, 0.0082 m, 0.771).  The frames are in millimetres, so the median is 1.5 depth steps.

  Frame-to-model loop over frames 0..9, 8..0 (18 steps, integrating every ok frame at its tracked pose) against the
  chained frame-to-frame camera_ref.egomotion over the same 18 steps, both against the truth of the last frame (frame 0):
    seed   frame to model        chained            overlap of the loop's steps   frame 9: model, chained
    0      0.0221 deg 0.0026 m   0.0074 deg 0.0008 m   0.758 .. 0.834             0.1925 deg 0.0147 m, 0.1797 deg 0.0136 m
    1      0.0174 deg 0.0026 m   0.0057 deg 0.0008 m   0.757 .. 0.848             0.1984 deg 0.0134 m, 0.1947 deg 0.0126 m
    2      0.0262 deg 0.0026 m   0.0155 deg 0.0010 m   0.757 .. 0.793             0.0912 deg 0.0150 m, 0.1142 deg 0.0139 m
  Finding: on these noise-free frames at 5 cm voxels fusion does NOT beat chaining.  Both drift by the same 0.02 degrees
  and 1.6 mm per frame on the way out (the rule's fixed point lies that far from the truth, tests/test_camera_host.py, and
  the frames are integrated at the drifted poses, so the model inherits the drift), both come back on the way in, and the
  model ends 2 .. 3 times further from the truth than the chain.  The bound asserted below is 1.5 times the worst seed:
  0.0393 degrees and 0.0041 m (volume_ref.MODEL_ROT_BOUND / MODEL_TRANS_BOUND).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import refine_ref  # noqa: E402
import volume_ref as V  # noqa: E402

SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def streams(synth):
    return {seed: V.small_stream(synth, seed) for seed in SEEDS}


def test_fused_surface_reaches_the_truth(synth, streams):
    for seed in SEEDS:
        s = streams[seed]
        vol = V.room_volume(seed)
        for f, T in enumerate(s["traj"]):
            n = vol.integrate(s["z"][f], V.SMALL_CAM, T.astype(np.float32))
            assert n > 0
        pose = V.between(synth, seed)
        assert all(np.abs(pose - T).max() > 1e-3 for T in s["traj"])
        z, maps, cnt = vol.raycast(pose.astype(np.float32), V.SMALL_CAM, V.SMALL["width"], V.SMALL["height"])
        zr = V.z_image(E.render(synth, s["world"], pose, **V.SMALL), V.SMALL_CAM)
        both = (z > 0) & (zr > 0)
        d = np.abs(z[both].astype(np.float64) - zr[both])
        med, p95, share = float(np.median(d)), float(np.percentile(d, 95)), both.sum() / (zr > 0).sum()
        print("seed %d: volume %s, median |dz| %.4f m, 95th percentile %.4f m, hits on %.3f of the valid pixels, %s"
              % (seed, vol.n, med, p95, share, cnt))
        assert med <= V.ROOM_VOXEL, (seed, med)
        assert share >= 0.5, (seed, share)
        assert cnt["hits"] == int((z > 0).sum()) and cnt["normals"] == int(maps[2].sum()) <= cnt["hits"]
        # a normal faces the camera and is a unit vector
        Vx, N, has = maps
        assert np.all((N[has] * Vx[has]).sum(axis=1) < 0) and np.allclose(np.linalg.norm(N[has], axis=1), 1.0, atol=1e-5)
        assert not N[~has].any() and not Vx[~has].any()


def test_frame_to_model_tracking_there_and_back(streams):
    worst = [0.0, 0.0]
    for seed in SEEDS:
        s = streams[seed]
        out = V.there_and_back(V.room_volume(seed), s)
        chain, prev = np.eye(4), 0
        for f, T, r in out[1:]:
            assert r["ok"] == 1, (seed, f, r)
            Tc, _ = E.egomotion(s["maps"][prev], s["maps"][f], V.SMALL_CAM)
            chain = chain @ np.linalg.inv(Tc.astype(np.float64))
            prev = f
            rot, tr = refine_ref.pose_error(T, s["traj"][f])
            crot, ctr = refine_ref.pose_error(chain, s["traj"][f])
            print("seed %d frame %d: frame to model %.4f deg %.4f m, chained %.4f deg %.4f m, overlap %.3f, iterations %s"
                  % (seed, f, rot, tr, crot, ctr, r["overlap"], r["iterations"]))
        assert tr < E.default_params()["max_corr_dist"], (seed, tr)            # nearer than the distance gate
        assert rot <= V.MODEL_ROT_BOUND and tr <= V.MODEL_TRANS_BOUND, (seed, rot, tr)
        worst = [max(worst[0], rot), max(worst[1], tr)]
        print("seed %d end pose: frame to model %.4f deg %.4f m, chained %.4f deg %.4f m" % (seed, rot, tr, crot, ctr))
    print("worst end pose of the frame-to-model loop: %.4f deg %.4f m" % tuple(worst))


def test_integer_properties_of_the_restatement():
    cam = dict(fx=60.0, fy=60.0, cx=31.5, cy=23.5, depth_scale=1.0, z_min=0.1, z_max=10.0)
    z = np.full((48, 64), 1.0, np.float32)
    z[:, 40:] = 0.0                                              # not valid: those voxels are never seen
    vol = V.Volume(32, 24, 32, 0.05, [-0.8, -0.6, 0.2], max_weight=3)
    eye = np.eye(4, dtype=np.float32)
    n1 = vol.integrate(z, cam, eye)
    q1, w1 = vol.q.copy(), vol.w.copy()
    assert n1 == int((w1 == 1).sum()) > 0 and set(np.unique(w1)) == {0, 1}
    zc = vol.origin[2] + (np.arange(32, dtype=np.float32) + np.float32(0.5)) * vol.voxel
    assert not w1[zc > np.float32(1.0) + vol.mu].any()            # behind the surface by more than mu: w stays 0
    assert w1[zc < np.float32(1.0)].any() and (q1[zc < np.float32(1.0) - vol.mu][w1[zc < np.float32(1.0) - vol.mu] > 0] == 32767).all()
    # the same frame again: f repeats, so F' = (F w + f) / (w + 1) = F up to one rounding of the quotient
    vol.integrate(z, cam, eye)
    assert np.array_equal(vol.w, 2 * w1) and np.abs(vol.q.astype(np.int32) - q1).max() <= 1
    assert np.array_equal(vol.q[np.abs(q1) == 32767], q1[np.abs(q1) == 32767])
    for _ in range(4):
        vol.integrate(z, cam, eye)
    assert set(np.unique(vol.w)) == {0, 3}                        # weights saturate at max_weight
    vol.reset()
    assert not vol.q.any() and not vol.w.any()
    # two runs from a reset volume give equal bits
    vol.integrate(z, cam, eye)
    assert np.array_equal(vol.q, q1) and np.array_equal(vol.w, w1)
    # the pose arithmetic: the inverse of the inverse and the product with the inverse
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = refine_ref.rodrigues(np.array([0.2, -0.4, 0.1]))[0]
    T[:3, 3] = [0.3, -1.0, 2.0]
    assert np.abs(V.compose(T, V.invert_pose(T)) - np.eye(4)).max() < 1e-6
    assert V.compose(eye, T).tobytes() == T.tobytes()


# ---------------------------------------------------------------- ABI
def test_volume_defaults(built_lib, ppf):
    p = ppf.default_volume_params()
    assert (p.nx, p.ny, p.nz) == (256, 256, 256) and p.voxel == np.float32(0.02) and p.max_weight == 128
    assert p.mu == np.float32(4.0) * np.float32(0.02) and list(p.reserved) == [0, 0, 0, 0]
    assert list(p.origin) == [np.float32(-2.56), np.float32(-2.56), 0.0]
    assert C.sizeof(ppf.VolumeParams) == 52
    with pytest.raises(TypeError):
        ppf.default_volume_params(no_such_field=1)


def test_volume_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Every OSLAM_E_INVALID case of the fusion stage with stand-in handles (zeroed host memory: device 0), on a machine
    with or without a GPU."""
    L = ppf.lib()
    fa, fb = C.create_string_buffer(4096), C.create_string_buffer(4096)
    vol, view = C.cast(fa, C.c_void_p), C.cast(fb, C.c_void_p)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    To = np.zeros(16, np.float32)
    h = C.c_void_p(0)
    INV = ppf.OSLAM_E_INVALID
    nan, inf = float("nan"), float("inf")

    assert L.oslam_volume_params_default(None) == INV
    assert L.oslam_volume_create(None, 0, C.byref(h)) == INV
    assert L.oslam_volume_create(C.byref(ppf.default_volume_params()), 0, None) == INV
    bad_p = [dict(nx=8), dict(ny=520), dict(nz=100), dict(nx=0), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan),
             dict(voxel=inf), dict(origin=[nan, 0, 0]), dict(origin=[0, inf, 0]), dict(origin=[0, 0, -inf]), dict(mu=nan),
             dict(mu=inf), dict(mu=0.03), dict(mu=-1.0), dict(max_weight=0), dict(max_weight=65536), dict(voxel=1e-42, mu=1.0)]
    for kw in bad_p:
        assert L.oslam_volume_create(C.byref(ppf.default_volume_params(**kw)), 0, C.byref(h)) == INV, kw
        assert not h.value
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_volume_create(C.byref(ppf.default_volume_params(mu=0.03)), 0, C.byref(h)))
    assert e.value.code == INV and "mu" in str(e.value)
    assert L.oslam_volume_destroy(None) == L.oslam_volume_reset(None) == INV

    bad_T = []
    T = eye.copy(); T[3] = np.nan; bad_T.append(T)
    T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad_T.append(T)
    T = eye.copy(); T[0] = -1; bad_T.append(T)
    T = eye.copy(); T[13] = 0.5; bad_T.append(T)

    def integrate(vo=vol, vi=view, T=eye):
        return L.oslam_volume_integrate(vo, vi, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None, None)

    def raycast(vo=vol, T=eye, cam=None, w=64, hh=48, out=C.byref(h), **kw):
        c = dict(fx=60.0, fy=60.0, cx=31.5, cy=23.5, depth_scale=1.0, z_min=0.5, z_max=8.0, max_jump=0.05)
        c.update(kw)
        cam_ = C.byref(ppf.Camera(**c)) if cam is None else cam
        return L.oslam_volume_raycast(vo, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None,
                                      None if cam == "null" else cam_, w, hh, out, None)

    def track(vo=vol, vi=view, T=eye, params=None, out=To):
        p = params if params is not None else ppf.default_egomotion_params()
        return L.oslam_volume_track(vo, vi, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None,
                                    C.byref(p), ppf._p(out) if out is not None else None, None)

    assert integrate(vo=None) == integrate(vi=None) == integrate(T=None) == INV
    assert raycast(vo=None) == raycast(T=None) == raycast(cam="null") == raycast(out=None) == INV
    assert track(vo=None) == track(vi=None) == track(T=None) == track(out=None) == INV
    for T in bad_T:
        assert integrate(T=T) == raycast(T=T) == track(T=T) == INV, T
    for kw in (dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(cx=inf), dict(cy=nan), dict(z_min=0.0), dict(z_min=2.0, z_max=1.0),
               dict(z_max=inf), dict(max_jump=-1.0), dict(max_jump=nan), dict(w=0), dict(hh=0), dict(w=16385), dict(hh=-3)):
        assert raycast(**kw) == INV, kw
        assert not h.value
    for kw in (dict(max_corr_dist=0.0), dict(min_overlap=1.5), dict(levels=[(17, 1)]), dict(levels=[]), dict(stop_rot=nan)):
        assert track(params=ppf.default_egomotion_params(**kw)) == INV, kw
    # a volume and a view on different devices: the stand-in view says device 1
    C.cast(fb, C.POINTER(C.c_int))[0] = 1
    assert integrate() == INV and "different devices" in L.oslam_last_error().decode()
    assert track() == INV and "different devices" in L.oslam_last_error().decode()
    C.cast(fb, C.POINTER(C.c_int))[0] = 0
    # the taps and the cloud of a view
    n = C.c_size_t(0)
    buf = np.zeros(64, np.float32)
    assert L.oslam_view_to_cloud(None, ppf._p(buf), ppf._p(buf), 4, C.byref(n)) == INV
    assert L.oslam_view_to_cloud(view, None, ppf._p(buf), 4, C.byref(n)) == INV
    assert L.oslam_view_to_cloud(view, ppf._p(buf), None, 4, C.byref(n)) == INV
    assert L.oslam_view_to_cloud(view, ppf._p(buf), ppf._p(buf), 4, None) == INV
    assert L.oslam_volume_voxels(None, ppf._p(buf), ppf._p(buf)) == L.oslam_volume_voxels(vol, None, ppf._p(buf)) == INV
    assert L.oslam_volume_voxels(vol, ppf._p(buf), None) == INV
    assert L.oslam_view_maps(None, ppf._p(buf), None) == L.oslam_view_maps(view, None, None) == INV
