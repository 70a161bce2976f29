"""CPU: the image pyramid's rule on hand-made images, its defaults and argument checks through the C-ABI, the split
property of the restated pyramid egomotion and the calibration of coarse-to-fine tracking against the single-image
egomotion (include/oslam.h at oslam_pyramid_create; restatement: tests/pyramid_ref.py).

Calibration.  The room of tests/test_camera_host.py (camera_ref.make_world), seeds 0, 1, 2, rendered at 640x480 from
camera_ref.trajectory at m x (3 degrees, 3 cm) per frame for m = 1, 2, 3, frames 0, 1, 2 of each stream (two pairs, src =
frame f - 1, dst = frame f, from the identity).  Four variants: the single-image egomotion ("parent", the default
schedule as strides over one pair) and the pyramid egomotion (the same schedule as pyramid levels 2, 1, 0), each with
max_corr_dist 0.30 m (the default) and 0.10 m (KinFu's).  "Followed": the criterion of
test_restatement_follows_the_moving_camera on every pair of the stream (camera_ref.ROT_BOUND, TRANS_BOUND, the chained
bounds, ok and overlap >= OVERLAP_CONSECUTIVE_MIN).  Measured with the restatement (float64 sums); per stream the pair
with the largest translation error, rotation error in degrees / translation error in metres / smallest overlap of the
stream, F = followed:

    m  seed   parent 0.30              pyramid 0.30             parent 0.10              pyramid 0.10
    1  0      0.0101 0.0008 0.927 F    0.0100 0.0008 0.927 F    0.0084 0.2626 0.752 -    0.0090 0.2917 0.793 -
    1  1      0.0105 0.0007 0.929 F    0.0105 0.0007 0.929 F    0.0105 0.0007 0.929 F    0.0105 0.0007 0.929 F
    1  2      0.0070 0.0008 0.920 F    0.0070 0.0008 0.920 F    0.0138 0.0010 0.761 -    0.0056 0.2597 0.635 -
    2  0      0.0205 0.4200 0.734 -    0.0204 0.4158 0.822 -    0.0197 0.4881 0.735 -    0.0191 0.0018 0.868 F
    2  1      0.0211 0.0020 0.877 F    0.0207 0.0016 0.878 F    0.0221 0.4660 0.744 -    0.0206 0.3736 0.744 -
    2  2      0.0178 0.4145 0.540 -    0.0190 0.4734 0.538 -    0.0208 0.5138 0.536 -    0.0215 0.5379 0.535 -
    3  0      0.0311 0.4442 0.717 -    0.0308 0.4234 0.717 -    0.0310 0.7299 0.710 -    0.0310 0.6639 0.554 -
    3  1      0.0314 0.8729 0.721 -    0.0287 0.8529 0.717 -    0.0322 0.8335 0.725 -    0.0292 0.7668 0.722 -
    3  2      0.0339 0.8856 0.446 -    0.0338 0.9456 0.444 -    0.0339 0.8267 0.448 -    0.0296 0.8663 0.449 -

    largest m followed on all seeds: parent 0.30: 1, pyramid 0.30: 1, parent 0.10: 0, pyramid 0.10: 0

A finding, not a success: on this room the pyramid does NOT widen the basin reliably.  At m = 1 and the default gate both
variants end within 0.0001 degrees and 0.1 mm of each other (the same full-resolution fixed point).  The pyramid rescues
single streams (m = 2, seed 0 with the 0.10 m gate: 0.0018 m where the single pair slides by 0.49 m) and loses others
(m = 1, seed 2 with the 0.10 m gate: 0.26 m where the single pair reaches 0.0010 m and misses only the overlap bound);
KinFu's 0.10 m gate still does not follow the stream at m = 1 on all seeds, with or without the pyramid; beyond m = 1
neither variant follows all three seeds.  Every failure is a translation of 0.26 .. 0.95 m with the rotation right to
0.034 degrees, the slide tests/test_camera_host.py describes; halving the images does not remove it while the gates stay
the same in metres at every level (per-level gates are out of scope here; why is not analysed further).  The defaults
of oslam_egomotion_params stay as they are.  Asserted: (1) at m = 1 and the default gate the pyramid's error on every
pair is within twice the parent's on the same pair; (2) for each gate the largest m the pyramid follows on all seeds
is not below the parent's.  The rest of the table is printed.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import pyramid_ref as P  # noqa: E402
import refine_ref  # noqa: E402

F = np.float32
CAM = dict(fx=100.0, fy=101.0, cx=31.5, cy=23.25, depth_scale=1.0, z_min=0.5, z_max=8.0)
SEEDS = (0, 1, 2)
MULTIPLES = (1, 2, 3)
GATES = (0.30, 0.10)
FRAMES = 3


def hand_made_cases():
    """name -> (z float32 [h, w], depth_band, expected z' or None): the rule's cases on hand-made images, shared with
    tests/test_gpu_pyramid.py."""
    band = F(P.DEPTH_BAND)
    out = {}
    out["constant"] = (np.full((9, 12), 2.5, np.float32), band, np.full((5, 6), 2.5, np.float32))
    step = np.full((8, 10), 1.0, np.float32)
    step[:, 5:] = 3.0                                   # a step of 2 m at u = 5: no output mixes the two sides
    want = np.full((4, 5), 1.0, np.float32)
    want[:, 3:] = 3.0                                   # centres 2u = 6, 8 lie on the far side
    out["step edge"] = (step, band, want)
    hole = np.full((5, 5), 2.0, np.float32)
    hole[2, 2] = 0.0
    want = np.full((3, 3), 2.0, np.float32)
    want[1, 1] = 0.0
    out["invalid centre"] = (hole, band, want)
    alone = np.zeros((5, 5), np.float32)
    alone[2, 2] = 1.75
    alone[0, 0], alone[4, 4], alone[2, 4] = 1.75 + 1.0, 1.75 - 1.0, 0.0          # out of band, and an invalid one
    want = np.zeros((3, 3), np.float32)
    want[1, 1] = 1.75
    want[0, 0], want[2, 2] = 2.75, 0.75
    out["lonely centre"] = (alone, band, want)
    # |z - c| == depth_band exactly is included, the next float above it is not: c = 2, band = 0.25, both exact in float
    c, b = F(2.0), F(0.25)
    edge = np.zeros((1, 3), np.float32)
    edge[0, 0], edge[0, 1] = c, c + b                                            # output (0, 0): centre c, neighbour in
    out["band edge in"] = (edge, b, np.array([[(c + (c + b)) / F(2.0), 0.0]], np.float32))
    edge = np.zeros((1, 3), np.float32)
    edge[0, 0], edge[0, 1] = c, np.nextafter(c + b, F(np.inf))
    assert np.abs(edge[0, 1] - c) > b
    out["band edge out"] = (edge, b, np.array([[c, 0.0]], np.float32))
    # clamping: the mean of values inside [z_min, z_max] stays there; the ends themselves survive
    ends = np.full((3, 3), CAM["z_min"], np.float32)
    out["at z_min"] = (ends, band, np.full((2, 2), CAM["z_min"], np.float32))
    out["at z_max"] = (np.full((3, 3), CAM["z_max"], np.float32), band, np.full((2, 2), CAM["z_max"], np.float32))
    return out


def test_rule_on_hand_made_images():
    for name, (z, band, want) in hand_made_cases().items():
        got, cam2, mj2 = P.pyr_down(z, CAM, 0.05, band)
        assert got.dtype == np.float32 and got.shape == want.shape, name
        assert got.tobytes() == want.tobytes(), (name, got, want)


def test_sizes_and_cameras_halve_exactly():
    rng = np.random.default_rng(3)
    for (w, h), (wo, ho) in (((1, 1), (1, 1)), ((2, 2), (1, 1)), ((5, 3), (3, 2)), ((7, 4), (4, 2)), ((640, 480), (320, 240)),
                             ((333, 251), (167, 126))):
        z = rng.uniform(1.0, 2.0, (h, w)).astype(np.float32)
        got, cam2, mj2 = P.pyr_down(z, CAM, 0.05)
        assert got.shape == (ho, wo), (w, h)
        assert (got > 0).all()
    _, cam2, mj2 = P.pyr_down(np.ones((4, 4), np.float32), CAM, 0.08)
    for k in ("fx", "fy", "cx", "cy"):
        assert F(cam2[k]) * F(2.0) == F(CAM[k]) and F(cam2[k]) == F(F(CAM[k]) / F(2.0)), k
    assert cam2["z_min"] == CAM["z_min"] and cam2["z_max"] == CAM["z_max"] and cam2["depth_scale"] == CAM["depth_scale"]
    assert F(mj2) == F(0.08) * F(2.0)
    pyr = P.pyramid(np.ones((7, 5), np.float32), CAM, 0.08, levels=3)
    assert [lv["z"].shape for lv in pyr] == [(7, 5), (4, 3), (2, 2)]
    assert F(pyr[2]["cam"]["cx"]) == F(CAM["cx"]) * F(0.25) and F(pyr[2]["max_jump"]) == F(0.08) * F(4.0)


def test_addition_order_is_row_major():
    """A window whose float sum depends on the order: the restatement adds dy outer, dx inner."""
    z = np.zeros((5, 5), np.float32)
    vals = (F(2.0) + np.arange(25, dtype=np.float32) * F(3e-7) * np.arange(25, dtype=np.float32)).astype(np.float32)
    z[:] = vals.reshape(5, 5)
    got, _, _ = P.pyr_down(z, CAM, 0.05)
    s = F(0)
    for v in z.reshape(-1):
        s = F(s + v)
    assert got[1, 1] == F(s / F(25.0))


# ---------------------------------------------------------------- ABI
def test_pyramid_defaults(built_lib, ppf):
    p = ppf.default_pyramid_params()
    assert p.n_levels == 3 and p.depth_band == np.float32(P.DEPTH_BAND) == np.float32(0.09) and list(p.reserved) == [0, 0, 0, 0]
    assert C.sizeof(ppf.PyramidParams) == 24
    q = ppf.default_pyramid_params(n_levels=2, depth_band=0.05)
    assert q.n_levels == 2 and q.depth_band == np.float32(0.05)
    with pytest.raises(TypeError):
        ppf.default_pyramid_params(no_such_field=1)
    assert ppf.lib().oslam_pyramid_params_default(None) == ppf.OSLAM_E_INVALID
    e = ppf.default_egomotion_params()                   # the egomotion defaults did not move
    assert [(l.stride, l.max_iterations) for l in e.level] == [(4, 4), (2, 5), (1, 10)] and e.max_corr_dist == np.float32(0.30)


def test_pyramid_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Every OSLAM_E_INVALID case of the pyramid's entry points with stand-in handles (zeroed host memory: device 0, no
    levels) on a machine with or without a GPU."""
    L = ppf.lib()
    fa, fb, fv = C.create_string_buffer(4096), C.create_string_buffer(4096), C.create_string_buffer(4096)
    a, b, vol = C.cast(fa, C.c_void_p), C.cast(fb, C.c_void_p), C.cast(fv, C.c_void_p)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    To = np.zeros(16, np.float32)
    res = ppf.EgomotionResult()
    out = C.c_void_p(0)
    INV = ppf.OSLAM_E_INVALID

    # oslam_pyramid_create
    assert L.oslam_pyramid_create(None, None, C.byref(out)) == INV
    assert L.oslam_pyramid_create(a, None, None) == INV
    for kw in (dict(n_levels=0), dict(n_levels=4), dict(depth_band=0.0), dict(depth_band=-0.01), dict(depth_band=float("nan")),
               dict(depth_band=float("inf"))):
        p = ppf.default_pyramid_params(**kw)
        assert L.oslam_pyramid_create(a, C.byref(p), C.byref(out)) == INV, kw
        assert out.value is None
    # oslam_pyramid_destroy, oslam_pyramid_level
    assert L.oslam_pyramid_destroy(None) == INV
    assert L.oslam_pyramid_level(None, 0, C.byref(out)) == INV and L.oslam_pyramid_level(a, 0, None) == INV
    for k in (0, 1, 2, 3, 1 << 31):                      # the stand-in has no levels
        assert L.oslam_pyramid_level(a, k, C.byref(out)) == INV, k
    C.cast(fa, C.POINTER(C.c_uint))[1] = 2               # two levels: 2 lies beyond it
    assert L.oslam_pyramid_level(a, 2, C.byref(out)) == INV and L.oslam_pyramid_level(a, 1, C.byref(out)) == ppf.OSLAM_OK
    C.cast(fa, C.POINTER(C.c_uint))[1] = 0

    def ego(src=a, dst=b, T=eye, params=None, o=To):
        p = params if params is not None else ppf.default_egomotion_params()
        return L.oslam_pyramid_egomotion(src, dst, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None,
                                         C.byref(p), ppf._p(o) if o is not None else None, C.byref(res))

    def track(v=vol, f=a, T=eye, pp=None, params=None, o=To):
        p = params if params is not None else ppf.default_egomotion_params()
        q = pp if pp is not None else ppf.default_pyramid_params()
        return L.oslam_volume_track_pyramid(v, f, ppf._p(np.ascontiguousarray(T, np.float32)) if T is not None else None,
                                            C.byref(q), C.byref(p), ppf._p(o) if o is not None else None, C.byref(res))

    assert ego(src=None) == ego(dst=None) == ego(o=None) == INV
    assert track(v=None) == track(f=None) == track(T=None) == track(o=None) == INV
    bad_T = []
    T = eye.copy(); T[3] = np.nan; bad_T.append(T)
    T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad_T.append(T)
    T = eye.copy(); T[0] = -1; bad_T.append(T)
    T = eye.copy(); T[13] = 0.5; bad_T.append(T)
    for T in bad_T:
        assert ego(T=T) == INV and track(T=T) == INV, T
    bad_p = [dict(max_corr_dist=0.0), dict(max_corr_dist=float("nan")), dict(min_normal_dot=float("nan")), dict(stop_rot=-1.0),
             dict(min_overlap=1.5), dict(levels=[(0, 1)]), dict(levels=[(17, 1)]), dict(levels=[(4, 4), (2, 1001)]),
             dict(levels=[]), dict(n_levels=4), dict(levels=[(3, 1)]), dict(levels=[(8, 1)]), dict(levels=[(16, 1)]),
             dict(levels=[(1, 2), (5, 2)])]
    for kw in bad_p:
        p = ppf.default_egomotion_params(**kw)
        assert ego(params=p) == INV, kw
        assert track(params=p) == INV, kw
    for kw in (dict(n_levels=0), dict(n_levels=4), dict(depth_band=0.0), dict(depth_band=float("nan"))):
        assert track(pp=ppf.default_pyramid_params(**kw)) == INV, kw
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(ego(params=ppf.default_egomotion_params(levels=[(3, 1)])))
    assert e.value.code == INV and "1, 2 or 4" in str(e.value)
    # a level the pyramids lack: the stand-ins have none, then one has three and the other two
    assert ego() == INV and "does not have" in L.oslam_last_error().decode()
    C.cast(fa, C.POINTER(C.c_uint))[1] = 3
    C.cast(fb, C.POINTER(C.c_uint))[1] = 2
    assert ego() == INV and "does not have" in L.oslam_last_error().decode()
    assert track(pp=ppf.default_pyramid_params(n_levels=2)) == INV and "does not have" in L.oslam_last_error().decode()
    C.cast(fa, C.POINTER(C.c_uint))[1] = 2               # the frame has two levels, the schedule asks for three
    assert track() == INV and "does not have" in L.oslam_last_error().decode()
    # pyramids on different devices: the stand-in destination says device 1
    C.cast(fb, C.POINTER(C.c_int))[0] = 1
    assert ego() == INV and "different devices" in L.oslam_last_error().decode()
    C.cast(fb, C.POINTER(C.c_int))[0] = 0
    C.cast(fa, C.POINTER(C.c_uint))[1] = 3
    C.cast(fv, C.POINTER(C.c_int))[0] = 1
    assert track() == INV and "different devices" in L.oslam_last_error().decode()
    # src == dst: the identity at once, without a device, whatever T_init is
    To[:] = 7
    Ti = np.eye(4, dtype=np.float32)
    Ti[:3, 3] = [1, 2, 3]
    assert ego(dst=a, T=Ti.reshape(16)) == ppf.OSLAM_OK
    assert np.array_equal(To, eye) and list(res.iterations) == [0, 0, 0] and res.launches == 0 and res.ok == 1
    assert res.converged == 1 and res.overlap == 1.0


# ---------------------------------------------------------------- the restated egomotion
@pytest.fixture(scope="module")
def worlds(synth):
    return {seed: E.make_world(synth, seed) for seed in SEEDS}


def stream_of(synth, world, seed, m, size=None):
    traj = E.trajectory(synth, seed, frames=FRAMES, deg=3.0 * m, step=0.03 * m)
    cam = E.CAM if size is None else dict(E.CAM, **{k: size[k] for k in ("fx", "fy", "cx", "cy")})
    pyrs = [P.with_maps(P.pyramid(E.render(synth, world, T, **(size or {})), cam, E.MAX_JUMP)) for T in traj]
    return traj, pyrs


def test_pyramid_egomotion_splits_at_level_boundaries(synth, worlds):
    """The restated pyramid egomotion equals the chain of single-level calls on the levels' maps, each from the previous
    pose: T, iterations, and the result of the last call.  On one-level pyramids it is camera_ref.egomotion itself."""
    import edge_inputs
    size = dict(edge_inputs.RAGGED)
    _, pyrs = stream_of(synth, worlds[0], 0, 1, size)
    a, b = pyrs[0], pyrs[1]
    for sums in ("f64", "f32"):
        T, r = P.egomotion_pyramid(a, b, sums=sums)
        Tc, its, last = None, [], None
        for stride, n in E.default_params()["levels"]:
            k = {4: 2, 2: 1, 1: 0}[stride]
            Tc, last = E.egomotion(a[k]["maps"], b[k]["maps"], b[k]["cam"], Tc, sums=sums, levels=[(1, n)])
            its.append(last["iterations"][0])
        assert T.tobytes() == Tc.tobytes() and r["iterations"] == its, (sums, r, its)
        assert (r["correspondences"], r["rmse"], r["overlap"], r["converged"], r["ok"]) == \
            (last["correspondences"], last["rmse"], last["overlap"], last["converged"], last["ok"]), (sums, r, last)
    # a schedule on level 0 alone is the single-image egomotion at stride 1, level for level
    T1, r1 = P.egomotion_pyramid(a[:1], b[:1], levels=[(1, 3), (1, 4)])
    T2, r2 = E.egomotion(a[0]["maps"], b[0]["maps"], b[0]["cam"], levels=[(1, 3), (1, 4)])
    assert T1.tobytes() == T2.tobytes() and r1["iterations"] == r2["iterations"]
    assert (r1["correspondences"], r1["rmse"], r1["overlap"], r1["converged"]) == \
        (r2["correspondences"], r2["rmse"], r2["overlap"], r2["converged"])
    with pytest.raises(ValueError):
        P.egomotion_pyramid(a[:2], b, levels=[(4, 1)])
    # a level without iterations is passed over; nothing scheduled gives the pose back
    Ti = np.eye(4, dtype=np.float32)
    Ti[0, 3] = 0.01
    T0, r0 = P.egomotion_pyramid(a, b, Ti, levels=[(4, 0), (2, 0)])
    assert T0.tobytes() == Ti.tobytes() and r0["iterations"] == [0, 0] and r0["overlap"] == 0.0
    T3, r3 = P.egomotion_pyramid(a, b, levels=[(4, 2), (2, 0), (1, 2)])
    T4, _ = P.egomotion_pyramid(a, b, levels=[(4, 2), (1, 2)])
    assert T3.tobytes() == T4.tobytes() and r3["iterations"][1] == 0


def followed(rows):
    """The criterion of test_restatement_follows_the_moving_camera on every pair of a stream."""
    return all(rot < E.ROT_BOUND and tr < E.TRANS_BOUND and crot < E.CHAIN_ROT_BOUND and ctr < E.CHAIN_TRANS_BOUND and ok and
               ov >= E.OVERLAP_CONSECUTIVE_MIN for rot, tr, crot, ctr, ov, ok in rows)


def test_calibration_pyramid_against_single_image(synth, worlds):
    table = {}                                            # (variant, gate, m, seed) -> rows per pair
    for m in MULTIPLES:
        for seed in SEEDS:
            traj, pyrs = stream_of(synth, worlds[seed], seed, m)
            for gate in GATES:
                for variant in ("parent", "pyramid"):
                    chain, rows = np.eye(4), []
                    for f in range(1, FRAMES):
                        if variant == "parent":
                            T, r = E.egomotion(pyrs[f - 1][0]["maps"], pyrs[f][0]["maps"], E.CAM, max_corr_dist=gate)
                        else:
                            T, r = P.egomotion_pyramid(pyrs[f - 1], pyrs[f], max_corr_dist=gate)
                        rot, tr = refine_ref.pose_error(T, E.truth(traj[f - 1], traj[f]))
                        chain = T.astype(np.float64) @ chain
                        crot, ctr = refine_ref.pose_error(chain, E.truth(traj[0], traj[f]))
                        rows.append((rot, tr, crot, ctr, r["overlap"], r["ok"]))
                    table[variant, gate, m, seed] = rows
                    worst = max(rows, key=lambda x: x[1])
                    print("m %d seed %d %-7s gate %.2f: worst pair rot %.4f deg trans %.4f m overlap %.3f  %s"
                          % (m, seed, variant, gate, worst[0], worst[1], min(x[4] for x in rows),
                             "followed" if followed(rows) else "NOT followed"))
    reach = {}
    for variant in ("parent", "pyramid"):
        for gate in GATES:
            ms = [m for m in MULTIPLES if all(followed(table[variant, gate, m, s]) for s in SEEDS)]
            reach[variant, gate] = max(ms) if ms else 0
    print("largest m followed on all seeds:", reach)
    # (1) m = 1, the default gate: both end on the same full-resolution level and differ in where it starts
    for seed in SEEDS:
        for pa, py in zip(table["parent", 0.30, 1, seed], table["pyramid", 0.30, 1, seed]):
            assert py[0] <= 2.0 * pa[0] and py[1] <= 2.0 * pa[1], (seed, pa, py)
    # (2) the pyramid reaches at least as far as the single image pair, with either gate
    for gate in GATES:
        assert reach["pyramid", gate] >= reach["parent", gate], (gate, reach)
