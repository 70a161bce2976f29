"""CPU: the render stage's arguments, its defaults, the restatement's independence of order, the calibration of
`footprint`, and the moving-object frames on the restatements (include/oslam.h at oslam_render_create).

Calibration of footprint (test_default_footprint_leaves_no_holes): synth model 0 at the object scale of the camera tests
(0.3), 20000 points voxel-gridded at d_dist = 0.0597 (646 points), rendered by tests/render_ref.py at 640 x 480
(fx = fy = 525) at three seeded rotations 3.5, 4.25 and 5 m before the camera, where the cap of 8 pixels does not bind
(half-widths up to 7, 6 and 5).  A hole is an unlabelled pixel whose four axis neighbours are labelled.  Measured:

    footprint   holes / labelled pixels, the three poses
    0.50        3 / 8782   2 / 6626   6 / 6181      (0.03 %, 0.03 %, 0.10 %)
    0.75        0 / 10313  0 / 7577   0 / 7132      (0 %)
    1.00        0 / 11220  0 / 8524   0 / 7844

0.75 keeps the holes at 0 % <= 1 %: it is the default.  (At full scale, d_dist = 0.2 at 5 m, every half-width is the
cap of 8 and the footprint has no say: a model that near is sparser than 17 pixels and needs a denser cloud.)

The moving-object frames (tests/render_world.py; 160 x 120, the camera turns 1.5 degrees and moves 3 cm, the object
covers 18 % of the pixels, turns 3 degrees and moves 5.4 cm on its own).  Error of the camera motion against the truth,
ppf.ht_dist (metres, radians), camera_ref.egomotion on the restatement's images:

    (a) raw frames                      0.012513 m   0.0017324 rad
    (b) object masked out (REMOVE)      0.002205 m   0.0003007 rad
    (c) frames without the object       0.002281 m   0.0003035 rad

(a) is 5.5 times (c).  (b) equals (c) to 4 % here; the margin the tests allow is MARGIN = 1.5 times (c) in both: the mask
takes a fifth of the pixels and a ring of two more around the silhouette, which costs a least-squares estimate about
1 / sqrt(0.8) = 1.12, and the rest is headroom for the pixels at the silhouette; (a) lies far outside it.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_edge_inputs as E  # noqa: E402
import render_ref as R  # noqa: E402
import render_world as RW  # noqa: E402

F = np.float32
MARGIN = 1.5


def test_render_and_mask_params_default(built_lib, ppf):
    p, want = ppf.default_render_params(), R.default_params()
    assert p.footprint == F(want["footprint"]) and p.max_splat == want["max_splat"] == 8
    assert p.depth_tol == F(want["depth_tol"]) and p.keep_back == want["keep_back"] and list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_render_params(max_splat=3).max_splat == 3
    with pytest.raises(TypeError):
        ppf.default_render_params(no_such_field=1)
    m = ppf.MaskParams()
    assert ppf.lib().oslam_mask_params_default(C.byref(m)) == ppf.OSLAM_OK
    want = R.default_mask_params()
    assert (m.mode, m.dilate, m.only) == (want["mode"], want["dilate"], want["only"]) == (ppf.MASK_REMOVE, 2, -1)
    assert ppf.lib().oslam_render_params_default(None) == ppf.OSLAM_E_INVALID
    assert ppf.lib().oslam_mask_params_default(None) == ppf.OSLAM_E_INVALID
    for name in ("oslam_render_create", "oslam_db_render", "oslam_render_view", "oslam_render_labels",
                 "oslam_render_destroy", "oslam_view_mask", "oslam_view_info"):
        assert name in ppf._SIGNATURES


def test_render_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: stand-in handles (zeroed host memory)
    are never looked at, on a machine with or without a GPU."""
    L = ppf.lib()
    bufs = [C.create_string_buffer(16384) for _ in range(4)]
    m0, m1, db, v = (C.cast(b, C.c_void_p) for b in bufs)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    good = ppf.Camera(100.0, 100.0, 16.0, 12.0, 1.0, 0.5, 10.0, 0.05)
    out = C.c_void_p(0)
    res = (ppf.RenderResult * 4)()
    member = np.zeros(4, np.uint32)

    def call(T=eye, H=1, params=None, cam=good, w=32, h=24, models=(m0,), o=True, T_null=False, ms_null=False, db_call=False):
        T = np.ascontiguousarray(T, np.float32).reshape(-1)
        arr = (C.c_void_p * max(len(models), 1))(*[x.value if x is not None else None for x in models])
        p = C.byref(params) if params is not None else None
        tp = None if T_null else ppf._p(T)
        op = C.byref(out) if o else None
        cp = C.byref(cam) if cam is not None else None
        if db_call:
            return L.oslam_db_render(db, None if ms_null else ppf._p(member), tp, H, cp, w, h, p, op, res)
        return L.oslam_render_create(None if ms_null else arr, tp, H, cp, w, h, p, op, res)

    for db_call in (False, True):
        kw = dict(db_call=db_call)
        assert call(ms_null=True, **kw) == ppf.OSLAM_E_INVALID
        assert call(T_null=True, **kw) == ppf.OSLAM_E_INVALID
        assert call(cam=None, **kw) == ppf.OSLAM_E_INVALID
        assert call(o=False, **kw) == ppf.OSLAM_E_INVALID
        assert call(H=0, **kw) == ppf.OSLAM_E_INVALID
        assert call(T=np.tile(eye, 1025), H=1025, models=(m0,) * 1025, **kw) == ppf.OSLAM_E_INVALID
        for bad in (dict(footprint=0.0), dict(footprint=-1.0), dict(footprint=float("nan")), dict(footprint=float("inf")),
                    dict(max_splat=9), dict(depth_tol=0.0), dict(depth_tol=-2.0), dict(depth_tol=float("nan")),
                    dict(depth_tol=float("inf"))):
            assert call(params=ppf.default_render_params(**bad), **kw) == ppf.OSLAM_E_INVALID, bad
        for cam in (ppf.Camera(0.0, 100.0, 16.0, 12.0, 1.0, 0.5, 10.0, 0.05), ppf.Camera(100.0, 100.0, 16.0, 12.0, 0.0, 0.5, 10.0, 0.05),
                    ppf.Camera(100.0, 100.0, 16.0, 12.0, 1.0, 0.0, 10.0, 0.05), ppf.Camera(100.0, 100.0, 16.0, 12.0, 1.0, 5.0, 1.0, 0.05),
                    ppf.Camera(100.0, 100.0, float("nan"), 12.0, 1.0, 0.5, 10.0, 0.05),
                    ppf.Camera(100.0, 100.0, 16.0, 12.0, 1.0, 0.5, 10.0, -1.0)):
            assert call(cam=cam, **kw) == ppf.OSLAM_E_INVALID
        for w, h in ((0, 24), (32, 0), (-1, 24), (16385, 24)):
            assert call(w=w, h=h, **kw) == ppf.OSLAM_E_INVALID
        bad_T = []
        T = eye.copy(); T[3] = np.nan; bad_T.append(T)
        T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad_T.append(T)
        T = eye.copy(); T[0] = -1; bad_T.append(T)
        T = eye.copy(); T[13] = 0.5; bad_T.append(T)
        for T in bad_T:
            assert call(T, **kw) == ppf.OSLAM_E_INVALID, T
            assert call(np.concatenate([np.zeros(16, np.float32), T]), H=2, models=(m0, m1), **kw) == ppf.OSLAM_E_INVALID
    assert call(T=np.tile(eye, 2), H=2, models=(m0, None)) == ppf.OSLAM_E_INVALID           # a NULL model
    # the handles, read only now: models on different devices; a member index outside the (empty stand-in) database
    C.cast(bufs[1], C.POINTER(C.c_int))[0] = 1
    assert call(T=np.tile(eye, 2), H=2, models=(m0, m1)) == ppf.OSLAM_E_INVALID
    assert "different devices" in L.oslam_last_error().decode()
    C.cast(bufs[1], C.POINTER(C.c_int))[0] = 0
    assert call(db_call=True) == ppf.OSLAM_E_INVALID
    assert "outside the database" in L.oslam_last_error().decode()
    assert not out.value
    # the render's own calls
    hv = C.c_void_p(0)
    lab = np.zeros(4, np.int32)
    assert L.oslam_render_view(None, C.byref(hv)) == ppf.OSLAM_E_INVALID
    assert L.oslam_render_view(v, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_render_labels(None, ppf._p(lab)) == ppf.OSLAM_E_INVALID
    assert L.oslam_render_labels(v, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_render_destroy(None) == ppf.OSLAM_E_INVALID
    cam, wi, hi = ppf.Camera(), C.c_int(0), C.c_int(0)
    assert L.oslam_view_info(None, C.byref(cam), C.byref(wi), C.byref(hi)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_info(v, None, C.byref(wi), C.byref(hi)) == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(call(params=ppf.default_render_params(max_splat=12)))
    assert e.value.code == ppf.OSLAM_E_INVALID and "max_splat" in str(e.value)


def test_mask_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    L = ppf.lib()
    bufs = [C.create_string_buffer(16384) for _ in range(2)]
    v, r = (C.cast(b, C.c_void_p) for b in bufs)
    out = C.c_void_p(0)
    res = ppf.MaskResult()

    def params(**kw):
        p = ppf.MaskParams()
        L.oslam_mask_params_default(C.byref(p))
        for k, x in kw.items():
            setattr(p, k, x)
        return p
    assert L.oslam_view_mask(None, r, None, C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_mask(v, None, None, C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    assert L.oslam_view_mask(v, r, None, None, C.byref(res)) == ppf.OSLAM_E_INVALID
    for bad in (dict(mode=2), dict(mode=-1), dict(dilate=9), dict(only=-2)):
        assert L.oslam_view_mask(v, r, C.byref(params(**bad)), C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID, bad
    # a stand-in render holds no images: refused without a device call
    assert L.oslam_view_mask(v, r, None, C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    assert not out.value
    with pytest.raises(ValueError):
        ppf.mask_view(None, None, mode="neither")


def test_restatement_does_not_depend_on_order(synth):
    """points shuffled within a model, and hypotheses shuffled with their labels mapped back: the same images"""
    c = E.size_case(synth)
    ref = E.reference(c)
    rng = np.random.default_rng(12)
    clouds = []
    for p, n, d in c["clouds"]:
        o = rng.permutation(len(p))
        clouds.append((p[o], n[o], d))
    a = R.render(clouds, c["T"], c["cam"], c["w"], c["h"])
    assert a["z"].tobytes() == ref["z"].tobytes() and np.array_equal(a["labels"], ref["labels"])
    assert np.array_equal(a["drawn"], ref["drawn"]) and np.array_equal(a["pixels"], ref["pixels"])
    m = E.many_case(256)
    rm = E.reference(m)
    o = rng.permutation(256)
    b = R.render([E.hypotheses(m)[k] for k in o], m["T"][o], m["cam"], m["w"], m["h"])
    # z never depends on the order; the labels do only where two hypotheses put bit-equal z on one pixel
    assert b["z"].tobytes() == rm["z"].tobytes()
    back = np.where(b["labels"] >= 0, o[np.clip(b["labels"], 0, None)], -1)
    differ = back != rm["labels"]
    assert np.array_equal(b["drawn"], rm["drawn"][o])
    for y, x in np.argwhere(differ):
        za = m["T"][back[y, x], 2, 3] + E.hypotheses(m)[back[y, x]][0][:, 2]
        assert rm["z"][y, x] in za                   # the other hypothesis draws the very same depth there: a tie
    assert differ.sum() < (rm["labels"] >= 0).sum()


def test_default_footprint_leaves_no_holes(synth, oracle):
    cam = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=1.0, z_min=0.5, z_max=12.0)
    mp, mn = synth.make_model(0, 20000)
    mp = np.ascontiguousarray(mp * F(0.3))
    d = synth.d_dist_for(mp, 0.05)
    gp, gn = oracle.voxel_grid(mp, mn, d)
    rng = synth.SplitMix64(311)
    for f in range(3):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.3 * f - 0.3, 0.2 - 0.2 * f, 3.5 + 0.75 * f]
        k = R.points(gp, gn, T, cam, 640, 480, d)[3]
        r = R.render([(gp, gn, d)], T[None], cam, 640, 480, footprint=R.default_params()["footprint"])
        holes, labelled = R.holes(r["labels"])
        print("pose %d: %d model points, half-widths up to %d, %d holes in %d labelled pixels (%.3f %%)"
              % (f, len(gp), k.max(), holes, labelled, 100.0 * holes / labelled))
        assert k.max() < 8 and labelled > 5000
        assert holes <= 0.01 * labelled, (f, holes, labelled)


@pytest.fixture(scope="module")
def world(synth, oracle):
    return RW.make(synth, oracle)


def test_masking_the_moving_object_repairs_the_camera_motion(ppf, world):
    masked, counts = RW.masked_frames(world)
    for f in range(2):
        c = counts[f]
        share = c["object_pixels"] / c["valid_in"]
        assert 0.12 < share < 0.30 and c["valid_in"] == c["valid_out"] + c["object_pixels"], c
        # the mask takes nine tenths of the object's pixels (measured: 91.5 % and 92.4 %; the rest lies at grazing
        # parts of the silhouette that the sparse model does not reach) and nothing that is not the object
        empty = world["empty"][f].astype(np.float32) * F(0.001)
        obj = world["frames"][f] != world["empty"][f]
        left = (masked[f] > 0) & (np.abs(masked[f] - empty) > 0.05)
        gone = (masked[f] == 0) & (world["empty"][f] > 0)
        assert left.sum() < 0.10 * obj.sum() and not (left & ~obj).any(), (left.sum(), obj.sum())
        assert (gone & ~obj).sum() <= 0.01 * obj.sum(), ((gone & ~obj).sum(), obj.sum())
    err = {}
    for name, (T, res) in RW.cpu_three_ways(world).items():
        err[name] = ppf.ht_dist(T, world["truth"])
        print("%-6s %.6f m %.7f rad, overlap %.3f" % (name, err[name][0], err[name][1], res["overlap"]))
        assert res["ok"], (name, res)
    for k in (0, 1):
        assert err["raw"][k] > 3.0 * err["empty"][k], err          # (a) is clearly worse than (c)
        assert err["masked"][k] < err["raw"][k], err               # (b) is better than (a)
        assert err["masked"][k] <= MARGIN * err["empty"][k], err   # and within the margin of (c)
