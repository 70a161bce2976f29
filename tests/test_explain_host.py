"""CPU: the explain stage's yardstick, its calibration, its rectangles and its arguments (include/oslam.h at
oslam_explain).

Calibration (explain_calib): the 11-member database of tests/arbitrate_calib.py (synthetic models 0..9 and 36, the near
twin of model 0; 1500 points voxel-gridded at d_dist), the six seeded frames of tests/verify_calib.py (seed 211, every
other one with the non-member occluder), every member's voting pose from the oracle (df 4), refined by
tests/refine_ref.py, verified by tests/view_ref.py, then judged by tests/explain_ref.py.  Measured on the CPU when the
default was set.  Verification finds models 1..9 on no frame, so "what verification found" is a subset of {0, 36}.

Conflict rate through / (agree + through) at the refined poses (every member alone; 1..9: the range over the members):

    frame  verified   depth_tol 1.0                      depth_tol 0.5
                      0      36     1..9                  0      36     1..9
    0      0, 36      0.120  0.165  0.300 .. 0.634        0.179  0.246  0.502 .. 0.843
    1      0          0.187  0.251  0.332 .. 0.642        0.279  0.330  0.447 .. 0.866
    2      0, 36      0.171  0.217  0.315 .. 0.640        0.262  0.309  0.541 .. 0.847
    3      0          0.232  0.274  0.138 .. 0.661        0.392  0.520  0.333 .. 0.856
    4      0, 36      0.192  0.223  0.302 .. 0.701        0.345  0.367  0.590 .. 0.888
    5      0, 36      0.141  0.194  0.246 .. 0.643        0.186  0.247  0.379 .. 0.853

Model 0 has the lower rate than 36 on 6 of 6 frames at both tolerances; the gap is 0.031 .. 0.064 at 1.0 and 0.022 ..
0.128 at 0.5: that, not the share gap below, is the thin margin of this rule.  The two low rates of the absent members
are member 9 on frames 3 and 5 (0.138, 0.246), a pose that hides behind the occluder; its `visible` is 0.703 and 0.421
there and oslam_verify's coverage rejects both (0.463, 0.293): this score complements oslam_verify and does not replace
it.  On frame 3 the twin's pose is 111 degrees from the truth.

First-round shares (min_owned_share 0) and the kept set at min_owned_share 0.52, over what verification found; "0 and 36
alone" (both poses whether verified or not) gives the same numbers on frames 0, 2, 4, 5 and is listed for 1 and 3:

    frame  depth_tol  tile      share 0   share 36   kept      0 and 36 alone: share 36, kept
    0      1.0        36 auto   1.000     0.042      0
    0      1.0        8         1.000     0.068      0
    0      0.5        36 auto   1.000     0.042      0
    0      0.5        8         1.000     0.081      0
    1      1.0        45 auto   1.000     -          0         0.000  0
    1      1.0        8         1.000     -          0         0.113  0
    1      0.5        45 auto   1.000     -          0         0.000  0
    1      0.5        8         1.000     -          0         0.147  0
    2      1.0        41 auto   1.000     0.000      0
    2      1.0        8         1.000     0.063      0
    2      0.5        41 auto   1.000     0.000      0
    2      0.5        8         1.000     0.080      0
    3      1.0, 0.5   41 auto   1.000     -          0         1.000  0, 36 (the poses do not meet)
    3      1.0, 0.5   8         1.000     -          0         1.000  0, 36
    4      1.0        30 auto   1.000     0.116      0
    4      1.0        8         1.000     0.081      0
    4      0.5        30 auto   1.000     0.095      0
    4      0.5        8         1.000     0.099      0
    5      1.0        32 auto   1.000     0.000      0
    5      1.0        8         1.000     0.019      0
    5      0.5        32 auto   1.000     0.000      0
    5      0.5        8         1.000     0.025      0

tests/arbitrate_ref.py over the same lists keeps 0 on frames 0, 1, 2, 3, 5 and keeps 36 on frame 4 (shares 0.343
against 1.000): the frame that depth residuals cannot separate, and this rule does.  Where the two compete, the present
model's share is 1.000 and the twin's at most 0.116 (0.147 with the unverified pose of frame 1): the gap is wide because
ownership follows one global score per hypothesis.  min_owned_share stays at the arbitration's 0.52, which lies inside
it.  The table reproduces the prototype's of the issue that asked for this stage.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arbitrate_ref as A  # noqa: E402
import explain_calib as EC  # noqa: E402
import explain_ref as X  # noqa: E402
import render_ref as R  # noqa: E402

F = np.float32
KCAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=30.0)


@pytest.fixture(scope="module")
def calib(synth, oracle):
    """the six calibration frames with the poses of model 0 and its twin (the members verification ever finds)"""
    return EC.frames(synth, oracle, members=[0, 36], n_frames=6, seed=211)


def test_the_present_model_is_kept_and_its_twin_suppressed(calib):
    frames, hyp = calib
    p = X.default_params()
    contested = [f for f, fr in enumerate(frames) if fr["found"] == [0, 1]]
    alone = [f for f, fr in enumerate(frames) if fr["found"] == [0]]
    assert contested == [0, 2, 4, 5] and alone == [1, 3], [fr["found"] for fr in frames]
    twin_shares = []
    for f, fr in enumerate(frames):
        for tol in EC.DEPTH_TOLS:
            for tile in EC.TILES:
                raw, res = EC.judge(hyp, fr, fr["found"], tol, tile, p["min_owned_share"])
                assert X.kept(res) == [0], (f, tol, tile, res)
                assert raw[0]["share"] == F(1), (f, tol, tile, raw[0])
                if f in contested:
                    assert res[1]["suppressed_by"] == 0 and EC.rate(raw[0]) < EC.rate(raw[1]), (f, tol, tile, raw)
                    twin_shares.append(float(raw[1]["share"]))
        # every member alone, both poses whether verified or not: model 0 has the lower conflict rate on 6 of 6
        for tol in EC.DEPTH_TOLS:
            r0, r1 = (X.explain([hyp[j]], [fr["T"][j]], fr["img"], EC.CAM, depth_tol=tol)[0] for j in (0, 1))
            assert EC.rate(r0) < EC.rate(r1), (f, tol, EC.rate(r0), EC.rate(r1))
    # the default lies inside the measured gap of the first-round shares
    assert max(twin_shares) < 0.15 < p["min_owned_share"] <= 1.0, max(twin_shares)


def test_frame_4_where_depth_residuals_keep_the_twin(calib):
    """The one frame of the calibration where oslam_arbitrate suppresses the real object: the ICP leaves model 0 in the
    worse pose and the twin's residuals are smaller.  The conflict rates decide the other way."""
    frames, hyp = calib
    fr = frames[4]
    T = EC.only(fr["T"], fr["found"])
    _, kept = A.arbitrate(hyp, T, fr["img"], EC.CAM)
    assert kept.tolist() == [False, True]
    res = X.explain(hyp, T, fr["img"], EC.CAM)
    assert X.kept(res) == [0] and res[1]["suppressed_by"] == 0 and res[0]["conflict_q"] < res[1]["conflict_q"], res


def test_a_duplicate_is_suppressed_by_its_first_copy(calib):
    frames, hyp = calib
    fr = frames[0]
    res = X.explain([hyp[0], hyp[0], hyp[0]], [fr["T"][0]] * 3, fr["img"], EC.CAM)
    assert X.kept(res) == [0] and [r["suppressed_by"] for r in res] == [-1, 0, 0]
    assert res[0]["conflict_q"] == res[1]["conflict_q"] == res[2]["conflict_q"] and res[0]["rounds"] == 3


def test_two_copies_side_by_side_both_survive(synth):
    mp, mn = synth.make_model(0, 1500)
    d = synth.d_dist_for(mp, 0.05)
    ext = synth.bbox_extent(mp)
    dense, _ = synth.make_model(0, 200000)
    Ts, pts = [], []
    for i in range(2):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(synth.SplitMix64(60 + i))
        T[:3, 3] = [1.15 * ext * (i - 0.5), 0.1 * i, 10.5 + 0.3 * i]
        Ts.append(T)
        pts.append(dense @ T[:3, :3].astype(np.float64).T + T[:3, 3])
    img = synth.render_depth(np.concatenate(pts), background_z=20.0, splat=1)
    res = X.explain([(mp, mn, d)] * 2, Ts, img, KCAM)
    assert X.kept(res) == [0, 1] and all(r["suppressed_by"] == -1 and r["share"] == F(1) for r in res), res


# ---------------------------------------------------------------- by hand: a wall, a patch, the classes
def test_classes_and_scores_by_hand():
    z_h = F([[0, 2, 2, 2], [2, 2, 2, 2]])
    z_o = F([[5, 0, 2.0625, 2.125], [2.25, 1.5, 1.875, 2]])
    tol = F(0.125)
    cls, r = X.classify(z_h, z_o, tol)
    assert cls.tolist() == [[-1, X.UNKNOWN, X.AGREE, X.AGREE], [X.THROUGH, X.OCCLUDED, X.AGREE, X.AGREE]]
    assert r.tolist() == [[0, 0, 32767, 65535], [0, 0, 65535, 0]]
    s = X.scores(cls, r, tol)
    assert (s["pixels"], s["agree"], s["occluded"], s["through"], s["unknown"], s["resid_sum"]) == (7, 4, 1, 1, 1, 163837)
    assert s["explained"] == F(4) / F(5) and s["visible"] == F(4) / F(6) and s["conflict_q"] == 65535 // 5
    assert s["mean_residual"] == F(((163837 / 4) / 65535.0) * 0.125)
    one_ulp = np.nextafter(F(2.125), F(np.inf))
    cls, _ = X.classify(F([[2, 2]]), np.array([[one_ulp, np.nextafter(F(1.875), F(0))]], np.float32), tol)
    assert cls.tolist() == [[X.THROUGH, X.OCCLUDED]]


# ---------------------------------------------------------------- the rectangle, through ctypes, no device
RECT_CAMS = [(dict(fx=75.0, fy=77.0, cx=40.3, cy=31.7, depth_scale=1.0, z_min=0.5, z_max=8.0), 83, 61),
             (dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=1.0, z_min=0.5, z_max=12.0), 640, 480)]


def rect_poses(synth, rng, cam, w, h, radius):
    """poses that put the cloud's centre on every border and corner, off the image, across z_min and behind the camera"""
    out = []
    us = (-0.4 * w, 0.0, 0.5 * w, w - 1.0, 1.4 * w)
    vs = (-0.4 * h, 0.0, 0.5 * h, h - 1.0, 1.4 * h)
    for u in us:
        for v in vs:
            for z in (3.0 * radius + cam["z_min"], 0.6 * cam["z_max"]):
                T = np.eye(4, dtype=np.float32)
                T[:3, :3] = synth.random_rotation(rng)
                T[:3, 3] = [(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z]
                out.append(T)
    for z in (cam["z_min"], cam["z_min"] - 0.5 * radius, 0.5 * radius, 0.0, -0.5 * radius, -3.0 * radius, cam["z_max"],
              cam["z_max"] + 0.9 * radius, cam["z_max"] + 2.0 * radius):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.3 * radius, -0.2 * radius, z]
        out.append(T)
    T = out[7].copy()
    T[:3, :3] *= F(1.0003)                               # still rigid to the pose check: the sphere grows with it
    out.append(T)
    return out


def test_rectangle_contains_everything_the_hypothesis_draws(built_lib, ppf, synth):
    rng = synth.SplitMix64(515)
    empty = whole = partial = drew = 0
    for k, scale in ((0, 0.12), (3, 0.3), (7, 0.05)):
        mp, mn = synth.make_model(k, 300)
        mp = np.ascontiguousarray(mp * F(scale))
        d = synth.d_dist_for(mp, 0.05)
        centre = mp.astype(np.float64).mean(axis=0)
        radius = float(np.sqrt(((mp.astype(np.float64) - centre) ** 2).sum(axis=1)).max())
        for cam, w, h in RECT_CAMS:
            pc = ppf.Camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], 1.0, cam["z_min"], cam["z_max"], 0.05)
            for T in rect_poses(synth, rng, cam, w, h, radius):
                for max_splat, keep_back in ((8, 0), (0, 1), (3, 1)):
                    x0, y0, rw, rh = ppf.explain_rect(centre, radius, T, pc, w, h, max_splat)
                    assert 0 <= x0 and 0 <= y0 and x0 + rw <= w and y0 + rh <= h and rw >= 0 and rh >= 0
                    draw, u, v, kk, _, _ = R.points(mp, mn, T, cam, w, h, d, 0.75, max_splat, keep_back)
                    if draw.any():
                        u0, u1 = np.maximum(u - kk, 0)[draw].min(), np.minimum(u + kk, w - 1)[draw].max()
                        v0, v1 = np.maximum(v - kk, 0)[draw].min(), np.minimum(v + kk, h - 1)[draw].max()
                        assert x0 <= u0 and u1 < x0 + rw and y0 <= v0 and v1 < y0 + rh, (k, w, T, (x0, y0, rw, rh), (u0, u1, v0, v1))
                        drew += 1
                    empty += rw == 0 or rh == 0
                    whole += (rw, rh) == (w, h)
                    partial += 0 < rw * rh < w * h
    assert min(empty, whole, partial) > 10 and drew > 100, (empty, whole, partial, drew)
    # a skipped hypothesis has the empty rectangle
    assert ppf.explain_rect([0, 0, 0], 1.0, np.zeros((4, 4), np.float32), pc, 640, 480)[2:] == (0, 0)


def test_rectangle_rejects_bad_arguments(built_lib, ppf):
    L = ppf.lib()
    cam = ppf.Camera(525.0, 525.0, 319.5, 239.5, 1.0, 0.5, 12.0, 0.05)
    c = np.zeros(3, np.float64)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    out = np.zeros(4, np.int32)

    def call(centre=c, radius=1.0, T=eye, camera=cam, w=640, h=480, max_splat=8, o=out):
        return L.oslam_explain_rect(ppf._p(centre) if centre is not None else None, radius, ppf._p(T) if T is not None else None,
                                    C.byref(camera) if camera is not None else None, w, h, max_splat,
                                    ppf._p(o) if o is not None else None)
    INV = ppf.OSLAM_E_INVALID
    assert call() == ppf.OSLAM_OK
    assert call(centre=None) == INV and call(T=None) == INV and call(camera=None) == INV and call(o=None) == INV
    assert call(radius=-1.0) == INV and call(radius=float("nan")) == INV and call(centre=np.array([0, np.inf, 0])) == INV
    assert call(max_splat=9) == INV and call(w=0) == INV and call(h=-3) == INV
    assert call(camera=ppf.Camera(0.0, 525.0, 319.5, 239.5, 1.0, 0.5, 12.0, 0.05)) == INV
    T = eye.copy(); T[0] = 2.0
    assert call(T=T) == INV


# ---------------------------------------------------------------- parameters and arguments
def test_explain_params_default(built_lib, ppf):
    p = ppf.default_explain_params()
    want = X.default_params()
    r, a = ppf.default_render_params(), ppf.default_arbitrate_params()
    assert (p.footprint, p.max_splat, p.keep_back) == (r.footprint, r.max_splat, r.keep_back)
    assert (p.tile, p.tile_spacing, p.min_tiles) == (a.tile, a.tile_spacing, a.min_tiles)
    assert p.depth_tol == F(1.0) and p.min_owned_share == F(want["min_owned_share"]) and list(p.reserved) == [0, 0, 0, 0]
    for k, v in want.items():
        assert getattr(p, k) == F(v) if isinstance(v, float) else getattr(p, k) == v, k
    assert ppf.default_explain_params(tile=16, keep_back=1).tile == 16
    with pytest.raises(TypeError):
        ppf.default_explain_params(window=1)
    assert C.sizeof(ppf.ExplainResult) == 88 and C.sizeof(ppf.ExplainParams) == 48


def test_explain_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: stand-in handles (zeroed host
    memory) are never looked at, on a machine with or without a GPU."""
    L = ppf.lib()
    bufs = [C.create_string_buffer(4096) for _ in range(3)]
    m, v, db = [C.cast(b, C.c_void_p) for b in bufs]
    ms = (C.c_void_p * 2)(m, m)
    eye2 = np.stack([np.eye(4, dtype=np.float32).reshape(16)] * 2)
    res = (ppf.ExplainResult * 2)()
    cnt, sm, z = np.zeros(64, np.uint32), np.zeros(64, np.uint64), np.zeros(64, np.float32)
    tile, nt = C.c_uint32(0), C.c_size_t(0)

    def call(T=eye2, params=None, mm=ms, vv=v, r=res, H=2):
        T = np.ascontiguousarray(T, np.float32)
        p = params if params is not None else ppf.default_explain_params()
        return L.oslam_explain(mm, ppf._p(T), H, vv, C.byref(p), r)

    def claims(T=eye2, params=None, mm=ms, vv=v, H=2, c=cnt, s=sm):
        T = np.ascontiguousarray(T, np.float32)
        p = params if params is not None else ppf.default_explain_params()
        return L.oslam_explain_claims(mm, ppf._p(T), H, vv, C.byref(p), ppf._p(c) if c is not None else None,
                                      ppf._p(s) if s is not None else None, 64, C.byref(tile), C.byref(nt))

    def ztap(T=eye2, params=None, mm=ms, vv=v, H=2, h=0, o=z):
        T = np.ascontiguousarray(T, np.float32)
        p = params if params is not None else ppf.default_explain_params()
        return L.oslam_explain_z(mm, ppf._p(T), H, vv, C.byref(p), h, ppf._p(o) if o is not None else None)

    INV = ppf.OSLAM_E_INVALID
    assert call(mm=None) == INV and call(vv=None) == INV and call(r=None) == INV
    assert L.oslam_explain(ms, None, 2, v, None, res) == INV
    assert call(H=0) == INV and call(H=X.MAX_HYPOTHESES + 1) == INV
    assert call(mm=(C.c_void_p * 2)(m, None)) == INV
    assert claims(mm=None) == INV and claims(vv=None) == INV and claims(c=None) == INV and claims(s=None) == INV and claims(H=0) == INV
    assert ztap(mm=None) == INV and ztap(vv=None) == INV and ztap(o=None) == INV and ztap(H=0) == INV and ztap(h=2) == INV
    bad_T = []
    T = eye2.copy(); T[1, 3] = np.nan; bad_T.append(T)
    T = eye2.copy(); T[1] = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[1, 15] = 1; bad_T.append(T)
    T = eye2.copy(); T[0, 0] = -1; bad_T.append(T)
    T = eye2.copy(); T[1, 13] = 0.5; bad_T.append(T)
    for T in bad_T:
        assert call(T) == INV and claims(T) == INV and ztap(T) == INV, T
    bad_p = [dict(depth_tol=0.0), dict(depth_tol=-1.0), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
             dict(footprint=0.0), dict(footprint=float("nan")), dict(max_splat=9), dict(tile=3), dict(tile=129),
             dict(tile_spacing=0.0), dict(tile_spacing=float("nan")), dict(tile_spacing=float("inf")),
             dict(min_owned_share=1.5), dict(min_owned_share=-0.1), dict(min_owned_share=float("nan"))]
    for kw in bad_p:
        p = ppf.default_explain_params(**kw)
        assert call(params=p) == INV and claims(params=p) == INV and ztap(params=p) == INV, kw
        assert L.oslam_db_explain(db, v, ppf._p(eye2), C.byref(p), res) == INV, kw
    assert L.oslam_db_explain(None, v, ppf._p(eye2), None, res) == INV
    assert L.oslam_db_explain(db, None, ppf._p(eye2), None, res) == INV
    assert L.oslam_db_explain(db, v, None, None, res) == INV
    assert L.oslam_db_explain(db, v, ppf._p(eye2), None, None) == INV
    assert L.oslam_explain_params_default(None) == INV
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(call(params=ppf.default_explain_params(tile=200)))
    assert e.value.code == INV and "tile" in str(e.value)
