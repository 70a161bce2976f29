"""CPU: the arbitration stage's yardstick, its calibration and its arguments (include/oslam.h at oslam_arbitrate).

Calibration (arbitrate_calib.table): an 11-member database (synthetic models 0..9 and 36, the near twin of model 0;
1500 points voxel-gridded at d_dist), the six seeded frames of tests/verify_calib.py (every other one with the
non-member occluder), every member's voting pose from the oracle (df 4), refined by tests/refine_ref.py, verified by
tests/view_ref.py, then arbitrated by tests/arbitrate_ref.py over the members verification found.  Models 1..9 were
found by verification on no frame, so "the largest of the rest" is empty.  First-round shares (min_owned_share 0, so
nothing is suppressed) and mean residuals in scene units (tol = d_dist = 0.175), measured on the CPU when the defaults
were set:

    frame  occluder  verify found   tile_spacing 1 (tile)     tile_spacing 2 (tile)     tile_spacing 3 (tile)    mean residual
                                    share 0   share 36        share 0   share 36        share 0   share 36       0        36
    0      no        0, 36          0.695     0.496   (18)    0.667     0.409   (36)    0.696     0.407   (53)   0.0151   0.0257
    1      yes       0              1.000     -       (23)    1.000     -       (45)    1.000     -       (67)   0.0207   -
    2      no        0, 36          0.583     0.588   (21)    0.694     0.417   (41)    0.632     0.368   (61)   0.0163   0.0203
    3      yes       0              1.000     -       (21)    1.000     -       (41)    1.000     -       (62)   0.0436   -
    4      no        0, 36          0.476     0.747   (15)    0.343     0.692   (30)    0.421     0.727   (45)   0.0359   0.0294
    5      yes       0, 36          0.573     0.618   (16)    0.629     0.421   (32)    0.667     0.381   (48)   0.0132   0.0194

No setting separates 0 from 36 on all six frames: on frame 4 the refined pose of the present model fits the image
worse than the twin's (mean residual 0.0359 against 0.0294) and the twin owns more at every spacing; a rule that
compares residuals follows the pose, and there the twin wins.  The poses explain it: on frame 4 the ICP of model 0
stops after 8 iterations 4.0 degrees from the truth (its voting pose was 8.1 degrees off), the twin's converges to 0.9
degrees.  With model 0 at the ground-truth pose it owns 0.595 against the refined twin's 0.436; with both at the
ground-truth pose their mean residuals are 0.0215 and 0.0219 and the twin owns 0.605 against 0.459: in that view the
facing sides coincide and depth alone does not tell the two apart.  On the other frames where both are found (0, 2, 5):
tile_spacing 1 does not separate (frame 2: 0.583 against 0.588); tile_spacing 2 has present >= 0.629, twin <= 0.421;
tile_spacing 3 has present >= 0.632, twin <= 0.407.  The gaps of 2 and 3 (0.208, 0.225) differ by less than the
frame-to-frame spread of either column, and over frames 0-3 the order is the other way round (0.250, 0.225):
tile_spacing stays at 2, the smaller tile, which keeps the seam between two real neighbours smaller.
min_owned_share is the middle of that gap, 0.52.  With these defaults: frames 0, 2, 5 keep model 0 and suppress 36,
frames 1, 3 keep model 0 alone, frame 4 keeps 36 and suppresses model 0.  The test runs frames 0-3 (one to two
minutes); frames 4 and 5 come from the same seeded sequence, run with 6 frames.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arbitrate_calib  # noqa: E402
import arbitrate_ref as A  # noqa: E402
import view_ref as V  # noqa: E402

F = np.float32
# the tiny frame of the by-hand cases: a 32x32 float image of a wall at z = 4, 8-pixel tiles (4 x 4 of them); a
# hypothesis is a cloud of points that face the camera, one on every fourth pixel, so four per tile
HCAM = dict(fx=10.0, fy=10.0, cx=15.5, cy=15.5, depth_scale=1.0, z_min=0.5, z_max=10.0)
D = 0.1                                 # d_dist: tol = 0.1 at depth_tol 1
EYE = np.eye(4, dtype=np.float32)
ZERO = np.zeros((4, 4), np.float32)
KCAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=30.0)


def wall():
    return np.full((32, 32), 4.0, np.float32)


def cloud(cols, dz=0.0):
    """(points, normals, d_dist): points on the pixels of the tile columns `cols` (0..3), at depth 4 + dz; dz a number
    or one per tile column"""
    dzs = dict(zip(cols, dz)) if np.ndim(dz) else {c: dz for c in cols}
    pts = []
    for c in cols:
        z = 4.0 + dzs[c]
        for u in range(8 * c + 2, 8 * c + 8, 4):
            for v in range(2, 32, 4):
                pts.append([(u - 15.5) * z / 10.0, (v - 15.5) * z / 10.0, z])
    p = np.array(pts, np.float32)
    return p, np.tile(F([0, 0, -1]), (len(p), 1)), D


def run(hyps, T=None, **kw):
    kw.setdefault("tile", 8)
    T = [EYE] * len(hyps) if T is None else T
    return A.arbitrate(hyps, T, wall(), HCAM, **kw)


def test_one_hypothesis_alone_keeps_everything():
    res, kept = run([cloud([0, 1, 2, 3])])
    r = res[0]
    assert kept.tolist() == [True] and (r["claimed"], r["owned"], r["suppressed_by"], r["rounds"], r["tile"]) == (16, 16, -1, 1, 8)
    assert r["share"] == F(1) and r["mean_residual"] == F(0)
    cnt, sm, tile, _ = A.claims([cloud([0, 1, 2, 3])], [EYE], wall(), HCAM, tile=8)
    assert cnt.shape == (1, 16) and (cnt == 4).all() and (sm == 0).all()


def test_identical_hypotheses_the_higher_index_is_suppressed_by_the_lower():
    c = cloud([0, 1, 2, 3])
    res, kept = run([c, c])
    assert kept.tolist() == [True, False]
    assert res[1]["suppressed_by"] == 0 and res[1]["owned"] == 0 and res[1]["share"] == F(0)
    assert res[0]["owned"] == 16 and res[0]["share"] == F(1) and res[0]["rounds"] == 2


def test_a_hypothesis_shifted_in_depth_loses_to_the_exact_one():
    c = cloud([0, 1, 2, 3])
    Ts = EYE.copy()
    Ts[2, 3] = 0.05                          # half a tolerance behind the wall
    res, kept = run([c, c], [Ts, EYE])       # the shifted one first: the index does not decide
    assert kept.tolist() == [False, True] and res[0]["suppressed_by"] == 1
    assert res[0]["claimed"] == 16 and res[0]["owned"] == 0
    assert abs(float(res[0]["mean_residual"]) - 0.05) < 1e-4 and res[1]["mean_residual"] == F(0)
    # quantisation: r = 0.05 of tol 0.1 -> q about 65535 / 2 per point
    cnt, sm, _, _ = A.claims([c], [Ts], wall(), HCAM, tile=8)
    assert (cnt == 4).all() and (abs(sm / 4.0 - 32767.5) < 2).all()


def test_disjoint_hypotheses_are_both_kept():
    res, kept = run([cloud([0, 1]), cloud([2, 3], dz=0.08)])
    assert kept.all() and all(r["share"] == F(1) and r["claimed"] == 8 and r["suppressed_by"] == -1 for r in res)
    assert res[0]["rounds"] == 1


def test_three_way_chain_recomputes_the_share_of_the_middle_one():
    """A is exact on the left half.  W covers everything, well on the right column (0.01) and badly elsewhere (0.09).
    M covers the right half at 0.05.  Round 1: A owns its 8, M the third column, W the fourth: shares 1, 0.25, 0.5.  W is
    suppressed -- by A, which owns 8 of its tiles (M 4).  Round 2: M owns all 8 of its tiles.  With min_owned_share 0.6
    M survives only because its share is computed again."""
    a = cloud([0, 1])
    w = cloud([0, 1, 2, 3], dz=[0.09, 0.09, 0.09, 0.01])
    m = cloud([2, 3], dz=0.05)
    res, kept = run([a, w, m], min_owned_share=0.6)
    assert kept.tolist() == [True, False, True]
    assert (res[1]["claimed"], res[1]["owned"], res[1]["suppressed_by"]) == (16, 4, 0) and res[1]["share"] == F(0.25)
    assert (res[2]["claimed"], res[2]["owned"]) == (8, 8) and res[2]["share"] == F(1) and res[0]["rounds"] == 2
    one, kept1 = run([a, w, m], min_owned_share=0.2)      # nobody below 0.2: one round, the first-round shares
    assert kept1.all() and [r["share"] for r in one] == [F(1), F(0.25), F(0.5)] and one[0]["rounds"] == 1


def test_min_tiles():
    small = cloud([3])                                    # 4 tiles
    full = cloud([0, 1, 2, 3], dz=0.05)
    res, kept = run([full, small], min_tiles=5)
    # the small one takes no part: it is not kept, nobody suppressed it, and it takes no tile from the other
    assert kept.tolist() == [True, False]
    assert (res[1]["claimed"], res[1]["owned"], res[1]["suppressed_by"]) == (4, 0, -1) and res[1]["share"] == F(0)
    assert res[0]["owned"] == 16 and res[0]["share"] == F(1)
    res, kept = run([full, small], min_tiles=4)
    assert kept.tolist() == [True, True] and res[0]["owned"] == 12 and res[1]["owned"] == 4


def test_skipped_poses():
    c = cloud([0, 1, 2, 3])
    res, kept = run([c, c, c], [ZERO, EYE, ZERO])
    assert kept.tolist() == [False, True, False]
    for r in (res[0], res[2]):
        assert (r["claimed"], r["owned"], r["suppressed_by"]) == (0, 0, -1) and r["share"] == F(0) and r["mean_residual"] == F(0)
    res, kept = run([c, c], [ZERO, ZERO])
    assert not kept.any() and all(r["rounds"] == 0 and r["claimed"] == 0 for r in res)


def test_automatic_tile():
    p = F([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, -1, 0]])          # centroid (0, 0, 0)
    n = np.tile(F([0, 0, -1]), (4, 1))

    def at(z, x=0.0):
        T = EYE.copy()
        T[0, 3], T[2, 3] = x, z
        return T
    m, big = (p, n, 0.125), (p, n, 0.25)
    assert A.choose_tile([m], [at(5.25)], 525.0) == 25              # 2 * 0.125 * 525 / 5.25
    assert A.choose_tile([m], [at(5.0)], 525.0) == 27               # 26.25 -> ceil
    assert A.choose_tile([m, big], [at(5.25), at(10.5)], 525.0) == 50       # the largest d_dist, the nearest centroid
    assert A.choose_tile([m, big], [at(5.25), ZERO], 525.0) == 25           # a skipped hypothesis does not count
    assert A.choose_tile([m], [at(5.25)], 525.0, tile_spacing=3.0) == 38    # 37.5 -> ceil
    assert A.choose_tile([m], [at(100.0)], 525.0) == 4 and A.choose_tile([m], [at(0.5)], 525.0) == 128
    assert A.choose_tile([m], [at(-3.0)], 525.0) == 128             # nothing in front of the camera
    assert A.choose_tile([m], [at(5.25)], 525.0, tile=16) == 16
    res, _ = A.arbitrate([cloud([0, 1, 2, 3])], [EYE], wall(), HCAM)
    assert res[0]["tile"] == 4                                      # 2 * 0.1 * 10 / 4 = 0.5 -> clamped


def two_objects(synth, front):
    """Models 0 and 5 at their ground-truth poses before a wall: side by side, or 5 nearer and partly in front of 0."""
    out, pts, T = [], [], []
    for k, t in ((0, [-1.2, 0.0, 10.5]), (5, [2.6, 0.2, 10.5]) if not front else (5, [1.6, 0.2, 6.5])):
        mp, mn = synth.make_model(k, 1500)
        dense, _ = synth.make_model(k, 200000)
        P = np.eye(4, dtype=np.float32)
        P[:3, :3] = synth.random_rotation(synth.SplitMix64(40 + k))
        P[:3, 3] = t
        out.append((mp, mn, synth.d_dist_for(mp, 0.05)))
        pts.append(dense @ P[:3, :3].astype(np.float64).T + P[:3, 3])
        T.append(P)
    return out, T, synth.render_depth(np.concatenate(pts), background_z=20.0, splat=1)


@pytest.mark.parametrize("front", [False, True])
def test_two_real_objects_are_both_kept(synth, front):
    hyps, T, img = two_objects(synth, front)
    for (mp, mn, d), P in zip(hyps, T):
        r, _ = V.verify(mp, mn, P, img, KCAM, d)
        assert r["found"], (front, r)
    res, kept = A.arbitrate(hyps, T, img, KCAM)
    assert kept.all() and all(r["suppressed_by"] == -1 for r in res), res


def test_calibration_separates_the_present_model_from_its_twin(oracle, synth):
    rows = arbitrate_calib.table(synth, oracle, n_frames=4, min_owned_share=A.default_params()["min_owned_share"])
    print(arbitrate_calib.format_rows(rows))
    p = A.default_params()
    c = [row["spacing"][p["tile_spacing"]] for row in rows]
    both = [x for row, x in zip(rows, c) if 0 in row["found"] and arbitrate_calib.TWIN in row["found"]]
    assert all(0 in row["found"] for row in rows) and both, [row["found"] for row in rows]
    # the present model is kept wherever verification found it, the twin nowhere next to it
    assert all(0 in x["kept"] for x in c), [x["kept"] for x in c]
    assert not any(arbitrate_calib.TWIN in x["kept"] for x in c), [x["kept"] for x in c]
    # the default lies inside the measured gap of the raw first-round shares
    lo = max(float(x["twin"]["share"]) for x in both)
    hi = min(float(x["present"]["share"]) for x in c)
    assert lo < p["min_owned_share"] <= hi, (lo, hi)


def test_arbitrate_params_default(built_lib, ppf):
    p = ppf.default_arbitrate_params()
    want = A.default_params()
    assert p.depth_tol == F(want["depth_tol"]) and p.window == want["window"] and p.tile == want["tile"]
    assert p.tile_spacing == F(want["tile_spacing"]) and p.min_tiles == want["min_tiles"]
    assert p.min_owned_share == F(want["min_owned_share"]) and list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_arbitrate_params(tile=16).tile == 16
    with pytest.raises(TypeError):
        ppf.default_arbitrate_params(no_such_field=1)
    dp = ppf.default_detect_params()
    assert dp.arbitrate.min_owned_share == p.min_owned_share and dp.verify.min_supported == ppf.default_verify_params().min_supported
    assert dp.instances.max_instances == ppf.default_instance_params().max_instances and dp.instances.keep_not_found == 1
    assert dp.refine.max_iterations == ppf.default_refine_params().max_iterations
    assert ppf.ARBITRATE_MAX_HYPOTHESES == A.MAX_HYPOTHESES


def test_arbitrate_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: stand-in handles (zeroed host
    memory) are never looked at, on a machine with or without a GPU."""
    L = ppf.lib()
    bufs = [C.create_string_buffer(4096) for _ in range(4)]
    m, v, db, sc = [C.cast(b, C.c_void_p) for b in bufs]
    ms = (C.c_void_p * 2)(m, m)
    eye2 = np.stack([np.eye(4, dtype=np.float32).reshape(16)] * 2)
    res = (ppf.ArbitrateResult * 2)()
    cnt, sm = np.zeros(64, np.uint32), np.zeros(64, np.uint64)
    tile, nt = C.c_uint32(0), C.c_size_t(0)

    def call(T=eye2, params=None, mm=ms, vv=v, r=res, H=2):
        T = np.ascontiguousarray(T, np.float32)
        p = params if params is not None else ppf.default_arbitrate_params()
        return L.oslam_arbitrate(mm, ppf._p(T), H, vv, C.byref(p), r)

    def claims(T=eye2, params=None, mm=ms, vv=v, H=2, c=cnt, s=sm):
        T = np.ascontiguousarray(T, np.float32)
        p = params if params is not None else ppf.default_arbitrate_params()
        return L.oslam_arbitrate_claims(mm, ppf._p(T), H, vv, C.byref(p), ppf._p(c) if c is not None else None,
                                        ppf._p(s) if s is not None else None, 64, C.byref(tile), C.byref(nt))

    INV = ppf.OSLAM_E_INVALID
    assert call(mm=None) == INV and call(vv=None) == INV and call(r=None) == INV
    assert L.oslam_arbitrate(ms, None, 2, v, None, res) == INV
    assert call(H=0) == INV and call(H=ppf.ARBITRATE_MAX_HYPOTHESES + 1) == INV
    assert call(mm=(C.c_void_p * 2)(m, None)) == INV
    assert claims(mm=None) == INV and claims(vv=None) == INV and claims(c=None) == INV and claims(s=None) == INV
    assert claims(H=0) == INV
    bad_T = []
    T = eye2.copy(); T[1, 3] = np.nan; bad_T.append(T)
    T = eye2.copy(); T[1] = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[1, 15] = 1; bad_T.append(T)
    T = eye2.copy(); T[0, 0] = -1; bad_T.append(T)
    T = eye2.copy(); T[1, 13] = 0.5; bad_T.append(T)
    for T in bad_T:
        assert call(T) == INV and claims(T) == INV, T
    bad_p = [dict(depth_tol=0.0), dict(depth_tol=-1.0), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
             dict(window=4), dict(tile=3), dict(tile=129), dict(tile_spacing=0.0), dict(tile_spacing=float("nan")),
             dict(tile_spacing=float("inf")), dict(min_owned_share=1.5), dict(min_owned_share=-0.1),
             dict(min_owned_share=float("nan"))]
    det = (ppf.Detection * 4)()
    n = C.c_size_t(0)
    for kw in bad_p:
        p = ppf.default_arbitrate_params(**kw)
        assert call(params=p) == INV and claims(params=p) == INV, kw
        assert L.oslam_db_arbitrate(db, v, ppf._p(eye2), C.byref(p), res) == INV, kw
        dp = ppf.default_detect_params()
        dp.arbitrate = p
        assert L.oslam_db_detect(db, sc, v, C.byref(dp), det, 4, C.byref(n)) == INV, kw
    assert L.oslam_db_arbitrate(None, v, ppf._p(eye2), None, res) == INV
    assert L.oslam_db_arbitrate(db, None, ppf._p(eye2), None, res) == INV
    assert L.oslam_db_arbitrate(db, v, None, None, res) == INV
    assert L.oslam_db_arbitrate(db, v, ppf._p(eye2), None, None) == INV
    for args in ((None, sc, v, None, det, 4, C.byref(n)), (db, None, v, None, det, 4, C.byref(n)),
                 (db, sc, None, None, det, 4, C.byref(n)), (db, sc, v, None, None, 4, C.byref(n)),
                 (db, sc, v, None, det, 0, C.byref(n)), (db, sc, v, None, det, 4, None)):
        assert L.oslam_db_detect(*args) == INV, args
    for field, kw in (("verify", dict(window=9)), ("refine", dict(max_corr_dist=0.0)), ("instances", dict(max_instances=0))):
        dp = ppf.default_detect_params()
        sub = getattr(dp, field)
        for k, val in kw.items():
            setattr(sub, k, val)
        assert L.oslam_db_detect(db, sc, v, C.byref(dp), det, 4, C.byref(n)) == INV, field
    assert L.oslam_arbitrate_params_default(None) == INV and L.oslam_detect_params_default(None) == INV
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(call(params=ppf.default_arbitrate_params(tile=200)))
    assert e.value.code == INV and "tile" in str(e.value)
