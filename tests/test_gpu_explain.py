"""GPU: the explain stage (oslam_explain, oslam_db_explain and the taps oslam_explain_z, oslam_explain_claims) against
the numpy restatement (tests/explain_ref.py) on the inputs of tests/explain_edge_inputs.py, bit for bit in the solo z
images, every counter, the claims table and every result field; then the 11-member depth stream with the twin.
tests/test_explain_edge_inputs.py asserts on the CPU that the edge inputs reach their branches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explain_edge_inputs as XE  # noqa: E402
import explain_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu

INTS = ("drawn", "pixels", "agree", "occluded", "through", "unknown", "resid_sum", "conflict_q", "claimed", "owned",
        "suppressed_by", "tile", "rounds")
FLOATS = ("explained", "visible", "mean_residual", "share")
DYN = ("launches", "ms_total")
STREAM_CAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=12.0)
MEMBERS = list(range(10)) + [36]
TWIN = len(MEMBERS) - 1


def view_of(ppf, img, cam):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stable(r):
    return {k: v for k, v in r.items() if k not in DYN}


def assert_equals_ref(got, want, what):
    """every field of the device results equals the restatement: integers exactly, floats bit for bit"""
    assert len(got) == len(want), what
    for h, (g, w) in enumerate(zip(got, want)):
        for k in INTS:
            assert g[k] == w[k], (what, h, k, stable(g), w)
        assert bool(g["kept"]) == bool(w["kept"]), (what, h, stable(g), w)
        for k in FLOATS:
            assert np.float32(g[k]).tobytes() == np.float32(w[k]).tobytes(), (what, h, k, stable(g), w)


@pytest.fixture(scope="module")
def cases(synth):
    """every edge input with the restatement's answer and its taps, computed once"""
    out = []
    for c in XE.edge_cases(synth):
        taps = {}
        out.append((c, XE.reference(c, taps), taps))
    return out


def run_case(ppf, c, want, taps, z_of=(0,)):
    models = [ppf.Model(p, n, d_dist=d) for p, n, d in c["clouds"]]
    ms = [models[m] for m in c["member"]]
    view = view_of(ppf, c["img"], c["cam"])
    p = ppf.default_explain_params(**c["params"])
    got = ppf.explain(ms, view, c["T"], p)
    assert_equals_ref(got, want, c["name"])
    for h in z_of:
        z = ppf.explain_z(ms, view, c["T"], h, p)
        assert np.array_equal(bits(z), bits(taps["z"][h])), (c["name"], h, np.argwhere(bits(z) != bits(taps["z"][h]))[:6])
    cnt, sm, tile = ppf.explain_claims(ms, view, c["T"], p)
    assert tile == want[0]["tile"] and cnt.shape == taps["cnt"].shape, (c["name"], tile, cnt.shape)
    assert np.array_equal(cnt.astype(np.int64), taps["cnt"]), (c["name"], np.argwhere(cnt != taps["cnt"])[:6])
    assert np.array_equal(sm.astype(np.int64), taps["sum"]), (c["name"], np.argwhere(sm.astype(np.int64) != taps["sum"])[:6])
    view.close()
    for m in models:
        m.close()
    return got


def test_edge_inputs_equal_restatement(built_lib, ppf, cases):
    launches = {}
    for c, want, taps in cases:
        H = len(c["member"])
        got = run_case(ppf, c, want, taps, z_of=range(H) if H <= 4 else (0, 1, H // 2, H - 1))
        launches[c["name"]] = (H, {r["launches"] for r in got})
    # the cost of a call does not depend on the number of hypotheses; nothing is launched when all are skipped
    assert launches["one hypothesis"] == (1, {4}) and launches["hypotheses 1024"] == (1024, {4}), launches
    assert launches["all skipped"] == (2, {0}) and launches["see through"] == (1, {4}), launches


@pytest.mark.parametrize("H", [257, 1024])
def test_identical_hypotheses_leave_the_first(built_lib, ppf, H):
    c = XE.identical_case(H)
    models = [ppf.Model(p, n, d_dist=d) for p, n, d in c["clouds"]]
    view = view_of(ppf, c["img"], c["cam"])
    p = ppf.default_explain_params(**c["params"])
    got = ppf.explain([models[0]] * H, view, c["T"], p)
    wk, wby = XE.identical_answer(H)
    assert [bool(r["kept"]) for r in got] == wk and [r["suppressed_by"] for r in got] == wby
    assert all(r["rounds"] == H and r["launches"] == 4 for r in got)
    small = XE.identical_case(257)
    want = XE.reference(small)
    if H == 257:
        assert_equals_ref(got, want, H)
    # record 0 is the survivor's and every other one the last record's of the restatement at 257, whatever H is
    for h, g in enumerate(got):
        w = dict(want[0] if h == 0 else want[-1], rounds=H)
        assert_equals_ref([g], [w], (H, h))
    again = ppf.explain([models[0]] * H, view, c["T"], p)
    assert [stable(r) for r in again] == [stable(r) for r in got]
    view.close()
    for m in models:
        m.close()


def test_database_form_limits_and_repeats(built_lib, ppf, cases):
    c, want, taps = [x for x in cases if x[0]["name"].startswith("sizes")][0]
    models = [ppf.Model(p, n, d_dist=d) for p, n, d in c["clouds"]]
    view = view_of(ppf, c["img"], c["cam"])
    p = ppf.default_explain_params(**c["params"])
    db = ppf.Database(models)
    a = ppf.explain(models, view, c["T"], p)
    b = db.explain(view, c["T"], p)
    assert [stable(r) for r in a] == [stable(r) for r in b]
    assert_equals_ref(b, want, "database")
    # the order of the hypotheses only renames them
    rev = ppf.explain(models[::-1], view, c["T"][::-1], p)
    for g, w in zip(rev[::-1], a):
        assert all(g[k] == w[k] for k in INTS[:8]) and all(bits(g[k]) == bits(w[k]) for k in FLOATS[:3]), (g, w)
    H = X.MAX_HYPOTHESES + 1
    with pytest.raises(ppf.OslamError) as e:
        ppf.explain([models[0]] * H, view, np.repeat(c["T"][:1], H, axis=0), p)
    assert e.value.code == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        ppf.explain_z(models, view, c["T"], 3, p)
    assert e.value.code == ppf.OSLAM_E_INVALID
    ok = ppf.explain(models, view, c["T"], p)
    assert [stable(r) for r in ok] == [stable(r) for r in a]      # the rejected calls left the stage usable
    db.close()
    view.close()
    for m in models:
        m.close()


def test_depth_stream_the_present_model_survives_its_twin(built_lib, ppf, synth):
    """The 10-frame depth stream of seed 93 (model 0 before a wall at 9 m) with 11 members: models 0..9 and 36, the near
    twin of model 0 that verification alone confirms next to it.  db.align -> db.refine -> db.verify -> db.explain over
    the members verification found; oslam_arbitrate loses model 0 on frame 8 of this stream.

    Asserted: the device equals the restatement on the device's own poses; wherever 0 and 36 are both verified exactly
    one of them survives; model 0 is kept wherever it is verified alone; model 0 is lost on at most a quarter of the
    contested frames (the cap of the arbitration's stream test: a condition, not a measurement).

    The restatement over these ten frames on the CPU, with the oracle's voting poses refined by tests/refine_ref.py and
    verified by tests/view_ref.py (members 0 and 36; 1..9 are verified on no calibration frame): 8 contested frames (0, 2,
    3, 5, 6, 7, 8, 9), model 0 lost on 0 of them and kept alone on frames 1 and 4.  Conflict rates of model 0 / member 36
    on the contested frames: 0.077/0.111, 0.093/0.125, 0.130/0.174, 0.092/0.118, 0.103/0.134, 0.199/0.241, 0.261/0.286,
    0.248/0.299; the twin's first-round share is at most 0.079.  (At depth_tol 0.5 frame 8 turns: 0.473 against 0.450,
    and model 0 is lost there, 1 of 8.)  tests/arbitrate_ref.py on the same poses loses model 0 on frame 8.

    Measured on one MI355X with the device's own poses: the same 8 contested frames, model 0 kept on all of them and alone
    on frames 1 and 4, the conflict rates above to the digits printed, the twin's first-round share at most 0.079."""
    frames = 10
    raw = [synth.make_model(k, 1500) for k in MEMBERS]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    clouds = [(g[0], g[1], d) for g in grids]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)
    contested, lost0, table = 0, [], []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        img = synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1)
        sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                  z_min=0.5, z_max=12.0, max_jump=0.08)
        view = view_of(ppf, img, STREAM_CAM)
        Ta, _ = db.align(sc)
        Tr, _, _ = db.refine(sc, Ta)
        _, found = db.verify(view, Tr)
        Tf = np.where(found[:, None, None], Tr, np.float32(0))
        res = db.explain(view, Tf)
        kept = np.array([bool(r["kept"]) for r in res])
        assert_equals_ref(res, X.explain(clouds, Tf, img, STREAM_CAM), f)
        table.append((f, [int(j) for j in np.flatnonzero(found)], [int(j) for j in np.flatnonzero(kept)],
                      res[0]["conflict_q"] / 65535.0, res[TWIN]["conflict_q"] / 65535.0, res[0]["share"], res[TWIN]["share"]))
        assert not (kept & ~found).any() and all(r["launches"] == (4 if found.any() else 0) for r in res)
        if found[0] and found[TWIN]:
            contested += 1
            assert kept[0] != kept[TWIN], (f, stable(res[0]), stable(res[TWIN]))       # exactly one of the two survives
            if not kept[0]:
                lost0.append(f)
        elif found[0]:
            assert kept[0], (f, stable(res[0]))                                        # verified alone: kept
        view.close()
        sc.close()
    db.close()
    for m in models:
        m.close()
    for row in table:
        print("frame %d found %s kept %s conflict 0: %.3f twin: %.3f share 0: %.3f twin: %.3f" % row)
    assert contested >= 1 and len(lost0) <= -(-contested // 4), (lost0, contested, table)
