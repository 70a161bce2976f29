"""GPU: the view kernels (k_view_z, k_verify, k_claim, k_arbitrate, k_view_normals, k_track, k_track_corr) and the front
end (k_vox_bbox's strided path, oslam_depth_to_cloud) on the inputs of tests/edge_inputs.py against the numpy
restatements: ragged images with points on and outside every border, model sizes around the wave and block sizes,
poses that overflow the projection, 255..1024 and identical hypotheses, and claims tables with exact ties through the
table tap (oslam_arbitrate_table).  tests/test_edge_inputs.py asserts on the CPU that these inputs reach their
branches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arbitrate_ref as A  # noqa: E402
import edge_inputs as E  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402
import view_ref as V  # noqa: E402
from test_gpu_arbitrate import assert_equals_ref, stable  # noqa: E402
from test_gpu_track import plain  # noqa: E402

pytestmark = pytest.mark.gpu


def view_of(ppf, img, cam, max_jump=E.MAX_JUMP):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=max_jump)


def assert_maps_equal(ppf, oracle, view, img, cam, max_jump):
    vtx, nrm, has = ppf.view_normals(view)
    Vr, Nr, ok = K.view_maps(img, cam, max_jump)
    assert np.array_equal(ok, has), np.argwhere(ok != has)[:6]
    assert np.array_equal(Vr.view(np.uint32), vtx.view(np.uint32)) and np.array_equal(Nr.view(np.uint32), nrm.view(np.uint32))
    assert not vtx[~has].any() and not nrm[~has].any()
    h, w = img.shape
    if h >= 3 and w >= 3:
        kw = dict(depth_scale=cam["depth_scale"], z_min=cam["z_min"], z_max=cam["z_max"], max_jump=max_jump)
        cp, cn = ppf.depth_to_cloud(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], **kw)
        op, on = oracle.depth_to_cloud(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], **kw)
        assert len(cp) == len(op) == int(has.sum())
        for a, b in ((cp, vtx[has]), (cn, nrm[has]), (op, cp), (on, cn)):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    return (Vr, Nr, ok)


def assert_model_on_view(ppf, model, mp, mn, d, view, img, cam, maps, poses, windows=range(4), tiles=(4, 7, 128, 0)):
    """every exact comparison of one model against one view: classes, counts, claims, correspondences"""
    total = np.zeros(6, np.int64)
    for name, T in poses.items():
        for window in windows:
            p = ppf.default_verify_params(window=window)
            got = ppf.verify_classes(model, view, T, p)
            want = E.ref_classes(mp, mn, T, img, cam, d, window)
            assert np.array_equal(got, want), (name, window, img.dtype, np.flatnonzero(got != want)[:8])
            r = model.verify(view, T, p)
            hist = np.bincount(got, minlength=6)
            assert [r[k] for k in V.NAMES] == list(hist) and int(hist.sum()) == len(mp), (name, window, r, hist)
            total += hist
        got = ppf.track_correspondences(model, view, T, 2.0, 0.8)
        with np.errstate(all="ignore"):
            want, _, _ = K.correspondences(mp, mn, T, maps, cam, np.float32(2.0) * np.float32(d), 0.8)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
    names = list(poses)
    Ts = np.stack([poses[n] for n in names]).astype(np.float32)
    for tile in tiles:
        for window in (0, 1, 3):
            p = ppf.default_arbitrate_params(window=window, tile=tile)
            cnt, sm, used = ppf.arbitrate_claims([model] * len(names), view, Ts, p)
            with np.errstate(all="ignore"):
                wc, ws, wt, _ = A.claims([(mp, mn, d)] * len(names), Ts, img, cam, window=window, tile=tile)
            assert used == wt and cnt.shape == wc.shape, (tile, window, used, wt, cnt.shape, wc.shape)
            assert np.array_equal(cnt.astype(np.int64), wc), (tile, window, np.argwhere(cnt != wc)[:6])
            assert np.array_equal(sm.astype(np.int64), ws), (tile, window, np.argwhere(sm.astype(np.int64) != ws)[:6])
    return total


@pytest.mark.parametrize("h,w", E.SHAPES)
def test_image_shapes_equal_restatement(built_lib, ppf, synth, oracle, h, w):
    c = E.shape_case(h, w, synth)
    model = ppf.Model(c["mp"], c["mn"], d_dist=c["d"])
    total = np.zeros(6, np.int64)
    for img, cam in ((c["img"], c["cam"]), (c["fimg"], c["fcam"])):
        view = view_of(ppf, img, cam)
        maps = assert_maps_equal(ppf, oracle, view, img, cam, E.MAX_JUMP)
        total += assert_model_on_view(ppf, model, c["mp"], c["mn"], c["d"], view, img, cam, maps, c["poses"])
        view.close()
    model.close()
    assert total[V.SUPPORTED] > 0 and total[V.OUT] > 0, total


def test_model_sizes_equal_restatement(built_lib, ppf, synth, oracle):
    c = E.size_case(synth)
    poses = {"truth": c["truth"], "previous": c["previous"]}
    with pytest.raises(ppf.OslamError):             # a model needs two points: size 1 exists for the restatement only
        ppf.Model(c["mp"][:1], c["mn"][:1], d_dist=c["d"])
    stopped = stepped = 0
    for fname, (img, cam) in c["frames"].items():
        view = view_of(ppf, img, cam, K.STREAM_MAX_JUMP)
        maps = assert_maps_equal(ppf, oracle, view, img, cam, K.STREAM_MAX_JUMP)
        for n in E.MODEL_SIZES[1:]:
            mp, mn = c["mp"][:n], c["mn"][:n]
            model = ppf.Model(mp, mn, d_dist=c["d"])
            assert_model_on_view(ppf, model, mp, mn, c["d"], view, img, cam, maps, poses, windows=(0, 1, 3), tiles=(7, 0))
            T1, res, found = ppf.track([model], view, c["previous"][None])
            W64, w64 = K.track(mp, mn, c["previous"], img, cam, c["d"], K.STREAM_MAX_JUMP, maps=maps)
            ver = model.verify(view, T1[0])
            assert plain(res[0]["verify"]) == plain(ver) and bool(found[0]) == bool(ver["found"]), (fname, n)
            if w64["correspondences"] < 6 and w64["iterations"] == 0:
                # fewer than 6 correspondences stop the step: the pose comes back bit for bit
                assert res[0]["iterations"] == 0 and res[0]["correspondences"] == w64["correspondences"], (fname, n, res[0], w64)
                assert T1[0].tobytes() == np.asarray(c["previous"], np.float32).tobytes(), (fname, n)
                stopped += w64["correspondences"] >= 1
                model.close()
                continue
            W32, _ = K.track(mp, mn, c["previous"], img, cam, c["d"], K.STREAM_MAX_JUMP, maps=maps, sums="f32")
            s_ang, s_dt = refine_ref.pose_error(W32, W64)
            ang, dt = refine_ref.pose_error(T1[0], W64)
            b_ang, b_dt = max(0.01, 8.0 * s_ang), max(1e-3 * c["d"], 8.0 * s_dt)
            print("%s n %4d: device vs float64 sums %.3e deg %.3e d_dist; spread of the restatement (float32 index order vs "
                  "float64) %.3e deg %.3e d_dist; bound %.3e deg %.3e d_dist; iterations %d / %d; correspondences %d / %d; "
                  "cond %.3e" % (fname, n, ang, dt / c["d"], s_ang, s_dt / c["d"], b_ang, b_dt / c["d"], res[0]["iterations"],
                                 w64["iterations"], res[0]["correspondences"], w64["correspondences"], w64["cond"]))
            assert abs(res[0]["iterations"] - w64["iterations"]) <= 1, (fname, n, res[0], w64)
            assert ang <= b_ang and dt <= b_dt, (fname, n, ang, dt / c["d"], b_ang, b_dt / c["d"], w64["cond"])
            stepped += 1
            model.close()
        view.close()
    assert stopped >= 1 and stepped >= 8, (stopped, stepped)


def test_poses_that_overflow_the_projection(built_lib, ppf, synth):
    """Translations of 1e30 and 3e38 and p'z exactly on z_min and z_max: the pixel is range-checked in float before it
    becomes an int, so these are OUT (or in view, on the limits) and nothing is read outside the image."""
    h, w = 61, 83
    c = E.shape_case(h, w, synth)
    cam = c["cam"]
    mp, mn = c["mp"].copy(), c["mn"].copy()
    mp[:40, 2] = 0.0                                  # with the poses below p'z is exactly the translation's z
    mp[:40, :2] *= np.float32(0.2)
    mn[:40] = [0.0, 0.0, -1.0]
    model = ppf.Model(mp, mn, d_dist=c["d"])
    poses = {}
    for name, t in (("x 1e30", (1e30, 0, 2)), ("x -1e30", (-1e30, 0, 2)), ("y 3e38", (0, 3e38, 2)), ("z 1e30", (0, 0, 1e30)),
                    ("z 3e38", (0, 0, 3e38)), ("z -3e38", (0, 0, -3e38)), ("xyz 3e38", (3e38, -3e38, 3e38)),
                    ("z_min", (0, 0, cam["z_min"])), ("z_max", (0, 0, cam["z_max"])),
                    ("below z_min", (0, 0, float(np.nextafter(np.float32(cam["z_min"]), np.float32(0))))),
                    ("above z_max", (0, 0, float(np.nextafter(np.float32(cam["z_max"]), np.float32(99)))))):
        poses[name] = E.rigid(t=t)
    tilt = E.border_poses(h, w)["tilt"].copy()
    tilt[:3, 3] = [3e38, 1e30, -1e30]
    poses["tilt 3e38"] = tilt
    view = view_of(ppf, c["img"], cam)
    maps = K.view_maps(c["img"], cam, E.MAX_JUMP)
    assert_model_on_view(ppf, model, mp, mn, c["d"], view, c["img"], cam, maps, poses)
    for name, T in poses.items():
        cls = ppf.verify_classes(model, view, T)
        pix = ppf.track_correspondences(model, view, T, 2.0, 0.8)
        if "e3" in name:
            assert np.isin(cls, (V.BACK, V.OUT)).all() and (cls == V.OUT).any() and (pix == -1).all(), (name, np.bincount(cls))
        elif name in ("z_min", "z_max"):
            assert (cls[:40] >= V.SUPPORTED).any(), (name, cls[:40])
        else:
            assert (cls[:40] == V.OUT).all(), (name, cls[:40])
        T1, res, found = ppf.track([model], view, T[None])
        if "e3" in name:
            assert res[0]["iterations"] == 0 and res[0]["correspondences"] == 0 and T1[0].tobytes() == T.tobytes() and not found[0]
    view.close()
    model.close()


@pytest.fixture(scope="module")
def many_models(ppf, synth):
    clouds = [synth.make_model(k, 300) for k in E.MANY_MODELS]
    d = synth.d_dist_for(clouds[0][0], 0.05)
    models = [ppf.Model(p, n, d_dist=d) for p, n in clouds]
    yield models
    for m in models:
        m.close()


@pytest.mark.parametrize("key,H", [("96x64/16", 255), ("96x64/16", 256), ("96x64/16", 257), ("160x32/32", 1024), ("192x32/32", 1024)])
def test_many_hypotheses_equal_restatement(built_lib, ppf, synth, many_models, key, H):
    c = E.many_case(synth, key, H)
    view = view_of(ppf, c["img"], c["cam"], K.STREAM_MAX_JUMP)
    models = [many_models[m] for m in c["mem"]]
    p = ppf.default_arbitrate_params(tile=c["tile"], **E.MANY_PARAMS)
    got, kept = ppf.arbitrate(models, view, c["T"], p)
    assert_equals_ref(got, c["want"], (key, H))
    assert np.array_equal(kept, c["kept"]) and all(r["launches"] == 2 for r in got)
    if H == 1024:                                     # the same call once more
        again, kept2 = ppf.arbitrate(models, view, c["T"], p)
        assert np.array_equal(kept, kept2) and [stable(r) for r in again] == [stable(r) for r in got]
    # The database form: member j = hypothesis j.  A database cannot hold one handle twice, so this block takes the three
    # reused models with the first live pose of each: it does not depend on H and is no 1024-hypothesis coverage of
    # oslam_db_arbitrate, which shares arbitrate_members with oslam_arbitrate after its argument checks.
    db = ppf.Database(many_models)
    first = [int(np.flatnonzero((c["mem"] == j) & c["T"].any(axis=(1, 2)))[0]) for j in range(3)]
    Td = np.stack([c["T"][i] for i in first])
    a, ka = ppf.arbitrate(many_models, view, Td, p)
    e, ke = db.arbitrate(view, Td, p)
    assert np.array_equal(ka, ke) and [stable(r) for r in a] == [stable(r) for r in e]
    want, _ = A.arbitrate(c["clouds"], Td, c["img"], c["cam"], tile=c["tile"], **E.MANY_PARAMS)
    assert_equals_ref(a, want, (key, "db"))
    if H == 1024:
        # k_track with 1024 workgroups: every entry equals the single call of its (model, pose)
        t = ppf.track(models, view, c["T"])
        t2 = ppf.track(models, view, c["T"])
        assert np.array_equal(t[0], t2[0]) and [plain(r) for r in t[1]] == [plain(r) for r in t2[1]] and np.array_equal(t[2], t2[2])
        assert all(r["launches"] == 1 for r in t2[1])
        dbt = db.track(view, c["mem"], c["T"])
        assert np.array_equal(dbt[0], t[0]) and [plain(r) for r in dbt[1]] == [plain(r) for r in t[1]]
        single, first_at = {}, {}
        for i in range(H):
            if not c["T"][i].any():
                assert not t[0][i].any() and not t[2][i] and t[1][i]["iterations"] == 0 and t[1][i]["verify"]["supported"] == 0
                continue
            k = (int(c["mem"][i]), c["T"][i].tobytes())
            if k not in single:                       # one single call per distinct (model, pose); duplicates share it
                s = ppf.track([models[i]], view, c["T"][i][None])
                assert s[1][0]["launches"] == 1
                single[k], first_at[k] = (s[0][0], plain(s[1][0]), bool(s[2][0])), i
            assert t[0][i].tobytes() == single[k][0].tobytes() and plain(t[1][i]) == single[k][1], (i, first_at[k])
            assert bool(t[2][i]) == single[k][2], i
        assert len(single) > 100 and sum(i >= 256 for i in first_at.values()) > 20, (len(single), sorted(first_at.values())[-5:])
        assert any(r["iterations"] >= 1 for r in t[1][256:])
    db.close()
    view.close()


@pytest.mark.parametrize("H", [257, 1024])
def test_identical_hypotheses_leave_one(built_lib, ppf, synth, many_models, H):
    sc = E.many_scene(synth, "96x64/16")
    view = view_of(ppf, sc["img"], sc["cam"])
    T = np.repeat(sc["TA"][None], H, axis=0)
    p = ppf.default_arbitrate_params(tile=sc["tile"], **E.MANY_PARAMS)
    got, kept = ppf.arbitrate([many_models[0]] * H, view, T, p)
    wk, wby = E.identical_answer(H)
    assert kept.tolist() == wk and [r["suppressed_by"] for r in got] == wby
    assert all(r["rounds"] == H and r["launches"] == 2 for r in got)
    assert got[0]["owned"] == got[0]["claimed"] >= 1 and all(r["owned"] == 0 and r["claimed"] == got[0]["claimed"] for r in got[1:])
    want = E.identical_case(synth, 257)["want"]
    if H == 257:
        assert_equals_ref(got, want, H)
    # H copies of one hypothesis: record 0 is the survivor's and every other one the last record's of the restatement at
    # 257, whatever H is (claims, share and mean residual do not depend on the number of copies)
    for h, g in enumerate(got):
        w = want[0] if h == 0 else want[-1]
        for k in ("claimed", "owned"):
            assert g[k] == w[k], (h, k, g, w)
        for k in ("share", "mean_residual"):
            assert np.float32(g[k]).tobytes() == np.float32(w[k]).tobytes(), (h, k, g, w)
    again, kept2 = ppf.arbitrate([many_models[0]] * H, view, T, p)
    assert np.array_equal(kept, kept2) and [stable(r) for r in again] == [stable(r) for r in got]
    view.close()


def test_more_than_1024_hypotheses_are_rejected(built_lib, ppf, synth, many_models):
    """The same limit inside oslam_db_detect needs more than 1024 real instances in one frame and stays untested.
    oslam_db_arbitrate takes one hypothesis per member and a database refuses a repeated handle, so its case is a
    database of 1025 two-point models."""
    sc = E.many_scene(synth, "96x64/16")
    view = view_of(ppf, sc["img"], sc["cam"])
    H = A.MAX_HYPOTHESES + 1
    T = np.repeat(sc["TA"][None], H, axis=0)
    db = ppf.Database(many_models)
    for call in (lambda: ppf.arbitrate([many_models[0]] * H, view, T), lambda: ppf.track([many_models[0]] * H, view, T),
                 lambda: db.track(view, np.zeros(H, np.uint32), T),
                 lambda: ppf.arbitrate_table(np.ones((H, 2), np.uint32), np.ones((H, 2), np.uint64))):
        with pytest.raises(ppf.OslamError) as e:
            call()
        assert e.value.code == ppf.OSLAM_E_INVALID
    db.close()
    mp, mn = synth.make_model(0, 2)
    tiny = [ppf.Model(mp, mn, d_dist=sc["d"]) for _ in range(H)]
    big = ppf.Database(tiny)
    with pytest.raises(ppf.OslamError) as e:
        big.arbitrate(view, T)
    assert e.value.code == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        big.track(view, np.arange(H), T)
    assert e.value.code == ppf.OSLAM_E_INVALID
    res, kept = ppf.arbitrate(tiny[:A.MAX_HYPOTHESES], view, T[:A.MAX_HYPOTHESES])
    assert len(res) == A.MAX_HYPOTHESES and all(r["launches"] == 2 for r in res)      # 1024 distinct handles are taken
    big.close()
    for m in tiny:
        m.close()
    ok, _ = ppf.arbitrate([many_models[0]] * 2, view, T[:2])
    assert ok[0]["launches"] == 2                     # the rejected calls left the stage usable
    view.close()


def assert_table_equals(ppf, name, cnt, sm, skipped, min_tiles, share):
    got, rounds = ppf.arbitrate_table(cnt, sm, skipped, min_tiles, share)
    want, wr = E.eliminate_table(cnt, sm, skipped, min_tiles, share)
    assert rounds == wr, (name, rounds, wr)
    for r in want:
        r["tile"], r["rounds"] = 0, wr
    assert_equals_ref(got, want, name)
    live = any(not s for s in skipped) if skipped is not None else True
    assert all(r["launches"] == (1 if live else 0) for r in got), name
    return got


def test_table_tap_ties_and_large_counts(built_lib, ppf):
    for name, (cnt, sm, sk, mt, share) in E.tie_tables().items():
        got = assert_table_equals(ppf, name, cnt, sm, sk, mt, share)
        again, _ = ppf.arbitrate_table(cnt, sm, sk, mt, share)
        assert [stable(r) for r in again] == [stable(r) for r in got], name
    got, rounds = ppf.arbitrate_table(np.ones((3, 2), np.uint32), np.ones((3, 2), np.uint64), np.ones(3, bool))
    assert rounds == 0 and all(r["launches"] == 0 and not r["kept"] and r["suppressed_by"] == -1 for r in got)
    # the argument checks of oslam_arbitrate
    one = np.ones((2, 2), np.uint32)
    for bad in (lambda: ppf.arbitrate_table(one, one.astype(np.uint64), None, 1, 1.5),
                lambda: ppf.arbitrate_table(one, one.astype(np.uint64), None, 1, float("nan")),
                lambda: ppf.arbitrate_table(one * (1 << 24), one.astype(np.uint64)),
                lambda: ppf.arbitrate_table(one, one.astype(np.uint64) << np.uint64(40)),
                lambda: ppf.arbitrate_table(np.zeros((0, 2), np.uint32), np.zeros((0, 2), np.uint64)),
                lambda: ppf.arbitrate_table(np.zeros((2, 0), np.uint32), np.zeros((2, 0), np.uint64))):
        with pytest.raises(ppf.OslamError) as e:
            bad()
        assert e.value.code == ppf.OSLAM_E_INVALID


def test_table_tap_random_sweep(built_lib, ppf):
    suppressed = ties = 0
    for k, (cnt, sm, sk, mt, share) in enumerate(E.random_tables()):
        got = assert_table_equals(ppf, ("random", k, cnt.shape), cnt, sm, sk, mt, share)
        suppressed += sum(r["suppressed_by"] >= 0 for r in got)
        shares = [r["share"] for r in got if r["claimed"]]
        ties += len(shares) - len(set(shares))
    assert suppressed > 200 and ties > 200, (suppressed, ties)


def test_voxel_grid_at_the_strided_sizes(built_lib, ppf, oracle, synth):
    for name, (pts, nrm, leaf) in E.voxel_cases(synth).items():
        go, gn = ppf.voxel_grid(pts, nrm, leaf=leaf)
        oo, on = oracle.voxel_grid(pts, nrm, leaf)
        assert len(go) == len(oo), (name, len(go), len(oo))
        assert np.array_equal(go.view(np.uint32), oo.view(np.uint32)) and np.array_equal(gn.view(np.uint32), on.view(np.uint32)), name
        if name == "none finite":
            assert len(go) == 0
        elif name in ("one voxel", "one point"):
            assert len(go) == 1
        else:
            assert 1 < len(go) <= len(pts), (name, len(go))


@pytest.mark.parametrize("h,w", [s for s in E.SHAPES if min(s) >= 3] + [(480, 640)])
def test_depth_to_cloud_at_ragged_shapes(built_lib, ppf, oracle, h, w):
    cam = E.cam_of(h, w)
    for img, scale in zip(E.images_of(h, w), (0.001, 1.0)):
        kw = dict(depth_scale=scale, z_min=cam["z_min"], z_max=cam["z_max"], max_jump=E.MAX_JUMP)
        cp, cn = ppf.depth_to_cloud(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], **kw)
        op, on = oracle.depth_to_cloud(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], **kw)
        assert len(cp) == len(op) and (len(cp) > 0 or img.dtype != np.uint16)
        assert np.array_equal(cp.view(np.uint32), op.view(np.uint32)) and np.array_equal(cn.view(np.uint32), on.view(np.uint32))
