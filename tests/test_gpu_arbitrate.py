"""GPU: the arbitration stage (oslam_arbitrate, oslam_db_arbitrate, oslam_arbitrate_claims, oslam_db_detect) against the
numpy restatement of tests/arbitrate_ref.py, the twin member on the depth stream, several copies of one model, and the
one-call chain against the manual one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arbitrate_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

DYN = ("launches", "ms_total")
KCAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=30.0)
WALL = 20.0
STREAM_CAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=12.0)
MEMBERS = list(range(10)) + [36]
TWIN = len(MEMBERS) - 1


def view_of(ppf, img, cam):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"])


def moved(T, dx=0.0, dy=0.0, dz=0.0):
    T = T.copy()
    T[:3, 3] += np.float32([dx, dy, dz])
    return T


def stable(r):
    return {k: v for k, v in r.items() if k not in DYN}


def assert_equals_ref(got, want, what):
    """every field of the device results equals the restatement: integers exactly, floats bit for bit"""
    for h, (g, w) in enumerate(zip(got, want)):
        for k in ("claimed", "owned", "suppressed_by", "tile", "rounds"):
            assert g[k] == w[k], (what, h, k, g, w)
        assert bool(g["kept"]) == bool(w["kept"]), (what, h, g, w)
        for k in ("share", "mean_residual"):
            assert np.float32(g[k]).tobytes() == np.float32(w[k]).tobytes(), (what, h, k, g, w)


@pytest.fixture(scope="module")
def frame(ppf, synth):
    """The frame of tests/test_gpu_verify.py, rebuilt: model 0 (1500 points) at 10.5 m before a wall at 20 m, its
    voting and refined poses and the poses of the known-answer cases; and model 36, its near twin."""
    mp, mn = synth.make_model(0, 1500)
    d = synth.d_dist_for(mp, 0.05)
    ext = synth.bbox_extent(mp)
    dense, _ = synth.make_model(0, 200000)
    rng = synth.SplitMix64(77)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth.random_rotation(rng)
    T[:3, 3] = [0.3, -0.2, 10.5]
    img = synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=WALL, splat=1)
    model = ppf.Model(mp, mn, d_dist=d)
    tp, tn = synth.make_model(36, 1200)
    twin = ppf.Model(tp, tn, d_dist=d)
    sc = ppf.Scene.from_depth(img, KCAM["fx"], KCAM["fy"], KCAM["cx"], KCAM["cy"], leaf=d, d_dist=d,
                              ref_point_downsample_factor=4, z_min=KCAM["z_min"], z_max=KCAM["z_max"], max_jump=0.08)
    Tv = model.ppf_lookup(sc).copy()
    Tr, _ = model.refine(sc, Tv)
    poses = {"truth": T, "vote": Tv, "refined": Tr, "toward": moved(T, dz=-2.0 * ext),
             "behind": moved(T, dz=WALL + ext - T[2, 3]), "right": moved(T, dx=50.0), "far": moved(T, dz=40.0),
             "half_out": moved(T, dx=6.0), "nudged": moved(T, dz=0.4 * d)}
    yield dict(mp=mp, mn=mn, tp=tp, tn=tn, d=d, img=img, model=model, twin=twin, poses=poses)
    sc.close()
    twin.close()
    model.close()


def hypotheses(c):
    """every pose of the frame with model 0, then some with the twin, and a skipped one in the middle"""
    names = list(c["poses"])
    models = [c["model"]] * len(names) + [c["twin"]] * 3
    clouds = [(c["mp"], c["mn"], c["d"])] * len(names) + [(c["tp"], c["tn"], c["d"])] * 3
    T = [c["poses"][n] for n in names] + [c["poses"]["truth"], np.zeros((4, 4), np.float32), c["poses"]["refined"]]
    return models, clouds, np.stack(T).astype(np.float32)


def test_claims_equal_restatement(built_lib, ppf, frame):
    c = frame
    fimg = c["img"].astype(np.float32) * np.float32(0.001)
    fimg[::7, ::5] = np.nan
    fimg[3::11, ::3] = -1.0
    fimg[5::13, 1::4] = np.inf
    fcam = dict(KCAM, depth_scale=1.0)
    models, clouds, T = hypotheses(c)
    total = 0
    for img, cam in ((c["img"], KCAM), (fimg, fcam)):
        view = view_of(ppf, img, cam)
        for window in range(4):
            for tile in (0, 4, 7, 32, 128):
                p = ppf.default_arbitrate_params(window=window, tile=tile)
                cnt, sm, used = ppf.arbitrate_claims(models, view, T, p)
                wc, ws, wt, _ = A.claims(clouds, T, img, cam, window=window, tile=tile)
                assert used == wt and cnt.shape == wc.shape, (window, tile, used, wt)
                assert np.array_equal(cnt.astype(np.int64), wc), (img.dtype, window, tile, np.argwhere(cnt != wc)[:6])
                assert np.array_equal(sm.astype(np.int64), ws), (img.dtype, window, tile, np.argwhere(sm.astype(np.int64) != ws)[:6])
                total += int(wc.sum())
        cnt, sm, used = ppf.arbitrate_claims(models, view, T, ppf.default_arbitrate_params(depth_tol=0.25, tile_spacing=3.0))
        wc, ws, wt, _ = A.claims(clouds, T, img, cam, depth_tol=0.25, tile_spacing=3.0)
        assert used == wt and np.array_equal(cnt.astype(np.int64), wc) and np.array_equal(sm.astype(np.int64), ws)
        view.close()
    assert total > 10000      # the claims are there: the comparison is not of empty tables


def test_results_equal_restatement(built_lib, ppf, frame):
    c = frame
    models, clouds, T = hypotheses(c)
    view = view_of(ppf, c["img"], KCAM)
    suppressed = 0
    for kw in (dict(), dict(tile=8), dict(tile=64, min_owned_share=0.9), dict(window=0, min_tiles=1, min_owned_share=0.3),
               dict(tile_spacing=1.0, min_owned_share=1.0), dict(min_owned_share=0.0), dict(min_tiles=100000)):
        got, kept = ppf.arbitrate(models, view, T, ppf.default_arbitrate_params(**kw))
        want, wkept = A.arbitrate(clouds, T, c["img"], KCAM, **kw)
        assert_equals_ref(got, want, kw)
        assert np.array_equal(kept, wkept)
        assert all(r["launches"] == 2 for r in got)
        suppressed += sum(r["suppressed_by"] >= 0 for r in got)
    assert suppressed > 0
    # the exact pose against its copy nudged by 0.4 d_dist in depth, in both orders: the exact one survives
    P = c["poses"]
    for Ts, want in (([P["nudged"], P["truth"]], [False, True]), ([P["truth"], P["nudged"]], [True, False])):
        got, kept = ppf.arbitrate([c["model"]] * 2, view, np.stack(Ts))
        assert kept.tolist() == want and got[want.index(False)]["suppressed_by"] == want.index(True), got
    # poses without a SUPPORTED point claim nothing and are never kept
    names = list(P)
    got, kept = ppf.arbitrate(models, view, T)
    assert kept.any() and not any(kept[names.index(n)] for n in ("toward", "behind", "right", "far", "half_out")), got
    view.close()


def test_launches_do_not_depend_on_hypotheses_and_results_repeat(built_lib, ppf, synth, frame):
    c = frame
    clouds = [synth.make_model(k, 300) for k in range(50)]
    d = synth.d_dist_for(clouds[0][0], 0.05)
    models = [ppf.Model(p, n, d_dist=d) for p, n in clouds]
    view = view_of(ppf, c["img"], KCAM)
    rng = synth.SplitMix64(9)
    T = np.zeros((50, 4, 4), np.float32)
    for j in range(50):
        T[j] = np.eye(4)
        T[j, :3, :3] = synth.random_rotation(rng)
        T[j, :3, 3] = [0.3, -0.2, 10.5 + 0.02 * j]
    launches = []
    for n in (2, 50):
        a, ka = ppf.arbitrate(models[:n], view, T[:n])
        b, kb = ppf.arbitrate(models[:n], view, T[:n])
        assert np.array_equal(ka, kb) and [stable(r) for r in a] == [stable(r) for r in b]
        assert all(r["launches"] == a[0]["launches"] for r in a)
        want, _ = A.arbitrate([(p, q, d) for p, q in clouds[:n]], T[:n], c["img"], KCAM)
        assert_equals_ref(a, want, n)
        launches.append(a[0]["launches"])
        # the database form: member j = hypothesis j of the same list
        db = ppf.Database(models[:n])
        e, ke = db.arbitrate(view, T[:n])
        assert np.array_equal(ka, ke) and [stable(r) for r in a] == [stable(r) for r in e]
        db.close()
    assert launches == [2, 2]
    z, kz = ppf.arbitrate(models[:3], view, np.zeros((3, 4, 4), np.float32))
    assert not kz.any() and all(r["launches"] == 0 and r["claimed"] == 0 and r["suppressed_by"] == -1 for r in z)
    view.close()
    for m in models:
        m.close()


def test_depth_stream_twin_is_suppressed(built_lib, ppf, synth):
    """The depth stream of tests/test_gpu_verify.py (10 frames of seed 93) with 11 members: models 0..9 and 36, the near
    twin of model 0 that verification alone confirms next to it.  db.align -> db.refine -> db.verify -> db.arbitrate
    over the members verification found.

    What is asserted is what the CPU calibration table supports (docstring of tests/test_arbitrate_host.py, measured
    before this stream was run).  No setting separates model 0 from 36 on all six calibration frames, so "model 0 kept
    in every frame, 36 in none" is not supported.  Supported, at tile_spacing 2 and min_owned_share 0.52:
      - where both are verified (calibration frames 0, 2, 4, 5) exactly one of the two survives: the loser's first-round
        share is 0.343-0.421, below 0.52, on all four; here: never both kept, and the survivor suppressed the other;
      - where model 0 is verified alone (frames 1, 3) it is kept;
      - model 0 is the survivor on 3 of the 4 contested frames; on frame 4 its ICP pose ends 4.0 degrees from the truth
        (the twin's 0.9) and the twin survives; here: model 0 is lost on at most ceil(contested / 4) frames.
    Verification's own bar (model 0 found in at least 9 of 10) and "verification alone reports the twin at least
    once" are asserted too, so the test cannot pass by finding nothing.

    Measured on one MI355X: verification alone reports the twin in 8 of the 10 frames (0, 2, 3, 5, 6, 7, 8, 9) and
    model 0 in all 10.  Arbitration suppresses the twin in 7 of the 8 (its first-round share 0.292-0.486, model 0 then
    owns everything).  On frame 8 the first-round shares are 0.500 (model 0, 16 of 32 tiles) and 0.581 (twin, 18 of 31):
    model 0 is suppressed and the twin kept -- 1 lost frame of 8 contested, where the calibration's rate allows 2.
    Both refined poses are about equally far from the truth there (2.2 and 2.5 degrees) and model 0's mean residual
    over all its points is even the smaller (0.0251 against 0.0273); with model 0 at the ground-truth pose the twin
    still owns 0.710 against 0.355: in that view depth residuals favour the twin."""
    frames = 10
    raw = [synth.make_model(k, 1500) for k in MEMBERS]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)
    found0 = kept0 = twin_verified = contested = 0
    lost0, table = [], []
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
        res, kept = db.arbitrate(view, Tf)
        table.append((f, [int(j) for j in np.flatnonzero(found)], [int(j) for j in np.flatnonzero(kept)],
                      round(res[0]["share"], 3), round(res[TWIN]["share"], 3)))
        found0 += bool(found[0])
        twin_verified += bool(found[TWIN])
        if found[0]:
            kept0 += bool(kept[0])
            if not kept[0]:
                lost0.append(f)
        assert not (kept & ~found).any()
        if found[0] and found[TWIN]:
            contested += 1
            assert kept[0] != kept[TWIN], (f, res[0], res[TWIN])             # exactly one of the two survives
            win, lose = (0, TWIN) if kept[0] else (TWIN, 0)
            assert res[lose]["suppressed_by"] == win and res[win]["suppressed_by"] == -1, (f, res[0], res[TWIN])
        elif found[0]:
            assert kept[0], (f, res[0])                                      # verified alone: kept
        view.close()
        sc.close()
    db.close()
    for m in models:
        m.close()
    print("verify alone reported the twin in %d of %d frames; model 0 found in %d, kept in %d" % (twin_verified, frames, found0, kept0))
    for row in table:
        print("frame %d found %s kept %s share 0: %.3f twin: %.3f" % row)
    assert found0 >= 9, table
    assert twin_verified >= 1, table             # otherwise this stream shows nothing about arbitration
    assert contested >= 1 and len(lost0) <= -(-contested // 4), (lost0, contested, table)


def copies_frame(ppf, synth, k, seed):
    """k copies of model 0 side by side at 10.5 m before the wall, with the rotations of the k-copy scene of
    tests/test_gpu_instances.py (synth.make_scene([0], S, seed, n_instances=k)), whose own translations lie outside any
    one camera's view."""
    mp, mn = synth.make_model(0, 1500)
    d = synth.d_dist_for(mp, 0.05)
    ext = synth.bbox_extent(mp)
    _, _, poses = synth.make_scene([0], 3000, seed, n_instances=k)
    dense, _ = synth.make_model(0, 200000)
    truths, pts = [], []
    for i, (_, P) in enumerate(poses):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = P[:3, :3]
        T[:3, 3] = [1.15 * ext * (i - 0.5 * (k - 1)), 0.1 * i, 10.5 + 0.3 * i]
        truths.append(T)
        pts.append(dense @ T[:3, :3].astype(np.float64).T + T[:3, 3])
    img = synth.render_depth(np.concatenate(pts), background_z=WALL, splat=1)
    return mp, mn, d, ext, truths, img


@pytest.mark.parametrize("k,seed", [(2, 3101), (3, 3102)])
def test_every_copy_of_one_model_survives(built_lib, ppf, synth, k, seed):
    mp, mn, d, ext, truths, img = copies_frame(ppf, synth, k, seed)
    model = ppf.Model(mp, mn, d_dist=d)
    sc = ppf.Scene.from_depth(img, KCAM["fx"], KCAM["fy"], KCAM["cx"], KCAM["cy"], leaf=d, d_dist=d,
                              ref_point_downsample_factor=4, z_min=KCAM["z_min"], z_max=KCAM["z_max"], max_jump=0.08)
    view = view_of(ppf, img, KCAM)
    # every copy at its ground-truth pose: all kept
    Tr = np.stack(truths)
    res, kept = ppf.arbitrate([model] * k, view, Tr)
    print("copies %d at the ground truth: verify found %s, shares %s"
          % (k, [bool(model.verify(view, T)["found"]) for T in Tr], [round(r["share"], 3) for r in res]))
    assert kept.all() and all(r["suppressed_by"] == -1 for r in res), res
    # and from the votes: whatever find_instances and verification confirm survives arbitration (refine's own presence
    # filter is off: a depth frame shows one side, verification judges presence)
    inst = model.find_instances(sc, params=ppf.default_instance_params(keep_not_found=1))
    Ti = [T for T, _ in inst if model.verify(view, T)["found"]]
    assert Ti, "find_instances found no copy that verification confirms"
    res, kept = ppf.arbitrate([model] * len(Ti), view, np.stack(Ti))
    near = [min(float(np.linalg.norm(T[:3, 3] - G[:3, 3])) for G in truths) for T in Ti]
    print("copies %d: find_instances %d, verified %d, kept %d, distance to the nearest truth / extent %s"
          % (k, len(inst), len(Ti), int(kept.sum()), [round(x / ext, 3) for x in near]))
    assert kept.all(), res
    view.close()
    sc.close()
    model.close()


def test_detect_equals_the_manual_chain(built_lib, ppf, synth):
    """Database.detect against find_instances -> verify of every instance -> arbitrate over the verified ones, on a
    frame with two copies of model 0 and a database of four members and the twin."""
    mp, mn, d, ext, truths, img = copies_frame(ppf, synth, 2, 3101)
    raw = [synth.make_model(m, 1500) for m in (0, 2, 3, 36)]
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)
    sc = ppf.Scene.from_depth(img, KCAM["fx"], KCAM["fy"], KCAM["cx"], KCAM["cy"], leaf=d, d_dist=d,
                              ref_point_downsample_factor=4, z_min=KCAM["z_min"], z_max=KCAM["z_max"], max_jump=0.08)
    view = view_of(ppf, img, KCAM)
    det = db.detect(sc, view)
    lists = db.find_instances(sc, params=ppf.default_detect_params().instances)
    flat = [(j, k, T) for j, lst in enumerate(lists) for k, (T, _) in enumerate(lst)]
    assert flat
    ver = [models[j].verify(view, T) for j, _, T in flat]
    Tz = np.stack([T if r["found"] else np.zeros((4, 4), np.float32) for (_, _, T), r in zip(flat, ver)])
    res, kept = ppf.arbitrate([models[j] for j, _, _ in flat], view, Tz)
    want = [(j, k, T, v, a) for (j, k, T), v, a, kp in zip(flat, ver, res, kept) if v["found"] and kp]
    assert len(det) == len(want) and len(det) >= 1, (len(det), len(want), ver, res)
    for g, (j, k, T, v, a) in zip(det, want):
        assert (g["model"], g["instance"]) == (j, k)
        assert np.asarray(g["T"], np.float32).tobytes() == np.asarray(T, np.float32).tobytes()
        assert stable(g["verify"]) == stable(v) and stable(g["arbitrate"]) == stable(a), (g, v, a)
    assert [g["model"] for g in det] == sorted(g["model"] for g in det)
    # the same call again gives the same detections
    again = db.detect(sc, view)
    assert [(g["model"], g["instance"], stable(g["arbitrate"])) for g in again] == \
        [(g["model"], g["instance"], stable(g["arbitrate"])) for g in det]
    view.close()
    sc.close()
    db.close()
    for m in models:
        m.close()
