"""GPU: the verification stage (oslam_view_*, oslam_verify, oslam_db_verify, oslam_verify_classes) against the numpy
restatement of tests/view_ref.py, and presence on the depth stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import view_ref as V  # noqa: E402
from test_verify_host import KCAM, WALL, moved  # noqa: E402

pytestmark = pytest.mark.gpu

DYN = ("launches", "ms_total")
STREAM_CAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=12.0)


def view_of(ppf, img, cam):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"])


def ref_classes(mp, mn, T, img, cam, d, window=1, depth_tol=1.0):
    z = V.view_z(img, cam["depth_scale"], cam["z_min"], cam["z_max"])
    return V.classify(mp, mn, T, z, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["z_min"], cam["z_max"],
                      V.tolerance(depth_tol, d), window)


@pytest.fixture(scope="module")
def frame(ppf, synth):
    """Model 0 (1500 points) at 10.5 m before a wall at 20 m, its voting and refined poses, and the poses of the
    known-answer cases."""
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
    sc = ppf.Scene.from_depth(img, KCAM["fx"], KCAM["fy"], KCAM["cx"], KCAM["cy"], leaf=d, d_dist=d,
                              ref_point_downsample_factor=4, z_min=KCAM["z_min"], z_max=KCAM["z_max"], max_jump=0.08)
    Tv = model.ppf_lookup(sc).copy()
    Tr, _ = model.refine(sc, Tv)
    poses = {"truth": T, "vote": Tv, "refined": Tr, "toward": moved(T, dz=-2.0 * ext),
             "behind": moved(T, dz=WALL + ext - T[2, 3]), "right": moved(T, dx=50.0), "far": moved(T, dz=40.0),
             "half_out": moved(T, dx=6.0)}
    yield dict(mp=mp, mn=mn, d=d, img=img, model=model, poses=poses)
    sc.close()
    model.close()


def test_classes_equal_restatement(built_lib, ppf, frame):
    c = frame
    # the same depths as a float image in metres (scale 1), with invalid entries of every kind sprinkled in
    fimg = c["img"].astype(np.float32) * np.float32(0.001)
    fimg[::7, ::5] = np.nan
    fimg[3::11, ::3] = -1.0
    fimg[5::13, 1::4] = np.inf
    fcam = dict(KCAM, depth_scale=1.0)
    for img, cam in ((c["img"], KCAM), (fimg, fcam)):
        view = view_of(ppf, img, cam)
        for name, T in c["poses"].items():
            for window in range(4):
                p = ppf.default_verify_params(window=window)
                got = ppf.verify_classes(c["model"], view, T, p)
                want = ref_classes(c["mp"], c["mn"], T, img, cam, c["d"], window)
                assert np.array_equal(got, want), (name, window, img.dtype, np.flatnonzero(got != want)[:8])
        got = ppf.verify_classes(c["model"], view, c["poses"]["truth"], ppf.default_verify_params(depth_tol=0.25))
        assert np.array_equal(got, ref_classes(c["mp"], c["mn"], c["poses"]["truth"], img, cam, c["d"], 1, 0.25))
        view.close()
    view = view_of(ppf, c["img"], KCAM)
    hist = {n: np.bincount(ppf.verify_classes(c["model"], view, T), minlength=6) for n, T in c["poses"].items()}
    view.close()
    assert hist["truth"][V.SUPPORTED] > 300 and hist["toward"][V.CONFLICT] > 300 and hist["right"][V.OUT] > 300
    assert hist["behind"][V.OCCLUDED] > 300 and hist["half_out"][V.OUT] > 0 and hist["half_out"][V.SUPPORTED] == 0


def test_counts_equal_tap_and_restatement(built_lib, ppf, frame):
    c = frame
    view = view_of(ppf, c["img"], KCAM)
    for name, T in c["poses"].items():
        r = c["model"].verify(view, T)
        cls = ppf.verify_classes(c["model"], view, T)
        h = np.bincount(cls, minlength=6)
        assert [r[k] for k in V.NAMES] == list(h), (name, r, h)
        want = V.scores(cls)
        assert np.float32(r["view_fitness"]) == np.float32(want["view_fitness"]), name
        assert np.float32(r["coverage"]) == np.float32(want["coverage"]), name
        assert bool(r["found"]) == want["found"], (name, r)
        assert r["launches"] == 1
    assert c["model"].verify(view, c["poses"]["truth"])["found"]
    for name in ("toward", "behind", "right", "far"):
        assert not c["model"].verify(view, c["poses"][name])["found"], name
    view.close()


def test_db_members_equal_single_calls_and_zero_poses_are_skipped(built_lib, ppf, synth, frame):
    c = frame
    others = []
    for k in (2, 3, 5):
        p, n = synth.make_model(k, 700)
        others.append(ppf.Model(p, n, d_dist=synth.d_dist_for(p, 0.05)))
    models = [c["model"]] + others
    db = ppf.Database(models)
    view = view_of(ppf, c["img"], KCAM)
    P = c["poses"]
    T = np.stack([P["refined"], P["truth"], np.zeros((4, 4), np.float32), P["toward"]])
    res, found = db.verify(view, T)
    for j, m in enumerate(models):
        if not T[j].any():
            assert all(res[j][k] == 0 for k in res[j] if k not in DYN) and not found[j]
            continue
        single = m.verify(view, T[j])
        assert {k: v for k, v in single.items() if k not in DYN} == {k: v for k, v in res[j].items() if k not in DYN}, j
    assert found[0] and not found[3]
    rz, fz = db.verify(view, np.zeros((4, 4, 4), np.float32))
    assert not fz.any() and all(r["supported"] == 0 and r["launches"] == 0 for r in rz)
    view.close()
    db.close()
    for m in others:
        m.close()


def test_launches_do_not_depend_on_members_and_results_repeat(built_lib, ppf, synth, frame):
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
    for members in (models[:1], models):
        db = ppf.Database(members)
        a, fa = db.verify(view, T[: len(members)])
        b, fb = db.verify(view, T[: len(members)])
        assert np.array_equal(fa, fb)
        assert [{k: v for k, v in r.items() if k not in DYN} for r in a] == \
            [{k: v for k, v in r.items() if k not in DYN} for r in b]
        assert all(r["launches"] == a[0]["launches"] for r in a)
        assert all(sum(r[k] for k in V.NAMES) == m.n for r, m in zip(a, members))
        launches.append(a[0]["launches"])
        db.close()
    assert launches == [1, 1]
    view.close()
    for m in models:
        m.close()


def test_depth_stream_finds_only_the_rendered_model(built_lib, ppf, synth):
    """The 10-model depth stream of tests/test_gpu_refine.py over 10 frames of the db50 seeds (tools/bench_configs.py
    verify reports the 50-model stream): db.align -> db.refine -> db.verify.  refine's `found` marks model 0 in about
    half of these frames; verification must find it in at least 9 and never report an absent member."""
    n_models, frames = 10, 10
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)
    found_frames, false, table = 0, [], []
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
        res, found = db.verify(view, Tr)
        table.append([(round(r["view_fitness"], 3), round(r["coverage"], 3), r["supported"]) for r in res])
        found_frames += bool(found[0])
        false += [(f, int(j)) for j in np.flatnonzero(found[1:]) + 1]
        view.close()
        sc.close()
    db.close()
    for m in models:
        m.close()
    assert found_frames >= 9 and not false, (found_frames, false, table)
