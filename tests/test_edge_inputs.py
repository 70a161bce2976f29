"""CPU: the conditions on the inputs of tests/edge_inputs.py, asserted on the numpy restatements alone, so that the
device comparisons of tests/test_gpu_view_edges.py cannot pass on empty or one-sided data: every border row, column and
corner and the ring outside are hit, every class occurs, a model size stops below 6 correspondences and another steps,
the many-hypotheses calls suppress across the 256-thread stride, identical hypotheses leave in descending order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arbitrate_ref as A  # noqa: E402
import edge_inputs as E  # noqa: E402
import track_ref as K  # noqa: E402
import view_ref as V  # noqa: E402


@pytest.mark.parametrize("h,w", E.SHAPES)
def test_shapes_pass_the_restatements_and_reach_every_border(synth, h, w):
    c = E.shape_case(h, w, synth)
    assert c["img"].shape == c["fimg"].shape == (h, w)
    if h * w >= 3:
        assert (c["img"] == 0).any() and (c["img"] == 65535).any()
    if h * w >= 40:
        f = c["fimg"]
        assert np.isnan(f).any() and (f == -1).any() and np.isinf(f).any() and (f == 0).any()
    assert abs(c["cam"]["cx"] - 0.5 * (w - 1)) > 0.05 * w and abs(c["cam"]["cy"] - 0.5 * (h - 1)) > 0.05 * h
    seen = np.zeros(6, np.int64)
    for img, cam in ((c["img"], c["cam"]), (c["fimg"], c["fcam"])):
        z = V.view_z(img, cam["depth_scale"], cam["z_min"], cam["z_max"])
        assert z.shape == (h, w) and np.isfinite(z).all()
        maps = K.view_maps(img, cam, E.MAX_JUMP)
        for name, T in c["poses"].items():
            for window in range(4):
                seen += np.bincount(E.ref_classes(c["mp"], c["mn"], T, img, cam, c["d"], window), minlength=6)
            K.correspondences(c["mp"], c["mn"], T, maps, cam, np.float32(2.0) * np.float32(c["d"]), 0.8)
        for tile in (4, 7, 128, 0):
            cnt, sm, used, _ = A.claims([(c["mp"], c["mn"], c["d"])] * 2, [c["poses"]["identity"], c["poses"]["tilt"]], img, cam,
                                        tile=tile)
            assert cnt.shape == (2, -(-w // used) * -(-h // used))
    assert seen[V.SUPPORTED] > 0 and seen[V.OUT] > 0, (h, w, seen)
    if (h, w) == (61, 83):
        assert (seen > 0).all(), seen
    if h >= 3 and w >= 3:
        maps = K.view_maps(c["img"], c["cam"], E.MAX_JUMP)
        assert maps[2].any()                                  # some pixel has a normal
        pix, _, _ = K.correspondences(c["mp"], c["mn"], c["poses"]["identity"], maps, c["cam"],
                                      np.float32(2.0) * np.float32(c["d"]), 0.8)
        assert (pix >= 0).any()
        # the identity pose: the grid points land on the pixels they were made from
        fu, fv, _, back = E.project(c["mp"], c["mn"], c["poses"]["identity"], c["cam"])
        fu, fv = fu[~back], fv[~back]
        hit = set(zip(fu.astype(int).tolist(), fv.astype(int).tolist()))
        for corner in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
            assert corner in hit, corner
        inside_u, inside_v = (fu >= 0) & (fu < w), (fv >= 0) & (fv < h)
        for cond in ((fu == 0) & inside_v, (fu == w - 1) & inside_v, (fv == 0) & inside_u, (fv == h - 1) & inside_u,     # the borders
                     (fu == -1) & inside_v, (fu == w) & inside_v, (fv == -1) & inside_u, (fv == h) & inside_u):          # one outside
            assert cond.any()
        for window in range(4):
            cls = E.ref_classes(c["mp"], c["mn"], c["poses"]["identity"], c["img"], c["cam"], c["d"], window)[~back]
            assert (cls[(fu == -1) | (fu == w) | (fv == -1) | (fv == h)] == V.OUT).all()
            border = inside_u & inside_v & ((fu == 0) | (fu == w - 1) | (fv == 0) | (fv == h - 1))
            assert (cls[border] >= V.SUPPORTED).all() and (cls[border] == V.SUPPORTED).any()


def test_model_sizes_stop_below_six_correspondences_and_step_above(synth):
    c = E.size_case(synth)
    img, cam = c["frames"]["640x480"]
    maps = K.view_maps(img, cam, K.STREAM_MAX_JUMP)
    few, stepped = [], []
    for n in E.MODEL_SIZES:
        W, w = K.track(c["mp"][:n], c["mn"][:n], c["previous"], img, cam, c["d"], K.STREAM_MAX_JUMP, maps=maps)
        if w["iterations"] == 0:
            pix, _, _ = K.correspondences(c["mp"][:n], c["mn"][:n], c["previous"], maps, cam, np.float32(2.0) * np.float32(c["d"]), 0.8)
            assert w["correspondences"] == int((pix >= 0).sum()) < 6 and np.array_equal(W, c["previous"])
            if 1 <= w["correspondences"]:
                few.append(n)
        elif w["correspondences"] >= 6:
            stepped.append(n)
    print("sizes with 1..5 correspondences:", few, "sizes that step:", stepped)
    assert few and stepped and max(stepped) == 1025


@pytest.mark.parametrize("key,H", [("96x64/16", 255), ("96x64/16", 256), ("96x64/16", 257), ("160x32/32", 1024), ("192x32/32", 1024)])
def test_many_hypotheses_suppress_across_the_thread_stride(synth, key, H):
    c = E.many_case(synth, key, H)
    w, h, tile = E.MANY_VIEWS[key]
    n_tiles = -(-w // tile) * -(-h // tile)
    assert n_tiles <= 24
    if H == 1024:
        assert (key == "160x32/32" and H * n_tiles * 8 == 40960) or (key == "192x32/32" and H * n_tiles * 8 > 40960)
    for i in (0, 255, 256, H - 1):
        if i < H:
            assert not c["T"][i].any()
    assert any((c["T"][i] == c["T"][j]).all() and c["mem"][i] == c["mem"][j] and c["T"][i].any()
               for i in range(3, H) for j in (i - 2,))       # exact duplicates
    sup = [(i, r["suppressed_by"]) for i, r in enumerate(c["want"]) if r["suppressed_by"] >= 0]
    assert sup and c["kept"].any() and c["want"][0]["rounds"] > 1
    assert len({c["mem"][i] for i in range(H) if c["T"][i].any()}) == 3
    # A kept hypothesis and a suppressor with an index >= 256: only the 1024 cases are built to reach them.  At 255 and
    # 256 no such index exists, and at 257 the only one, 256 = H - 1, is one of the skipped poses the issue asks for.
    if H == 1024:
        assert any(i >= 256 for i in np.flatnonzero(c["kept"])), np.flatnonzero(c["kept"])
        assert any(by >= 256 for _, by in sup), sup[:8]


def test_identical_hypotheses_leave_in_descending_order(synth):
    H = 257
    c = E.identical_case(synth, H)
    kept, by = E.identical_answer(H)
    assert [r["kept"] for r in c["want"]] == kept and [r["suppressed_by"] for r in c["want"]] == by
    assert c["rounds"] == H and c["order"] == list(range(H - 1, 0, -1))
    assert c["want"][0]["claimed"] >= 1


def test_tie_tables_hold_their_ties():
    t = E.tie_tables()
    for k in range(6):
        res, rounds = E.eliminate_table(*t["mean tie %d" % k])
        assert [r["kept"] for r in res] == [True, False, False] and [r["suppressed_by"] for r in res] == [-1, 0, 0], k
    res, _ = E.eliminate_table(*t["large counts"])
    cnt, sm = t["large counts"][:2]
    assert int(cnt.max()) * int(sm.max()) > (1 << 63) and res[2]["owned"] >= 1 and res[3]["owned"] >= 1
    for gap in (256, 512):
        res, _ = E.eliminate_table(*t["share tie +%d" % gap])
        for h in (3, 17, 39):
            assert res[h]["kept"] and not res[h + gap]["kept"] and res[h + gap]["suppressed_by"] == h
            assert res[h + gap]["share"] == np.float32(0.5)
        res, _ = E.eliminate_table(*t["beat tie +%d" % gap])
        H = gap + 40
        assert res[H - 1]["suppressed_by"] == 5 and res[5]["kept"] and res[5 + gap]["kept"]
    for name, nbytes in (("40960 bytes", 40960), ("40960 bytes 512x10", 40960), ("40968 bytes", 40968)):
        assert t[name][0].size * 8 == nbytes
        res, rounds = E.eliminate_table(*t[name])
        assert rounds > 1 and any(r["kept"] for r in res)
    res, rounds = E.eliminate_table(*t["min_tiles above every claim"])
    assert rounds == 0 and not any(r["kept"] for r in res)
    res, _ = E.eliminate_table(*t["all skipped but one"])
    assert [h for h, r in enumerate(res) if r["kept"]] == [7]
    tabs = E.random_tables()
    assert len(tabs) == 205 and sum(c.shape[0] > 256 for c, *_ in tabs) == 5


def test_track_sums_switch_keeps_the_float64_path(synth):
    """the float64 sums are the restatement the other tests use; the float32 sums in index order land close by"""
    c = E.size_case(synth)
    img, cam = c["frames"]["333x251"]
    a, ra = K.track(c["mp"][:513], c["mn"][:513], c["previous"], img, cam, c["d"], K.STREAM_MAX_JUMP)
    b, rb = K.track(c["mp"][:513], c["mn"][:513], c["previous"], img, cam, c["d"], K.STREAM_MAX_JUMP, sums="f32")
    assert ra["iterations"] >= 1 and rb["iterations"] >= 1 and ra["cond"] > 1
    assert np.abs(a - b).max() < 1e-3 and not np.array_equal(a, c["previous"])
