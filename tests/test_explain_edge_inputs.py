"""CPU: the inputs of tests/explain_edge_inputs.py reach the branches they are meant for, asserted on the restatement
(tests/explain_ref.py), and the rectangles the host gives the same hypotheses (oslam_explain_rect, no device) have the
shapes the GPU test needs: empty for the hypothesis off the image, widths that are no multiple of 32 and heights that
are no multiple of 8, more than one 32 x 8 block."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explain_edge_inputs as XE  # noqa: E402
import explain_ref as X  # noqa: E402
import render_edge_inputs as E  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def cases(synth):
    out = {}
    for c in XE.edge_cases(synth):
        taps = {}
        out[c["name"]] = (c, XE.reference(c, taps), taps)
    return out


def classes_of(c, taps, h):
    z_o = X.view_ref.view_z(c["img"], 1.0, c["cam"]["z_min"], c["cam"]["z_max"])
    tol = X.view_ref.tolerance(c["params"]["depth_tol"], E.hypotheses(c)[h][2])
    cls, _ = X.classify(taps["z"][h], z_o, tol)
    return cls, z_o, tol


def test_tolerance_to_the_ulp_and_invalid_pixels(cases):
    c, res, taps = cases["border default"]
    cls, z_o, tol = classes_of(c, taps, 0)
    z_h = taps["z"][0]
    on = z_h > 0
    for key, want in (("behind_eq", X.AGREE), ("front_eq", X.AGREE), ("behind_ulp", X.THROUGH), ("front_ulp", X.OCCLUDED),
                      ("occluder", X.OCCLUDED)):
        later = [k for k in list(XE.PATTERN)[list(XE.PATTERN).index(key) + 1:]] + ["invalid"]
        s = on & XE.pattern(z_h.shape, key)
        for k in later:                                   # a later pattern overwrites an earlier one
            s &= ~XE.pattern(z_h.shape, k)
        s &= (z_o > 0) & (z_h >= F(1))                    # in front of the splats at z_min the image is invalid
        assert s.sum() >= 2 and (cls[s] == want).all(), (key, s.sum(), cls[s])
        if key.endswith("_eq"):
            assert (np.abs(z_o[s] - z_h[s]) == tol).all()
        if key.endswith("_ulp"):
            assert (np.abs(z_o[s] - z_h[s]) > tol).all() and (np.abs(z_o[s] - z_h[s]) < tol * F(1.0001)).all()
    s = on & (XE.pattern(z_h.shape, "invalid") | XE.pattern(z_h.shape, "nan"))
    assert s.sum() >= 4 and (cls[s] == X.UNKNOWN).all()
    r = res[0]
    assert min(r["agree"], r["occluded"], r["through"], r["unknown"]) > 0
    assert r["pixels"] == int(on.sum()) == r["agree"] + r["occluded"] + r["through"] + r["unknown"]
    # a residual at the tolerance quantises to the cap
    _, q = X.classify(z_h, z_o, tol)
    assert q.max() == 65535 and r["resid_sum"] == int(q.sum())


def test_splats_touch_every_border_and_corner(cases):
    c, res, taps = cases["border default"]
    z = taps["z"][0]
    for a, b in E.BORDER_PIXELS:
        assert z[b, a] > 0, (a, b)
    c0, r0, t0 = cases["border max_splat 0"]
    assert (t0["z"][0] > 0).sum() < (z > 0).sum() and r0[0]["drawn"] == res[0]["drawn"]
    assert cases["border keep_back"][1][0]["drawn"] == res[0]["drawn"] + 1
    assert {cases[n][1][0]["tile"] for n in cases if n.startswith("border") or n == "near capped"} >= {4, 7, 128}
    assert cases["border keep_back"][1][0]["tile"] not in (0, 7, 128)      # the automatic tile, resolved


def test_rectangles(built_lib, ppf, cases):
    seen_w, seen_h, blocks = set(), set(), 0
    for name, (c, res, taps) in cases.items():
        cam = ppf.Camera(c["cam"]["fx"], c["cam"]["fy"], c["cam"]["cx"], c["cam"]["cy"], 1.0, c["cam"]["z_min"],
                         c["cam"]["z_max"], 0.05)
        for h, ((mp, _, _), T) in enumerate(zip(E.hypotheses(c), c["T"])):
            if h >= 40:
                break
            centre = mp.astype(np.float64).mean(axis=0)
            radius = float(np.sqrt(((mp.astype(np.float64) - centre) ** 2).sum(axis=1)).max())
            x0, y0, w, hh = ppf.explain_rect(centre, radius, T, cam, c["w"], c["h"], c["params"]["max_splat"])
            ys, xs = np.nonzero(taps["z"][h] > 0)
            if len(ys):
                assert x0 <= xs.min() and xs.max() < x0 + w and y0 <= ys.min() and ys.max() < y0 + hh, (name, h)
                seen_w.add(w % 32)
                seen_h.add(hh % 8)
                blocks = max(blocks, ((w + 31) // 32) * ((hh + 7) // 8))
            if name == "off image" and h >= 1:
                assert w == 0 or hh == 0, (name, h, (x0, y0, w, hh))
    assert len(seen_w - {0}) >= 3 and len(seen_h - {0}) >= 3 and blocks >= 4, (seen_w, seen_h, blocks)


def test_off_image_and_skipped(cases):
    c, res, taps = cases["off image"]
    assert res[0]["kept"] and res[0]["drawn"] > 0
    for h in (1, 2, 3):
        r = res[h]
        assert not r["kept"] and r["suppressed_by"] == -1 and r["drawn"] == r["pixels"] == r["claimed"] == 0, (h, r)
    c, res, taps = cases["skipped between"]
    assert res[1] == dict(X.zero_result(), tile=res[1]["tile"], rounds=res[1]["rounds"]) and res[0]["kept"] and res[2]["pixels"] > 0
    c, res, taps = cases["all skipped"]
    assert all(r["rounds"] == 0 and not r["kept"] and r["pixels"] == 0 for r in res)
    c, res, taps = cases["one hypothesis"]
    assert len(res) == 1 and res[0]["kept"] and res[0]["rounds"] == 1 and res[0]["share"] == F(1)


def test_conflict_rates(cases):
    c, res, taps = cases["see through"]
    r = res[0]
    assert r["agree"] == 0 and r["through"] == r["pixels"] > 0 and r["explained"] == F(0) and r["conflict_q"] == 0
    assert r["claimed"] == 0 and not r["kept"] and (taps["cnt"] == 0).all()
    c, res, taps = cases["all agree"]
    r = res[0]
    assert r["through"] == 0 and r["agree"] == r["pixels"] > 0 and r["conflict_q"] == 0 and r["explained"] == F(1)
    assert r["kept"] and (taps["sum"] == 0).all() and taps["cnt"].sum() == r["agree"]
    c, res, taps = cases["equal rates"]
    a, b, dup = res
    assert a["conflict_q"] == b["conflict_q"] == dup["conflict_q"] > 0 and a["through"] == b["through"] > 0
    assert a["kept"] and b["kept"] and not dup["kept"] and dup["suppressed_by"] == 0 and dup["owned"] == 0
    assert not ((taps["cnt"][0] > 0) & (taps["cnt"][1] > 0)).any()      # the two patches never meet
    assert (taps["sum"][0] == taps["cnt"][0] * a["conflict_q"]).all()


def test_sizes_and_many(cases):
    c, res, taps = cases["sizes 255 256 257"]
    assert [len(x[0]) for x in c["clouds"]] == [255, 256, 257] and all(r["drawn"] > 0 and r["pixels"] > 0 for r in res)
    assert res[0]["tile"] == 7 and c["w"] % 7 and c["h"] % 7            # a partial last tile
    cb, rb, tb = cases["border max_splat 0"]
    last = tb["cnt"].reshape(-(-cb["h"] // 7), -(-cb["w"] // 7))
    assert rb[0]["tile"] == 7 and cb["w"] % 7 and cb["h"] % 7 and last[:, -1].sum() > 0 and last[-1, :].sum() > 0    # and claimed
    for n in (255, 256, 257, 1024):
        c, res, taps = cases["hypotheses %d" % n]
        assert len(res) == n and len(c["clouds"]) == 3 and res[0]["tile"] == 128 and taps["cnt"].shape == (n, 1)
        skipped = [h for h in range(n) if not c["T"][h].any()]
        assert len(skipped) >= n // 17 and all(res[h]["pixels"] == 0 for h in skipped)
        assert sum(r["agree"] > 0 for r in res) > n // 8 and sum(r["through"] > 0 for r in res) > 0
    c = XE.identical_case(257)
    res = XE.reference(c)
    wk, wby = XE.identical_answer(257)
    assert [r["kept"] for r in res] == wk and [r["suppressed_by"] for r in res] == wby and res[0]["rounds"] == 257
