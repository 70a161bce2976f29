"""CPU: the inputs of tests/render_edge_inputs.py reach the branches they are meant for, shown on the restatement
(tests/render_ref.py).  tests/test_gpu_render.py compares the device with the restatement on the same inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_edge_inputs as E  # noqa: E402
import render_ref as R  # noqa: E402

F = np.float32


def pts_of(c, hyp=0, **kw):
    mp, mn, d = E.hypotheses(c)[hyp]
    p = dict(c["params"], **kw)
    return R.points(mp, mn, c["T"][hyp], c["cam"], c["w"], c["h"], d, p["footprint"], p["max_splat"], p["keep_back"])


def test_the_image_is_ragged():
    assert E.W % 32 and E.W % 8 and E.H_IMG % 8 and E.SIZE_W % 32 and E.SIZE_H % 8


def test_border_points_are_clipped_and_outside_points_draw_nothing():
    cases, idx = E.border_cases()
    c = cases[0]
    draw, u, v, k, pz, back = pts_of(c)
    on = idx["border"]
    assert draw[on].all() and (k[on] == 2).all()
    assert sorted(zip(u[on].tolist(), v[on].tolist())) == sorted(E.BORDER_PIXELS)
    clipped = (u[on] - k[on] < 0) | (u[on] + k[on] >= E.W) | (v[on] - k[on] < 0) | (v[on] + k[on] >= E.H_IMG)
    assert clipped.all()
    assert not draw[idx["outside"]].any()
    ref = E.reference(c)
    for a, b in ((0, 0), (E.W - 1, 0), (0, E.H_IMG - 1), (E.W - 1, E.H_IMG - 1)):      # a corner keeps a 3 x 3 of the 5 x 5
        ys, xs = slice(max(b - 2, 0), min(b + 3, E.H_IMG)), slice(max(a - 2, 0), min(a + 3, E.W))
        assert (ref["labels"][ys, xs] == 0).sum() == 9
    # the ring one pixel outside would reach in with k = 2: nothing of it is there
    assert ref["labels"][7, 0] == -1 and ref["labels"][7, E.W - 1] == -1 and ref["labels"][0, 9] == -1
    assert int(ref["drawn"][0]) == int(draw.sum()) and int(ref["pixels"][0]) == int((ref["labels"] == 0).sum())


def test_z_limits_to_the_ulp_and_half_widths():
    cases, idx = E.border_cases()
    c = cases[0]
    draw, u, v, k, pz, back = pts_of(c)
    i_min, i_max, i_below, i_above = (idx[n][0] for n in ("z_min", "z_max", "below", "above"))
    assert pz[i_min] == E.Z_MIN and pz[i_max] == E.Z_MAX and draw[i_min] and draw[i_max]
    assert pz[i_below] < E.Z_MIN and pz[i_above] > E.Z_MAX and not draw[i_below] and not draw[i_above]
    assert pz[i_below] == np.nextafter(E.Z_MIN, F(0)) and pz[i_above] == np.nextafter(E.Z_MAX, F(np.inf))
    assert k[i_max] == 0 and k[i_min] == 8
    ref = E.reference(c)
    assert ref["z"][8, 30] == E.Z_MAX and (ref["z"] == E.Z_MAX).sum() == 1          # the far point: a single pixel
    near = cases[-1]
    assert near["name"] == "near capped"
    mp, mn, d = near["clouds"][0]
    rho = F(np.float64(F(0.75)) * np.float64(F(d)))
    assert np.floor((rho * F(E.CAM["fx"])) / F(0.6) + F(0.5)) > 8 and (pts_of(near)[3] == 8).all()
    zero = [x for x in cases if x["name"] == "border max_splat 0"][0]
    assert (pts_of(zero)[3] == 0).all()
    rz = E.reference(zero)
    assert int(rz["pixels"][0]) == len(set(zip(*[a[pts_of(zero)[0]].tolist() for a in pts_of(zero)[1:3]])))
    three = [x for x in cases if x["name"] == "border max_splat 3"][0]
    assert pts_of(three)[3].max() == 3


def test_two_points_of_one_pixel_and_back_faces():
    cases, idx = E.border_cases()
    c = cases[0]
    draw, u, v, k, pz, back = pts_of(c)
    a, b = idx["pair"]
    assert (u[a], v[a]) == (u[b], v[b]) == (24, 14) and draw[a] and draw[b] and pz[b] < pz[a]
    ref = E.reference(c)
    assert ref["z"][14, 24] == pz[b]
    i = idx["back"][0]
    assert back[i] and not draw[i] and back.sum() == 1
    keep = [x for x in cases if x["name"] == "border keep_back"][0]
    assert pts_of(keep)[0][i]
    rk = E.reference(keep)
    assert int(rk["drawn"][0]) == int(ref["drawn"][0]) + 1 and ref["labels"][6, 12] == -1 and rk["labels"][6, 12] == 0


def test_ties_go_to_the_lower_index_in_both_orders():
    xy, yx, skipped, none = E.tie_cases()
    a, b = E.reference(xy), E.reference(yx)
    assert a["z"].tobytes() == b["z"].tobytes()
    tie = (a["labels"] == 0) & (b["labels"] == 0)        # won by whoever comes first: bit-equal keys apart from the index
    assert tie[8:13, 8:13].all() and tie.sum() == 25
    assert a["z"][10, 10] == F(E.PLANE_Z)
    assert a["labels"][16, 16] == 1 and b["labels"][16, 16] == 0 and a["z"][16, 16] == F(1.9)
    s = E.reference(skipped)
    assert set(np.unique(s["labels"]).tolist()) == {-1, 0, 2} and s["drawn"][1] == 0 and s["pixels"][1] == 0
    assert s["tol"][1] == 0 and s["tol"][0] == F(E.D_EDGE)
    assert np.array_equal(s["labels"] == 2, a["labels"] == 1)
    n = E.reference(none)
    assert not n["z"].any() and (n["labels"] == -1).all() and not n["drawn"].any() and not n["pixels"].any()


def test_model_sizes_and_many_hypotheses(synth):
    c = E.size_case(synth)
    assert [len(x[0]) for x in c["clouds"]] == [255, 256, 257]
    ref = E.reference(c)
    assert (ref["drawn"] > 60).all() and (ref["pixels"] > 0).all(), ref["drawn"]
    assert len(pts_of(c, 2)[0]) == 257                   # the last hypothesis needs a second workgroup for one point
    m = E.many_case()
    assert len(m["member"]) == 1024 and len(m["clouds"]) == 3
    rm = E.reference(m)
    skipped = np.arange(1024) % 17 == 5
    assert not rm["drawn"][skipped].any() and (rm["drawn"][~skipped] >= 1).all()
    assert (rm["pixels"] > 0).sum() >= 200 and rm["labels"].max() > 512      # labels well beyond a workgroup's 256
    assert int(rm["pixels"].sum()) == int((rm["labels"] >= 0).sum())


def test_mask_by_hand():
    c, ref, img, names = E.mask_case()
    assert ref["pixels"][1] == 0 and ref["drawn"][1] == 6                 # the hidden hypothesis owns no pixel
    lab = ref["labels"]
    assert (lab[:10, :12] == 0).all() and (lab >= 0).sum() == 120          # the labels touch the corner's two borders
    for key in names:
        assert lab[names[key]] == 0
    z_o = R.V.view_z(img, 1.0, c["cam"]["z_min"], c["cam"]["z_max"])
    counts = {}
    for dilate in (0, 2, 8):
        rem, cr = R.mask(z_o, ref, R.REMOVE, dilate)
        keep, ck = R.mask(z_o, ref, R.KEEP, dilate)
        counts[dilate] = cr["object_pixels"]
        assert cr["valid_in"] == ck["valid_in"] == cr["valid_out"] + ck["valid_out"] == img.size - 1
        assert cr["object_pixels"] == ck["object_pixels"] == ck["valid_out"]
        assert np.array_equal((rem > 0) | (keep > 0), z_o > 0) and not ((rem > 0) & (keep > 0)).any()
        assert keep[names["exact"]] > 0 and rem[names["exact"]] == 0       # exactly tol behind: inside
        assert keep[names["beyond"]] == 0 and rem[names["beyond"]] > 0     # one ulp more: outside
        assert keep[names["occluder"]] == 0 and rem[names["occluder"]] == F(1.0)
        assert keep[names["invalid"]] == 0 and rem[names["invalid"]] == 0
    # the observed plane is larger than the render: the window reaches it, clipped by the two borders
    assert counts[0] == 120 - 3 and counts[2] == 14 * 12 - 3 and counts[8] == 14 * 16 - 3, counts
    only1, c1 = R.mask(z_o, ref, R.KEEP, 2, only=1)
    assert c1["object_pixels"] == 0 and not only1.any()
    only0, c0 = R.mask(z_o, ref, R.KEEP, 2, only=0)
    assert c0["object_pixels"] == counts[2]


@pytest.mark.parametrize("dilate", [0, 2])
def test_generic_observed_image_has_every_kind_of_pixel(synth, dilate):
    c = E.size_case(synth)
    ref = E.reference(c)
    img = E.observed(c, ref)
    z_o = R.V.view_z(img, 1.0, c["cam"]["z_min"], c["cam"]["z_max"])
    on = ref["labels"] >= 0
    assert np.isnan(img).any() and (z_o[on] == 0).any()
    obj = R.object_pixels(z_o, ref["z"], ref["labels"], ref["tol"], dilate)
    assert obj.any() and (on & (z_o > 0) & ~obj).any() and (~on & obj).any() == (dilate > 0)
