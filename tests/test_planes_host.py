"""CPU: the planes stage (include/oslam.h at oslam_view_planes) -- its defaults and argument checks through the C-ABI
with zeroed stand-in handles, the branches of the restatement (tests/planes_ref.py) on the named inputs
(tests/planes_inputs.py), the restatement's properties, the calibration table of DESIGN.md 7za
(tests/planes_calib.py) and the conditions the restatement has to meet on the calibration room before anything runs on
a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planes_calib as PC  # noqa: E402
import planes_inputs as PI  # noqa: E402
import planes_ref as PR  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def small():
    """Every small named input with the restatement's result and the trace over all of them."""
    trace = PR.new_trace()
    out = {}
    for c in PI.small_cases():
        res, z = PR.find_in_depth(c["depth"], c["cam"], c["max_jump"], trace=trace, **c["params"])
        out[c["name"]] = dict(c, res=res, z=z)
    return out, trace


# ---------------------------------------------------------------- defaults and argument checks
def test_planes_params_default(built_lib, ppf):
    p, want = ppf.default_planes_params(), PR.default_params()
    assert p.dist_tol == F(want["dist_tol"]) == F(0.02) and p.min_normal_dot == F(want["min_normal_dot"]) == F(0.9)
    assert p.label_min_dot == F(want["label_min_dot"]) == 0.0 and p.max_planes == want["max_planes"] == 4
    assert p.min_pixels == want["min_pixels"] == 0 and list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_planes_params(max_planes=8).max_planes == 8 and ppf.PLANES_MAX == PR.PLANES_MAX == 8
    assert ppf.PLANES_CANDIDATES == PR.CANDIDATES == 256 and C.sizeof(ppf.Plane) == PR.PLANE_DTYPE.itemsize == 32
    with pytest.raises(TypeError):
        ppf.default_planes_params(no_such_field=1)
    assert ppf.lib().oslam_planes_params_default(None) == ppf.OSLAM_E_INVALID
    for name in ("oslam_planes_params_default", "oslam_view_planes", "oslam_planes_get", "oslam_planes_labels",
                 "oslam_planes_rounds", "oslam_view_remove_planes", "oslam_planes_destroy"):
        assert name in ppf._SIGNATURES and hasattr(ppf.lib(), name)


def test_planes_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: the stand-in handles (zeroed host
    memory) are never looked at by a call that its parameters already refuse, with or without a GPU."""
    import torch
    L = ppf.lib()
    vbuf, pbuf = C.create_string_buffer(16384), C.create_string_buffer(16384)
    v, pl = C.cast(vbuf, C.c_void_p), C.cast(pbuf, C.c_void_p)
    res = ppf.PlanesResult()
    out = C.c_void_p(1)
    assert L.oslam_view_planes(None, None, C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    assert not out.value
    assert L.oslam_view_planes(v, None, None, C.byref(res)) == ppf.OSLAM_E_INVALID
    nan, inf = float("nan"), float("inf")
    for bad in (dict(dist_tol=0.0), dict(dist_tol=-0.02), dict(dist_tol=nan), dict(dist_tol=inf), dict(dist_tol=-inf),
                dict(dist_tol=1e-40), dict(min_normal_dot=1.5), dict(min_normal_dot=-1.5), dict(min_normal_dot=nan),
                dict(label_min_dot=1.0001), dict(label_min_dot=-2.0), dict(label_min_dot=nan), dict(label_min_dot=inf),
                dict(max_planes=0), dict(max_planes=9), dict(max_planes=1 << 31)):
        out = C.c_void_p(1)
        p = ppf.default_planes_params(**bad)
        assert L.oslam_view_planes(v, C.byref(p), C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID, bad
        assert not out.value, bad
        assert L.oslam_view_planes(v, C.byref(p), C.byref(out), None) == ppf.OSLAM_E_INVALID, bad
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_planes(v, C.byref(ppf.default_planes_params(max_planes=12)), C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "max_planes" in str(e.value)
    # good parameters: without a device the call says so, with one the stand-in view has no image
    out = C.c_void_p(1)
    rc = L.oslam_view_planes(v, None, C.byref(out), C.byref(res))
    assert rc == (ppf.OSLAM_E_INVALID if torch.cuda.is_available() else ppf.OSLAM_E_DEVICE) and not out.value

    # oslam_view_remove_planes: NULLs, the mode, only; then the handles' device, size and plane count
    mres = ppf.MaskResult()
    for args in ((None, pl, 0, -1), (v, None, 0, -1), (v, pl, 2, -1), (v, pl, -1, -1), (v, pl, 0, -2), (v, pl, 1, 0)):
        out = C.c_void_p(1)
        assert L.oslam_view_remove_planes(*args, C.byref(out), C.byref(mres)) == ppf.OSLAM_E_INVALID, args[2:]
        assert not out.value
    assert L.oslam_view_remove_planes(v, pl, 0, -1, None, C.byref(mres)) == ppf.OSLAM_E_INVALID
    ints = C.cast(pbuf, C.POINTER(C.c_int))
    ints[0] = 1                                                      # another device
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_remove_planes(v, pl, 0, -1, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "devices" in str(e.value)
    ints[0], ints[1], ints[2] = 0, 640, 480                         # another size than the stand-in view's 0 x 0
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_remove_planes(v, pl, 0, -1, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "size" in str(e.value)
    ints[1], ints[2] = 0, 0
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_remove_planes(v, pl, 1, 0, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "only" in str(e.value)
    # the taps and the destructor
    n = C.c_size_t(7)
    assert L.oslam_planes_get(None, None, 0, C.byref(n)) == ppf.OSLAM_E_INVALID and n.value == 7
    assert L.oslam_planes_get(pl, None, 0, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_planes_get(pl, None, 0, C.byref(n)) == ppf.OSLAM_OK and n.value == 0      # a stand-in holds no plane
    assert L.oslam_planes_labels(None, None) == ppf.OSLAM_E_INVALID and L.oslam_planes_labels(pl, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_planes_rounds(None, None, None) == ppf.OSLAM_E_INVALID and L.oslam_planes_rounds(pl, None, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_planes_destroy(None) == ppf.OSLAM_E_INVALID


# ---------------------------------------------------------------- the restatement on the named inputs
def test_inputs_reach_every_branch_of_the_rule(small):
    cases, trace = small
    print("%d inputs; trace %s" % (len(cases), trace))
    for name, c in cases.items():
        r = c["res"]
        print("%-40s %d x %d: %d plane(s), ended by %s, labelled %d of %d valid" % (
            name, c["depth"].shape[1], c["depth"].shape[0], r["n_planes"], r["end"], r["labelled"], r["valid_in"]))
    for k in PR.TRACE_KEYS:
        assert trace[k] > 0, (k, trace)
    sizes = {c["depth"].shape[::-1] for c in cases.values()}
    assert {(37, 21), (64, 16), (33, 9), (7, 5), (3, 3), (40, 1)} <= sizes
    assert {c["depth"].dtype for c in cases.values()} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert {c["params"].get("max_planes", 4) for c in cases.values()} >= {1, 4, 8}


def test_named_inputs_do_what_their_names_say(small):
    cases, _ = small
    for kind in ("f32", "u16"):
        one = cases["one_plane_37x21_" + kind]["res"]
        assert one["n_planes"] == 1 and one["labelled"] == one["valid_in"] == 37 * 21
        # the symmetric corner: node (a, b) and node (15 - a, b) tie bit for bit; the lowest index wins each round
        tie = cases["tie_corner_33x9_" + kind]["res"]
        cnt = tie["counts"][0].reshape(16, 16)
        assert np.array_equal(cnt, cnt[:, ::-1]) and cnt.max() > 0
        assert tie["n_planes"] == 2 and int(tie["planes"]["candidate"][0]) == int(np.argmax(tie["counts"][0]))
        assert int(tie["planes"]["candidate"][0]) % 16 < 8 <= int(tie["planes"]["candidate"][1]) % 16
        assert tie["planes"]["normal"][0][0] * tie["planes"]["normal"][1][0] < 0    # one half, then the other
        stairs = cases["staircase_64x16_" + kind]["res"]
        assert stairs["n_planes"] == 8 and stairs["end"] == "max_planes" and stairs["labelled"] < stairs["valid_in"]
        assert cases["thin_strip_64x16_" + kind]["res"]["end"] == "degenerate"
        assert cases["one_normal_3x3_" + kind]["res"]["end"] == "degenerate"
        assert cases["one_normal_3x3_" + kind]["res"]["counts"][0].max() == 1
        assert cases["no_normals_40x1_" + kind]["res"]["end"] == "no_candidate"
        assert cases["holes_and_step_37x21_" + kind]["res"]["n_planes"] == 2
        far = cases["far_plane_64x16_" + kind]["res"]
        # the pixels beyond the bound were counted and are labelled, but took no part in the fit
        assert far["n_planes"] == 1 and far["planes"]["support"][0] < far["counts"][0].max() < far["planes"]["pixels"][0] == 64 * 16
        for mp in (1, 4, 8):
            a = cases["room_corner_37x21_%s_max%d_dot0" % (kind, mp)]["res"]
            b = cases["room_corner_37x21_%s_max%d_dot0.95" % (kind, mp)]["res"]
            assert a["n_planes"] == b["n_planes"] == min(mp, 3) and b["labelled"] < a["labelled"]
            assert np.array_equal(a["planes"]["normal"], b["planes"]["normal"])     # the label gate does not move the fit
    exact, short = cases["min_pixels_exact_37x21"], cases["min_pixels_one_short_37x21"]
    assert exact["res"]["counts"][0].max() == exact["params"]["min_pixels"] == short["params"]["min_pixels"] - 1
    assert exact["res"]["n_planes"] == 1 and short["res"]["n_planes"] == 0 and short["res"]["end"] == "min_pixels"
    assert np.array_equal(short["res"]["counts"], exact["res"]["counts"])           # the round that ended keeps its counts


def test_restatement_properties(small):
    cases, _ = small
    for name, c in cases.items():
        r, z = c["res"], c["z"]
        lab = r["labels"]
        assert lab.min() >= -1 and lab.max() == r["n_planes"] - 1 and not (lab[z == 0] >= 0).any(), name
        assert [int((lab == k).sum()) for k in range(r["n_planes"])] == [int(x) for x in r["planes"]["pixels"]], name
        for p in r["planes"]:
            n = p["normal"].astype(np.float64)
            assert abs(np.linalg.norm(n) - 1.0) < 1e-6 and p["support"] <= r["counts"].max() and p["rms"] >= 0, name
        # the two modes partition the valid pixels, with and without `only`
        for only in (-1, r["n_planes"] - 1):
            if only < -1:
                continue
            zr, (vin, obj, kept) = PR.remove(z, lab, "remove", only)
            zk, (vin2, obj2, kept2) = PR.remove(z, lab, "keep", only)
            assert vin == vin2 == r["valid_in"] and obj == obj2 == kept2 and kept + kept2 == vin, name
            assert np.array_equal(zr + zk, z) and not (zr * zk).any(), name
        # a second run gives the same bytes
        again, _ = PR.find_in_depth(c["depth"], c["cam"], c["max_jump"], **c["params"])
        assert all(again[k].tobytes() == r[k].tobytes() for k in ("planes", "labels", "counts", "moments")), name
    assert PR.launches(4, True) == 17 and PR.launches(8, False) == 32 and PR.launches(1, False) == 4


def test_moment_sums_cannot_overflow():
    """The header's proof in numbers: |q| <= 2^17 after the float range test, a product <= 2^34, w * h <= 2^28 pixels."""
    q = int(np.rint(PR.BOUND))
    assert q == 1 << 17 and q * q * (1 << 28) == 1 << 62 < (1 << 63) - 1
    assert 16384 * 16384 == 1 << 28                                  # the largest image a view can hold
    # rintf cannot leave the bound: the float test is on the value that is converted
    assert int(np.rint(np.nextafter(PR.BOUND, F(0)))) <= q


# ---------------------------------------------------------------- the calibration room
def test_room_with_the_defaults_keeps_objects_and_labels_planes(pkg):
    worst_obj, worst_plane = 1.0, 1.0
    for f, planes in zip(PC.FRAMES, (3, 2, 2, 2)):
        res, _, s = PC.run(f)
        lost, n = PC.lost_normals(f)
        print("frame %d: %d planes, plane pixels labelled %.4f, object pixels kept %.4f; kept object pixels that lose their "
              "normal in the reduced view %.4f of %d" % (f, s["planes"], s["plane_labelled"], s["object_kept"], lost, n))
        assert s["planes"] == planes and s["object_kept"] >= 0.99 and s["plane_labelled"] >= 0.95, (f, s)
        assert lost < 0.02, (f, lost)
        worst_obj, worst_plane = min(worst_obj, s["object_kept"]), min(worst_plane, s["plane_labelled"])
    print("worst: object pixels kept %.4f, plane pixels labelled %.4f" % (worst_obj, worst_plane))


def test_calibration_table_holds(pkg):
    rows = PC.table()
    print(PC.fmt(rows))
    assert len(rows) == 27
    cell = {(r["noise_mm"], r["dist_tol"], r["min_normal_dot"]): r for r in rows}
    for noise in PC.NOISE_MM:
        d = cell[(noise, 0.02, 0.9)]
        # the defaults hold the host test's thresholds at every noise level
        assert d["plane_labelled"] >= 0.95 and d["object_kept"] >= 0.99, d
        # a wider gate labels no fewer plane pixels and eats into the objects
        wide = cell[(noise, 0.03, 0.9)]
        assert wide["object_kept"] < d["object_kept"], (d, wide)
        # the normal gate hardly matters on this room: the distance gate decides
        for dot in PC.MIN_NORMAL_DOT:
            assert abs(cell[(noise, 0.02, dot)]["plane_labelled"] - d["plane_labelled"]) < 0.002
    # a gate of 0.01 m is below the noise: it loses the planes at 3 mm and collapses at 6 mm
    assert cell[(3.0, 0.01, 0.9)]["plane_labelled"] < 0.9 and cell[(6.0, 0.01, 0.9)]["plane_labelled"] < 0.5
    for r in rows:
        if r["noise_mm"] == 0.0:
            assert r["planes"] == (3, 2, 2, 2), r
