"""CPU: the segments stage (include/oslam.h at oslam_view_segments) -- its defaults and argument checks through the
C-ABI with zeroed stand-in handles, the branches of the restatement (tests/segments_ref.py) on the named inputs
(tests/segments_inputs.py), the restatement's properties, the union-find header as a program of its own
(tests/native/seg_union_check.c, plain and under the sanitizers) and the calibration table of DESIGN.md 7zb
(tests/segments_calib.py) with the conditions the restatement has to meet on the calibration room."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_calib as SC  # noqa: E402
import segments_inputs as SI  # noqa: E402
import segments_ref as SR  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objective-slam_amd", "csrc")


@pytest.fixture(scope="module")
def small():
    """Every small named input with the restatement's result and the trace over all of them."""
    trace = SR.new_trace()
    out = {}
    for c in SI.small_cases():
        res, z, lab = SI.restate(c, trace)
        out[c["name"]] = dict(c, res=res, z=z, plane_labels=lab)
    return out, trace


# ---------------------------------------------------------------- defaults and argument checks
def test_segments_params_default(built_lib, ppf):
    p, want = ppf.default_segments_params(), SR.default_params()
    assert p.max_step == want["max_step"] == 0.0 and p.rel_step == want["rel_step"] == 0.0
    assert p.min_pixels == want["min_pixels"] == 0 and p.max_segments == want["max_segments"] == 16
    assert list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_segments_params(max_segments=64).max_segments == 64 and ppf.SEGMENTS_MAX == SR.SEGMENTS_MAX == 64
    assert ppf.SEGMENTS_CANDIDATES == SR.CANDIDATES == 4096 and ppf.SEGMENTS_LAUNCHES == SR.LAUNCHES == 6
    assert C.sizeof(ppf.Segment) == SR.SEGMENT_DTYPE.itemsize == 32 and C.sizeof(ppf.SegmentsParams) == 32
    assert C.sizeof(ppf.SegmentsResult) == 28
    with pytest.raises(TypeError):
        ppf.default_segments_params(no_such_field=1)
    assert ppf.lib().oslam_segments_params_default(None) == ppf.OSLAM_E_INVALID
    for name in ("oslam_segments_params_default", "oslam_view_segments", "oslam_segments_get", "oslam_segments_labels",
                 "oslam_segments_roots", "oslam_view_select_segments", "oslam_segments_destroy"):
        assert name in ppf._SIGNATURES and hasattr(ppf.lib(), name)


def test_segments_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Argument checks run before any device call: the stand-in handles are zeroed host memory (a view of 0 x 0 pixels on
    device 0 with max_jump 0), and a call that its parameters or its handles' fields refuse never gets further."""
    import torch
    L = ppf.lib()
    vbuf, pbuf, sbuf = C.create_string_buffer(16384), C.create_string_buffer(16384), C.create_string_buffer(16384)
    v, pl, sg = C.cast(vbuf, C.c_void_p), C.cast(pbuf, C.c_void_p), C.cast(sbuf, C.c_void_p)
    res = ppf.SegmentsResult()
    out = C.c_void_p(1)
    assert L.oslam_view_segments(None, None, None, C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    assert not out.value
    assert L.oslam_view_segments(v, None, None, None, C.byref(res)) == ppf.OSLAM_E_INVALID
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_step=-0.01), dict(max_step=nan), dict(max_step=inf), dict(max_step=-inf), dict(rel_step=-0.01),
                dict(rel_step=nan), dict(rel_step=inf), dict(max_segments=0), dict(max_segments=65), dict(max_segments=1 << 31)):
        out = C.c_void_p(1)
        p = ppf.default_segments_params(**dict(dict(max_step=0.05), **bad))
        assert L.oslam_view_segments(v, None, C.byref(p), C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID, bad
        assert not out.value, bad
        assert L.oslam_view_segments(v, pl, C.byref(p), C.byref(out), None) == ppf.OSLAM_E_INVALID, bad
    assert bytes(res) == bytes(ppf.SegmentsResult())                # a refused call writes nothing
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_segments(v, None, C.byref(ppf.default_segments_params(max_segments=99)), C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "max_segments" in str(e.value)
    # max_step 0 means the view's max_jump, and the stand-in view has none
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_segments(v, None, None, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "max_jump" in str(e.value)
    # planes of another device or size
    ok = ppf.default_segments_params(max_step=0.05)
    ints = C.cast(pbuf, C.POINTER(C.c_int))
    ints[0] = 1
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_segments(v, pl, C.byref(ok), C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "devices" in str(e.value)
    ints[0], ints[1], ints[2] = 0, 640, 480
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_segments(v, pl, C.byref(ok), C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "size" in str(e.value)
    ints[1], ints[2] = 0, 0
    # good parameters: without a device the call says so, with one the stand-in view has no image
    out = C.c_void_p(1)
    rc = L.oslam_view_segments(v, pl, C.byref(ok), C.byref(out), C.byref(res))
    assert rc == (ppf.OSLAM_E_INVALID if torch.cuda.is_available() else ppf.OSLAM_E_DEVICE) and not out.value

    # oslam_view_select_segments: NULLs, the mode, only; then the handles' device, size and segment count
    mres = ppf.MaskResult()
    for args in ((None, sg, 0, -1), (v, None, 0, -1), (v, sg, 2, -1), (v, sg, -1, -1), (v, sg, 0, -2), (v, sg, 1, 0)):
        out = C.c_void_p(1)
        assert L.oslam_view_select_segments(*args, C.byref(out), C.byref(mres)) == ppf.OSLAM_E_INVALID, args[2:]
        assert not out.value
    assert L.oslam_view_select_segments(v, sg, 0, -1, None, C.byref(mres)) == ppf.OSLAM_E_INVALID
    ints = C.cast(sbuf, C.POINTER(C.c_int))
    ints[0] = 1
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_select_segments(v, sg, 0, -1, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "devices" in str(e.value)
    ints[0], ints[1], ints[2] = 0, 640, 480
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_select_segments(v, sg, 0, -1, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "size" in str(e.value)
    ints[1], ints[2] = 0, 0
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_select_segments(v, sg, 1, 0, C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "only" in str(e.value)
    # the taps and the destructor
    n = C.c_size_t(7)
    assert L.oslam_segments_get(None, None, 0, C.byref(n)) == ppf.OSLAM_E_INVALID and n.value == 7
    assert L.oslam_segments_get(sg, None, 0, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_segments_get(sg, None, 0, C.byref(n)) == ppf.OSLAM_OK and n.value == 0    # a stand-in holds no segment
    assert L.oslam_segments_labels(None, None) == ppf.OSLAM_E_INVALID and L.oslam_segments_labels(sg, None) == ppf.OSLAM_E_INVALID
    assert L.oslam_segments_roots(None, None) == ppf.OSLAM_E_INVALID and L.oslam_segments_roots(sg, None) == ppf.OSLAM_E_INVALID
    buf = np.zeros(4, np.int32)
    assert L.oslam_segments_labels(sg, buf.ctypes.data_as(C.c_void_p)) == ppf.OSLAM_E_INVALID      # no image
    assert L.oslam_segments_destroy(None) == ppf.OSLAM_E_INVALID


def test_scene_from_view_takes_planes_or_segments(built_lib, ppf):
    with pytest.raises(TypeError):
        ppf.Scene.from_view(object(), planes=object(), segments=object())
    with pytest.raises(TypeError):
        ppf.find_segments(object(), params=ppf.default_segments_params(), max_step=0.1)
    with pytest.raises(ValueError):
        ppf.select_segments(object(), object(), mode="neither")


# ---------------------------------------------------------------- the restatement on the named inputs
def test_inputs_reach_every_branch_of_the_rule(small):
    cases, trace = small
    print("%d inputs; trace %s" % (len(cases), trace))
    for name, c in cases.items():
        r = c["res"]
        print("%-34s %3d x %-3d: %4d components, %4d candidates, %2d segments, %5d of %5d in pixels labelled%s" % (
            name, c["depth"].shape[1], c["depth"].shape[0], r["n_components"], r["n_candidates"], r["n_segments"],
            r["labelled"], r["valid_in"], ", LIMIT" if r["limit"] else ""))
    for k in SR.TRACE_KEYS:
        assert trace[k] > 0, (k, trace)
    sizes = {c["depth"].shape[::-1] for c in cases.values()}
    assert {(1, 1), (3, 3), (7, 5), (40, 1), (1, 40), (33, 9), (64, 32), (65, 33), (97, 70), (130, 67)} <= sizes
    assert {c["depth"].dtype for c in cases.values()} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert {c["params"].get("max_segments", 16) for c in cases.values()} >= {2, 16, 64}
    assert any(c["planes"] is not None for c in cases.values())


def test_named_inputs_do_what_their_names_say(small):
    cases, _ = small
    res = lambda n: cases[n]["res"]
    for n in ("full_97x70", "serpentine_130x67", "comb_97x70"):
        r = res(n)
        assert r["n_components"] == r["n_segments"] == 1 and r["labelled"] == r["valid_in"], n
        assert r["records"]["root"][0] == 0 and (r["roots"][cases[n]["z"] > 0] == 0).all(), n
    assert res("full_97x70")["records"]["sides"][0] == 15
    serp = cases["serpentine_130x67"]
    assert serp["z"][66, 129] > 0 and serp["res"]["roots"][66, 129] == 0        # the far end, in the last tile
    assert res("spirals_65x33")["n_components"] == 2
    ring = res("ring_and_island_40x36")
    assert ring["n_segments"] == 2 and sorted(int(s) for s in ring["records"]["sides"]) == [0, 15]
    assert res("diagonal_blobs_65x40")["n_components"] == 5
    chk = res("checkerboard_64x32")
    assert chk["n_candidates"] == 1024 and chk["n_segments"] == 64 and (chk["records"]["pixels"] == 1).all()
    assert list(chk["records"]["root"]) == sorted(chk["records"]["root"]) and chk["records"]["root"][1] == 2   # ties: by root
    lim = res("checkerboard_limit_130x67")
    assert lim["limit"] and lim["n_components"] == lim["n_candidates"] == 4355 > SR.CANDIDATES and lim["labels"] is None
    for sfx in ("_x", "_y"):
        for n in ("steps_exact", "steps_rel"):
            r = res(n + sfx)
            # joined at exactly the gate, cut one ulp above it, inside a tile and on the seam
            assert sorted(int(p) for p in r["records"]["pixels"]) == [20, 25, 30, 55, 75, 130], (n, sfx)
        assert res("steps_exact" + sfx)["roots"].tobytes() == res("steps_rel" + sfx)["roots"].tobytes()
    # the pair that a fused multiply-add decides differently: the rule's two roundings against the exact sum
    za, zb = (F(x) for x in SI.fma_pair())
    two = F(F(0.05) + F(F(0.01) * za))
    one = F(float(F(0.05)) + float(F(0.01)) * float(za))
    assert two != one and bool(F(zb - za) <= two) != bool(F(zb - za) <= one)
    assert res("fma_pair_40x5")["n_components"] == (2 if F(zb - za) <= two else 4)
    assert res("split_by_holes_37x21")["n_components"] == 2
    eq = res("two_equal_33x9")
    assert list(eq["records"]["pixels"]) == [9, 9] and eq["records"]["root"][0] < eq["records"]["root"][1]
    assert eq["labels"][1, 20] == 0 and eq["labels"][5, 2] == 1
    ex = res("exact_and_short_33x9")
    assert ex["n_components"] == 2 and ex["n_candidates"] == 1 and ex["records"]["pixels"][0] == 9 == cases["exact_and_short_33x9"]["params"]["min_pixels"]
    cap = res("patchwork_cap_65x33")
    assert cap["n_candidates"] > cap["n_segments"] == 2 and cap["labelled"] < cap["valid_in"]
    far = cases["far_off_axis_40x5"]
    # 15 columns of 40 lie within the bound: the centroid is theirs alone, the box and the count are everyone's
    assert far["res"]["records"]["pixels"][0] == 200 and far["res"]["records"]["u1"][0] == 39
    assert abs(float(far["res"]["records"]["centroid"][0][0]) - 9000.0 * 7.0) < 1.0 < 9000.0 * 19.5
    pl = cases["room_corner_planes_37x21"]
    assert (pl["plane_labels"] >= 0).sum() > 0 and not (pl["res"]["roots"][pl["plane_labels"] >= 0] >= 0).any()
    assert pl["res"]["n_segments"] >= 1                               # the sphere


def test_restatement_properties(small):
    cases, _ = small
    for name, c in cases.items():
        r, z = c["res"], c["z"]
        inn = z > 0
        if c["plane_labels"] is not None:
            inn = inn & (c["plane_labels"] < 0)
        roots = r["roots"]
        assert ((roots >= 0) == inn).all() and r["valid_in"] == int(inn.sum()), name
        idx = np.arange(z.size).reshape(z.shape)
        assert (roots[inn] <= idx[inn]).all() and (roots.ravel()[roots[inn]] == roots[inn]).all(), name
        assert r["n_components"] == int((roots == idx).sum()), name
        # a plain flood fill agrees: the components are the transitive closure of the edges
        assert np.array_equal(roots, flood(z, inn, c)), name
        if r["limit"]:
            continue
        lab, rec = r["labels"], r["records"]
        assert lab.min() >= -1 and lab.max() == r["n_segments"] - 1 and not (lab[~inn] >= 0).any(), name
        assert [int((lab == k).sum()) for k in range(r["n_segments"])] == [int(x) for x in rec["pixels"]], name
        key = [(-int(p), int(q)) for p, q in zip(rec["pixels"], rec["root"])]
        assert key == sorted(key) and len(set(key)) == len(key), name
        for k in range(r["n_segments"]):
            vv, uu = np.nonzero(lab == k)
            assert (rec["u0"][k], rec["v0"][k], rec["u1"][k], rec["v1"][k]) == (uu.min(), vv.min(), uu.max(), vv.max()), name
            assert rec["root"][k] == idx[lab == k].min(), name
        for only in (-1, r["n_segments"] - 1):
            zr, (vin, obj, kept) = SR.select(z, lab, "remove", only)
            zk, (vin2, obj2, kept2) = SR.select(z, lab, "keep", only)
            assert vin == vin2 == int((z > 0).sum()) and obj == obj2 == kept2 and kept + kept2 == vin, name
            assert np.array_equal(zr + zk, z) and not (zr * zk).any(), name
        again, _, _ = SI.restate(c)
        assert all(again[k].tobytes() == r[k].tobytes() for k in ("roots", "labels", "records")), name


def flood(z, inn, case):
    """Components by a stack-based flood fill over the same gate, pixel by pixel: the slow definition."""
    h, w = z.shape
    step = case["params"].get("max_step", 0.0) or case["max_jump"]
    rel = case["params"].get("rel_step", 0.0)
    roots = np.full((h, w), -1, np.int32)
    for v0, u0 in zip(*np.nonzero(inn)):
        if roots[v0, u0] >= 0:
            continue
        root, stack = v0 * w + u0, [(v0, u0)]
        roots[v0, u0] = root
        while stack:
            v, u = stack.pop()
            for dv, du in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                y, x = v + dv, u + du
                if 0 <= y < h and 0 <= x < w and inn[y, x] and roots[y, x] < 0 and SR.gate(z[v, u], z[y, x], step, rel):
                    roots[y, x] = root
                    stack.append((y, x))
    return roots


def test_centroid_sums_cannot_overflow():
    """The header's proof in numbers: |q| <= 2^30 after the float range test, w * h <= 2^28 pixels."""
    q = int(np.rint(SR.BOUND))
    assert q == 1 << 30 and q * (1 << 28) == 1 << 58 < (1 << 63) - 1 and q < (1 << 31) - 1
    assert 16384 * 16384 == 1 << 28
    assert int(np.rint(np.nextafter(SR.BOUND, F(0)))) <= q


# ---------------------------------------------------------------- the union-find header as a program of its own
@pytest.fixture(scope="module")
def edge_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("seg_union") / "edges.txt"
    cases = SI.small_cases()
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for c in cases:
            n, a, b, roots = SI.edges_of(c)
            f.write("%d %d\n" % (n, len(a)))
            f.write("".join("%d %d\n" % (x, y) for x, y in zip(a.tolist(), b.tolist())))
            f.write(" ".join(str(x) for x in roots.ravel().tolist()) + "\n")
    return str(path), len(cases)


@pytest.mark.parametrize("name,flags", [
    ("seg_union_check", ["-O2"]),
    ("seg_union_check_san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all"]),
])
def test_union_find_header_under_threads(edge_file, name, flags):
    path, n_cases = edge_file
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-g", "-std=gnu11", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "seg_union_check.c")] + flags + ["-o", out], check=True)
    r = subprocess.run([out, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and ("seg_union_check ok: %d cases" % n_cases).encode() in r.stdout, (
        r.returncode, r.stdout.decode()[-500:], r.stderr.decode()[-2000:])


# ---------------------------------------------------------------- the calibration room
def test_room_objects_are_segments_with_the_defaults(pkg):
    for f, size in SC.FRAMES:
        res, objs = SC.run(f, size)
        print("frame %d %s: %d in pixels, %d components, %d of min_pixels or more; objects (pixels, segment, completeness, "
              "purity) %s" % (f, size, res["valid_in"], res["n_components"], res["n_candidates"],
                              [None if o is None else (o["pixels"], o["segment"], round(o["completeness"], 3),
                                                       round(o["purity"], 3)) for o in objs]))
        assert res["n_candidates"] <= 8, (f, size)
        assert (objs[0] is None) == (f == 9), (f, size)
        for k in (1, 2):
            assert objs[k]["completeness"] >= 0.94 and objs[k]["purity"] >= 0.95, (f, size, k, objs[k])
        if objs[0] is not None:
            assert objs[0]["completeness"] >= 0.70 and objs[0]["purity"] >= 0.95, (f, size, objs[0])
        assert len({o["segment"] for o in objs if o is not None}) == len([o for o in objs if o is not None])


def test_calibration_table_holds(pkg):
    rows = SC.table()
    print(SC.fmt(rows))
    assert len(rows) == 8
    cell = {(r["max_step"], r["rel_step"]): r for r in rows}
    d = cell[(0.08, 0.0)]                                            # the stream camera's max_jump: the default gate
    assert d["obj12"][0] >= 0.94 and d["obj12"][1] >= 0.95 and d["obj0"][0] >= 0.70 and d["obj0"][1] >= 0.95
    assert max(d["segments"]) <= 8
    # under a gate of 0.02 the objects crumble
    assert cell[(0.02, 0.0)]["components"][0] == 174 and cell[(0.02, 0.0)]["obj12"][0] < 0.6
    assert cell[(0.05, 0.0)]["obj12"][0] < d["obj12"][0]
    # a wider gate never splits more
    for rs in SC.REL_STEPS:
        comps = [sum(cell[(g, rs)]["components"]) for g in SC.GATES]
        assert comps == sorted(comps, reverse=True)
