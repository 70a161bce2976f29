"""GPU: the segments stage (oslam_view_segments, oslam_view_select_segments) against the numpy restatement of
tests/segments_ref.py on the named inputs of tests/segments_inputs.py, byte for byte: the root image, the label image,
the record words, the result counts, the launch count and the selected views with their counters; then once end to end
on frame 0 of the calibration room at 640 x 480.

Mutations the comparisons catch (mutation: input -> the bytes that change):
  - seams merged in one direction only (the vertical or the horizontal borders left out of k_seg_seam): serpentine_130x67,
    comb_97x70, full_97x70, steps_*_x against steps_*_y -> roots (a component falls apart at the tile border), n_components,
    records;
  - a union that links the lower root under the higher one: comb_97x70, serpentine_130x67 and every patchwork of more than
    one tile -> roots (a component's root is no longer its smallest index; find stops early where L[i] > i);
  - a flatten that stops after one hop: serpentine_130x67 (its chain of seam merges is dozens of tiles long), comb_97x70
    -> roots, the counts per root, records;
  - `<` for `<=` in the gate: steps_exact_x / _y and steps_rel_x / _y (steps of exactly the gate, inside a tile and on a
    seam) -> roots, six components become eight;
  - a fused multiply-add in the rel_step gate: fma_pair_40x5 (a pair, inside a tile and on a seam, that the two roundings
    and the single rounding decide differently) -> roots, n_components;
  - 8-connectivity: diagonal_blobs_65x40 (corners that meet at a tile corner and inside a tile, both diagonals),
    checkerboard_64x32 (1024 components become one), spirals_65x33 -> roots, n_components;
  - a rank tie broken by the higher root: checkerboard_64x32 (1024 candidates of one pixel, 64 kept), two_equal_33x9
    -> record words, labels;
  - a tile row or column missed at a ragged edge: every image whose size is no multiple of 32 (65x33, 97x70, 130x67,
    33x9, 7x5, 40x1, 1x40) -> roots and labels of the last row or column;
  - counts added per pixel to the local root rather than the final root, or the tile's count added twice:
    serpentine_130x67, comb_97x70, full_97x70 (one component over many tiles) -> pixels of the records, n_candidates;
  - a component of exactly min_pixels refused: exact_and_short_33x9 -> n_candidates, records;
  - a pixel beyond the centroid's bound clamped, or left out of the count or the box as well: far_off_axis_40x5 -> record
    words;
  - plane pixels not taken out, or taken out of the labels only: room_corner_planes_*, the room frames -> roots, valid_in;
  - ranks beyond max_segments labelled: patchwork_cap_65x33 and every patchwork with more than 16 candidates -> labels;
  - the list of candidates written past its end: checkerboard_limit_130x67 -> the error code and both counts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planes_inputs as PI  # noqa: E402
import refine_ref  # noqa: E402
import segments_calib as SC  # noqa: E402
import segments_inputs as SI  # noqa: E402
import segments_ref as SR  # noqa: E402
import track_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = SI.small_cases()
LIMIT = "checkerboard_limit_130x67"


@pytest.fixture(scope="module")
def wanted(synth):
    """name -> (case, the restatement's result, its z image): computed once, shared and left unchanged."""
    out = {}
    for c in SMALL + SI.room_cases(synth):
        res, z, _ = SI.restate(c)
        out[c["name"]] = (c, res, z)
    assert sorted(n for n in out if n.startswith("room_f")) == sorted(SI.ROOM_NAMES)
    return out


def find(ppf, view, case, **kw):
    pl = ppf.find_planes(view, **case["planes"]) if case["planes"] is not None else None
    try:
        return ppf.find_segments(view, pl, **dict(case["params"], **kw))
    finally:
        if pl is not None:
            pl.close()


def same(sg, res, name):
    roots, lab = sg.roots(), sg.labels()
    assert roots.tobytes() == res["roots"].tobytes(), (name, np.argwhere(roots != res["roots"])[:8])
    assert lab.tobytes() == res["labels"].tobytes(), (name, np.argwhere(lab != res["labels"])[:8])
    assert len(sg.segments) == res["n_segments"], (name, sg.segments, res["records"])
    assert sg.records.tobytes() == res["records"].tobytes(), (name, sg.segments, res["records"])
    r = sg.result
    got = tuple(r[k] for k in ("n_segments", "n_components", "n_candidates", "valid_in", "labelled"))
    assert got == tuple(res[k] for k in ("n_segments", "n_components", "n_candidates", "valid_in", "labelled")), (name, r)
    assert r["launches"] == SR.LAUNCHES == 6, (name, r)
    return roots, lab, sg.records


@pytest.mark.parametrize("name", [c["name"] for c in SMALL if c["name"] != LIMIT] + SI.ROOM_NAMES)
def test_segments_equal_restatement(built_lib, ppf, wanted, name):
    case, res, z = wanted[name]
    view = SI.view_of(ppf, case)
    sg = find(ppf, view, case)
    print("%s: %d components, %d candidates, segments %s, %d of %d in pixels labelled, %d launches, %.3f ms" % (
        name, sg.result["n_components"], sg.result["n_candidates"], [(s["pixels"], s["root"]) for s in sg.segments[:6]],
        sg.result["labelled"], sg.result["valid_in"], sg.result["launches"], sg.result["ms_total"]))
    first = same(sg, res, name)
    # a second call gives the same bytes
    pl = ppf.find_planes(view, **case["planes"]) if case["planes"] is not None else None
    sg2 = ppf.find_segments(view, pl, params=ppf.default_segments_params(**case["params"]))
    second = same(sg2, res, name)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    sg2.close()
    if pl is not None:
        pl.close()

    cam1 = dict(case["cam"], depth_scale=1.0)
    n = res["n_segments"]
    modes = [("remove", -1), ("keep", -1)] + ([("remove", n - 1), ("keep", 0)] if n else [])
    for mode, only in modes:
        out = ppf.select_segments(view, sg, mode, only)
        wz, wcnt = SR.select(z, res["labels"], mode, only)
        _, gz = ppf.view_maps(out)
        m = out.mask_result
        assert gz.tobytes() == wz.tobytes(), (name, mode, only)
        assert (m["valid_in"], m["object_pixels"], m["valid_out"], m["launches"]) == wcnt + (1,), (name, mode, only, m, wcnt)
        # a genuine view: its cloud is the cloud of the restated image's maps
        po, no = ppf.view_to_cloud(out)
        wp, wn = K.cloud_of_maps(*K.view_maps(wz, cam1, case["max_jump"]))
        assert po.tobytes() == wp.tobytes() and no.tobytes() == wn.tobytes(), (name, mode, only, len(po), len(wp))
        cam, w, h = ppf.view_camera(out)
        cam0, w0, h0 = ppf.view_camera(view)
        assert (w, h) == (w0, h0) and bytes(cam) == bytes(cam0)
        out.close()
    for only in (n, n + 7, -2):
        with pytest.raises(ppf.OslamError) as e:
            ppf.select_segments(view, sg, "keep", only)
        assert e.value.code == ppf.OSLAM_E_INVALID
    sg.close()
    view.close()


def test_more_candidates_than_the_list_holds(built_lib, ppf, wanted):
    """4355 components of one pixel with min_pixels 1: OSLAM_E_LIMIT, both counts, nothing else written."""
    import ctypes as C
    case, res, _ = wanted[LIMIT]
    assert res["limit"] and res["n_candidates"] == 4355
    view = SI.view_of(ppf, case)
    with pytest.raises(ppf.OslamError) as e:
        find(ppf, view, case)
    assert e.value.code == ppf.OSLAM_E_LIMIT and "4355 of 4355" in str(e.value)
    r = ppf.SegmentsResult()
    C.memset(C.byref(r), 0xA5, C.sizeof(r))
    before = bytes(r)
    h = C.c_void_p(1)
    p = ppf.default_segments_params(**case["params"])
    assert ppf.lib().oslam_view_segments(view._h, None, C.byref(p), C.byref(h), C.byref(r)) == ppf.OSLAM_E_LIMIT
    assert not h.value and (r.n_components, r.n_candidates) == (res["n_components"], res["n_candidates"])
    r.n_components, r.n_candidates = 0xA5A5A5A5, 0xA5A5A5A5
    assert bytes(r) == before
    # with min_pixels 2 the same image has no candidate at all, and the call succeeds
    sg = find(ppf, view, case, min_pixels=2)
    assert sg.result["n_components"] == 4355 and sg.result["n_candidates"] == 0 and not sg.segments
    assert (sg.labels() == -1).all()
    sg.close()
    view.close()


def test_segments_of_another_view_are_refused(built_lib, ppf, wanted):
    a, b = wanted["split_by_holes_37x21"][0], wanted["patchwork_7x5_f32"][0]
    va, vb = SI.view_of(ppf, a), SI.view_of(ppf, b)
    sg = ppf.find_segments(va)
    pl = ppf.find_planes(va)
    with pytest.raises(ppf.OslamError) as e:
        ppf.select_segments(vb, sg)
    assert e.value.code == ppf.OSLAM_E_INVALID and "size" in str(e.value)
    with pytest.raises(ppf.OslamError) as e:
        ppf.find_segments(vb, pl)
    assert e.value.code == ppf.OSLAM_E_INVALID and "size" in str(e.value)
    with pytest.raises(ppf.OslamError) as e:
        ppf.find_segments(va, max_step=-1.0)
    assert e.value.code == ppf.OSLAM_E_INVALID
    with pytest.raises(TypeError):
        ppf.Scene.from_view(va, pl, segments=sg)
    for x in (sg, pl, va, vb):
        x.close()


def test_recognition_on_the_rooms_segments(built_lib, ppf, synth, wanted):
    """Frame 0 of the room at 640 x 480: find_planes, find_segments(view, planes), and for each of the room's three objects
    the scene of the segment that holds most of its pixels, with the chain align + refine + verify (against the original
    view) of that object's model on it.  For an object whose segment holds at least 0.95 of its pixels (objects 1 and 2 by
    the calibration) everything the reduced scene of DESIGN.md 7za finds the segment scene finds, with a pose error within a
    quarter above the reduced scene's or under the refinement's stop floor.  Object 0 (0.88 of its pixels in its segment)
    and every model against every foreign segment are printed, not asserted.  Measured on one MI355X: DESIGN.md 7zb."""
    case, res, _ = wanted["room_f0_640x480"]
    view = SI.view_of(ppf, case)
    models, d, truth = PI.room_models(ppf, synth)
    pl = ppf.find_planes(view)
    sg = ppf.find_segments(view, pl)
    lab = sg.labels()
    assert lab.tobytes() == res["labels"].tobytes()
    masks = SC.frame(0, "full")[3]
    own, share = [], []
    for k in range(3):
        ls = lab[masks[k]]
        own.append(int(np.bincount(ls[ls >= 0]).argmax()))
        share.append(float((ls == own[k]).mean()))
    print("segments %s; objects' segments %s holding %s of their pixels" % (
        [(s["pixels"], s["box"]) for s in sg.segments], own, [round(s, 3) for s in share]))
    assert len(set(own)) == 3 and share[1] >= 0.95 and share[2] >= 0.95
    reduced = ppf.Scene.from_view(view, pl, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
    b = PI.chain(ppf, models, reduced, view)
    rp = ppf.default_refine_params()
    floor_rot, floor_trans = np.degrees(rp.stop_rot), rp.stop_trans * d
    scenes = [ppf.Scene.from_view(view, segments=sg, only=own[k], leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
              for k in range(3)]
    print("scene points after the voxel grid (leaf %.4f): reduced %d, segments %s" % (
        d, reduced.numPoints(), [s.numPoints() for s in scenes]))
    err = lambda x, k: refine_ref.pose_error(x["T"], truth[k]) if x["T"].any() else (float("nan"), float("nan"))
    for k in range(3):
        s = PI.chain(ppf, [models[k]], scenes[k], view)[0]
        (rb, tb), (rs, ts) = err(b[k], k), err(s, k)
        print("object %d: reduced scene found %s, error %.4f deg %.5f m; its segment's scene found %s, error %.4f deg %.5f m" % (
            k, b[k]["found"], rb, tb, s["found"], rs, ts))
        for j in range(3):
            if j != k:
                print("  model %d against object %d's segment: found %s" % (k, j, PI.chain(ppf, [models[k]], scenes[j], view)[0]["found"]))
        if share[k] >= 0.95 and b[k]["found"]:
            assert s["found"], k
            assert rs <= max(1.25 * rb, floor_rot) and ts <= max(1.25 * tb, floor_trans), (k, (rb, tb), (rs, ts))
    for x in models + scenes + [reduced, sg, pl, view]:
        x.close()
