"""GPU: the planes stage (oslam_view_planes, oslam_view_remove_planes) against the numpy restatement of
tests/planes_ref.py on the named inputs of tests/planes_inputs.py, byte for byte: the plane records, the label image,
the per-round counts and moments, the launch count and the reduced views with their counters; then once end to end on
frame 0 of the calibration room at 640 x 480.

Mutations the comparisons catch (each changes bytes that are compared on at least one named input):
  - a tie for the winner going to the highest index: the candidate and every later round of tie_corner_33x9 and of every
    image small enough for lattice nodes to coincide (7 x 5, 3 x 3, 33 x 9's rows);
  - labelling only pixels that have a normal: labels and pixels of every image (border rows and columns have none);
  - counting labelled or invalid pixels in the score: counts from round 1 on, holes_and_step's from round 0;
  - a count compared with min_pixels by <= instead of <: min_pixels_exact finds no plane;
  - ending the search without keeping the round's counts, or running a round after the end: counts and moments of
    staircase, thin_strip and min_pixels_one_short;
  - a pixel beyond the moments' bound clamped instead of left out, or left out of the labels too: far_plane's moments,
    support and labels;
  - a fused multiply-add or another grouping in a gate: counts on the room frames, where thousands of pixels lie within an
    ulp of a gate; a float sum in the moments: the moments;
  - a tile or a row missed at a ragged edge: every image whose size is no multiple of 256 pixels or of 32 x 8;
  - the normal not turned towards the camera, or d from p0 instead of the centroid: the records.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import planes_inputs as PI  # noqa: E402
import planes_ref as PR  # noqa: E402
import refine_ref  # noqa: E402
import track_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = PI.small_cases()
ROOM_NAMES = ["room_f0_320x240", "room_f5_320x240", "room_f0_640x480"]


@pytest.fixture(scope="module")
def wanted(synth):
    """name -> (case, the restatement's result, its z image): computed once, shared and left unchanged."""
    out = {}
    for c in SMALL + PI.room_cases(synth):
        res, z = PR.find_in_depth(c["depth"], c["cam"], c["max_jump"], **c["params"])
        out[c["name"]] = (c, res, z)
    assert sorted(n for n in out if n.startswith("room_f")) == sorted(ROOM_NAMES)
    return out


def same(pl, res, name):
    counts, moments = pl.rounds()
    assert len(pl.planes) == res["n_planes"], (name, pl.planes, res["planes"])
    assert pl.records.tobytes() == res["planes"].tobytes(), (name, pl.planes, res["planes"])
    assert counts.tobytes() == res["counts"].tobytes(), (name, np.argwhere(counts != res["counts"])[:8])
    assert moments.tobytes() == res["moments"].tobytes(), (name, moments, res["moments"])
    lab = pl.labels()
    assert lab.tobytes() == res["labels"].tobytes(), (name, np.argwhere(lab != res["labels"])[:8])
    r = pl.result
    assert (r["n_planes"], r["valid_in"], r["labelled"]) == (res["n_planes"], res["valid_in"], res["labelled"]), (name, r)
    return counts, moments, lab


@pytest.mark.parametrize("name", [c["name"] for c in SMALL] + ROOM_NAMES)
def test_planes_equal_restatement(built_lib, ppf, wanted, name):
    case, res, z = wanted[name]
    mp = case["params"].get("max_planes", 4)
    view = PI.view_of(ppf, case)
    pl = ppf.find_planes(view, **case["params"])
    print("%s: %d plane(s) %s, %d of %d valid pixels labelled, %d launches, %.3f ms" % (
        name, len(pl.planes), [(p["support"], p["pixels"], p["candidate"]) for p in pl.planes], pl.result["labelled"],
        pl.result["valid_in"], pl.result["launches"], pl.result["ms_total"]))
    first = same(pl, res, name)
    assert pl.result["launches"] == PR.launches(mp, built=True) == 4 * mp + 1
    # a second call gives the same bytes; the maps exist now
    pl2 = ppf.find_planes(view, params=ppf.default_planes_params(**case["params"]))
    second = same(pl2, res, name)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    assert pl2.result["launches"] == PR.launches(mp, built=False) == 4 * mp
    pl2.close()

    cam1 = dict(case["cam"], depth_scale=1.0)
    modes = [("remove", -1), ("keep", -1)] + ([("remove", res["n_planes"] - 1), ("keep", 0)] if res["n_planes"] else [])
    for mode, only in modes:
        out = ppf.remove_planes(view, pl, mode, only)
        wz, wcnt = PR.remove(z, res["labels"], mode, only)
        maps, gz = ppf.view_maps(out)
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
    for only in (res["n_planes"], res["n_planes"] + 7, -2):
        with pytest.raises(ppf.OslamError) as e:
            ppf.remove_planes(view, pl, "keep", only)
        assert e.value.code == ppf.OSLAM_E_INVALID
    pl.close()
    view.close()


def test_planes_of_another_view_are_refused(built_lib, ppf, wanted):
    a, b = wanted["one_plane_37x21_f32"][0], wanted["one_plane_7x5_f32"][0]
    va, vb = PI.view_of(ppf, a), PI.view_of(ppf, b)
    pl = ppf.find_planes(va)
    with pytest.raises(ppf.OslamError) as e:
        ppf.remove_planes(vb, pl)
    assert e.value.code == ppf.OSLAM_E_INVALID and "size" in str(e.value)
    with pytest.raises(ppf.OslamError) as e:
        ppf.find_planes(va, dist_tol=0.0)
    assert e.value.code == ppf.OSLAM_E_INVALID
    with pytest.raises(TypeError):
        ppf.find_planes(va, params=ppf.default_planes_params(), dist_tol=0.01)
    for x in (pl, va, vb):
        x.close()


def test_recognition_on_the_room_without_its_planes(built_lib, ppf, synth, wanted):
    """Frame 0 of the room at 640 x 480: the chain align + refine + verify (against the original view) of the room's three
    objects on the full scene and on Scene.from_view(view, planes), with the same leaf.  Every object the full scene finds
    the reduced scene finds, at least one is found, and a reduced pose error stays within a quarter above the full
    scene's (or under the refinement's own stop criterion, its convergence floor).  Measured on one MI355X: see
    DESIGN.md 7za."""
    case, res, _ = wanted["room_f0_640x480"]
    view = PI.view_of(ppf, case)
    models, d, truth = PI.room_models(ppf, synth)
    pl = ppf.find_planes(view)
    full = ppf.Scene.from_view(view, None, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
    reduced = ppf.Scene.from_view(view, pl, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
    n_before, n_after = len(ppf.view_to_cloud(view)[0]), None
    rv = ppf.remove_planes(view, pl)
    n_after = len(ppf.view_to_cloud(rv)[0])
    rv.close()
    print("scene points with a normal: %d before, %d after removal; after the voxel grid (leaf %.4f): %d and %d" % (
        n_before, n_after, d, full.numPoints(), reduced.numPoints()))
    assert n_after < n_before // 5 and reduced.numPoints() < full.numPoints()
    a, b = PI.chain(ppf, models, full, view), PI.chain(ppf, models, reduced, view)
    rp = ppf.default_refine_params()
    floor_rot, floor_trans = np.degrees(rp.stop_rot), rp.stop_trans * d
    errs = []
    for k in range(3):
        ea = refine_ref.pose_error(a[k]["T"], truth[k]) if a[k]["T"].any() else (float("nan"), float("nan"))
        eb = refine_ref.pose_error(b[k]["T"], truth[k]) if b[k]["T"].any() else (float("nan"), float("nan"))
        errs.append((ea, eb))
        print("object %d: full scene found %s, error %.4f deg %.5f m; reduced scene found %s, error %.4f deg %.5f m" % (
            k, a[k]["found"], ea[0], ea[1], b[k]["found"], eb[0], eb[1]))
    any_full = any(x["found"] for x in a)
    assert any(x["found"] for x in b)
    for k in range(3):
        (ra, ta), (rb, tb) = errs[k]
        if a[k]["found"]:
            assert b[k]["found"], k
            assert rb <= max(1.25 * ra, floor_rot) and tb <= max(1.25 * ta, floor_trans), (k, errs[k])
        elif b[k]["found"] and not any_full:
            # the full scene finds nothing at this leaf: the reduced scene is held to the truth alone (the reference's
            # acceptance test: 12 degrees, a tenth of the diameter)
            assert rb < 12.0 and tb < 0.1 * synth.bbox_extent(np.asarray(synth.make_model(k, 500)[0]) * E.OBJECT_SCALE), (k, errs[k])
    for x in models + [full, reduced, pl, view]:
        x.close()
