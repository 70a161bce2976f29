"""GPU: the render stage (k_render_splat, k_render_resolve, k_view_mask) against the numpy restatement
(tests/render_ref.py) on the inputs of tests/render_edge_inputs.py, bit for bit in the z image, the labels, every
counter and the masked view in both modes; then the render at work: a masked view is a genuine view, the two modes
partition a frame, and masking a moving object out of two frames repairs the camera motion estimated between them.
tests/test_render_edge_inputs.py asserts on the CPU that the edge inputs reach their branches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_edge_inputs as E  # noqa: E402
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_JUMP = 0.05


def camera_of(ppf, cam, max_jump=MAX_JUMP):
    return ppf.Camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], 1.0, cam["z_min"], cam["z_max"], max_jump)


def view_of(ppf, img, cam, max_jump=MAX_JUMP):
    return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=max_jump)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def z_of(ppf, view):
    return ppf.view_maps(view)[1]


def device_render(ppf, c):
    """-> (Render, the models it borrows)"""
    models = [ppf.Model(p, n, d_dist=d) for p, n, d in c["clouds"]]
    r = ppf.render([models[m] for m in c["member"]], c["T"], (camera_of(ppf, c["cam"]), c["w"], c["h"]),
                   ppf.default_render_params(**c["params"]))
    return r, models


def assert_render_equals(ppf, r, ref, name):
    z, lab = z_of(ppf, r.view), r.labels()
    assert np.array_equal(lab, ref["labels"]), (name, np.argwhere(lab != ref["labels"])[:6])
    assert np.array_equal(bits(z), bits(ref["z"])), (name, np.argwhere(bits(z) != bits(ref["z"]))[:6])
    assert [x["drawn"] for x in r.results] == ref["drawn"].tolist(), name
    assert [x["pixels"] for x in r.results] == ref["pixels"].tolist(), name


def assert_masks_equal(ppf, view, z_o, r, ref, name, settings=E.MASK_SETTINGS):
    for s in settings:
        mv, res = ppf.mask_view(view, r, "keep" if s["mode"] == R.KEEP else "remove", s["dilate"], s["only"])
        want, cnt = R.mask(z_o, ref, s["mode"], s["dilate"], s["only"])
        got = z_of(ppf, mv)
        mv.close()
        assert np.array_equal(bits(got), bits(want)), (name, s, np.argwhere(bits(got) != bits(want))[:6])
        assert {k: res[k] for k in cnt} == cnt and res["launches"] == 1, (name, s, res, cnt)


@pytest.fixture(scope="module")
def cases(synth):
    """every edge input with the restatement's answer, computed once"""
    return [(c, E.reference(c)) for c in E.render_cases(synth)]


def test_edge_inputs_equal_restatement(built_lib, ppf, cases):
    launches = {}
    for c, ref in cases:
        r, models = device_render(ppf, c)
        assert_render_equals(ppf, r, ref, c["name"])
        launches[c["name"]] = (len(c["member"]), {x["launches"] for x in r.results})
        img = E.observed(c, ref)
        view = view_of(ppf, img, c["cam"])
        z_o = z_of(ppf, view)
        assert np.array_equal(bits(z_o), bits(R.V.view_z(img, 1.0, c["cam"]["z_min"], c["cam"]["z_max"])))
        settings = E.MASK_SETTINGS if c["w"] == E.W else [s for s in E.MASK_SETTINGS if s["dilate"] != 8]
        assert_masks_equal(ppf, view, z_o, r, ref, c["name"], settings)
        view.close()
        r.close()
        for m in models:
            m.close()
    # the cost of a call does not depend on the number of hypotheses; an empty render skips the splat
    assert launches["border default"] == (1, {2}) and launches["hypotheses 1024"] == (1024, {2}), launches
    assert launches["all skipped"] == (2, {1}), launches


def test_mask_by_hand_equals_restatement(built_lib, ppf):
    c, ref, img, names = E.mask_case()
    r, models = device_render(ppf, c)
    assert_render_equals(ppf, r, ref, c["name"])
    view = view_of(ppf, img, c["cam"])
    z_o = z_of(ppf, view)
    settings = E.MASK_SETTINGS + [dict(mode=m, dilate=2, only=o) for m in (R.REMOVE, R.KEEP) for o in (0, 1)]
    assert_masks_equal(ppf, view, z_o, r, ref, c["name"], settings)
    with pytest.raises(ppf.OslamError) as e:                      # the render has two hypotheses
        ppf.mask_view(view, r, "keep", 2, only=2)
    assert e.value.code == ppf.OSLAM_E_INVALID
    other = view_of(ppf, img, dict(c["cam"], fx=c["cam"]["fx"] + 0.5))
    small = view_of(ppf, img[:-1], c["cam"])
    for v in (other, small):                                       # another camera, another size
        with pytest.raises(ppf.OslamError) as e:
            ppf.mask_view(v, r)
        assert e.value.code == ppf.OSLAM_E_INVALID
        v.close()
    view.close()
    r.close()
    for m in models:
        m.close()


def test_database_render_and_masked_view_is_a_view(built_lib, ppf, synth, cases):
    c, ref = [x for x in cases if x[0]["name"].startswith("sizes")][0]
    models = [ppf.Model(p, n, d_dist=d) for p, n, d in c["clouds"]]
    db = ppf.Database(models)
    cam = camera_of(ppf, c["cam"])
    a = ppf.render([models[m] for m in c["member"]], c["T"], (cam, c["w"], c["h"]))
    b = db.render((cam, c["w"], c["h"]), c["member"], c["T"])
    assert np.array_equal(a.labels(), b.labels()) and np.array_equal(bits(z_of(ppf, a.view)), bits(z_of(ppf, b.view)))
    assert [(x["drawn"], x["pixels"]) for x in a.results] == [(x["drawn"], x["pixels"]) for x in b.results]
    assert_render_equals(ppf, b, ref, "database")
    # a render takes a view's camera too, and the render's own view goes wherever a view goes
    img = E.observed(c, ref)
    view = view_of(ppf, img, c["cam"])
    again = ppf.render([models[m] for m in c["member"]], c["T"], view)
    assert np.array_equal(again.labels(), ref["labels"])
    ver = models[2].verify(again.view, c["T"][2])
    assert ver["supported"] > 0 and ver["conflict"] == 0, ver
    z_o = z_of(ppf, view)
    for mode, name in ((R.REMOVE, "remove"), (R.KEEP, "keep")):
        mv, _ = ppf.mask_view(view, a, name)
        want, _ = R.mask(z_o, ref, mode)
        gp, gn = ppf.view_to_cloud(mv)
        wp, wn = ppf.depth_to_cloud(want, c["cam"]["fx"], c["cam"]["fy"], c["cam"]["cx"], c["cam"]["cy"], depth_scale=1.0,
                                    z_min=c["cam"]["z_min"], z_max=c["cam"]["z_max"], max_jump=MAX_JUMP)
        assert len(gp) == len(wp) and np.array_equal(bits(gp), bits(wp)) and np.array_equal(bits(gn), bits(wn)), name
        mv.close()
    # the tracker renders its live tracks through the database: three detections make three tracks in id order
    tr = ppf.Tracker(db)
    assert tr.render(view) is None
    tr.update([dict(model=k, T=c["T"][k]) for k in range(3)])
    live = tr.render(view)
    assert np.array_equal(live.labels(), ref["labels"]) and [x["pixels"] for x in live.results] == ref["pixels"].tolist()
    for x in (live, tr, again, a, b, view, db):
        x.close()
    for m in models:
        m.close()


# ---------------------------------------------------------------- the render at work: a moving object before static planes
MARGIN = 1.5            # tests/test_render_host.py: how far (b) may lie from (c), with the CPU's numbers and the reasoning


@pytest.fixture(scope="module")
def world(synth, oracle):
    import render_world as RW
    w = RW.make(synth, oracle)
    w["RW"] = RW
    return w


def world_views(ppf, w, key):
    RW = w["RW"]
    return [view_of(ppf, img, RW.CAM, RW.MAX_JUMP) for img in w[key]]


def test_modes_partition_the_frame_and_the_object_view_verifies(built_lib, ppf, world):
    RW = world["RW"]
    gp, gn, d = world["cloud"]
    model = ppf.Model(gp, gn, d_dist=d)
    view = world_views(ppf, world, "frames")[0]
    T = world["T_obj"][0]
    r = ppf.render([model], T[None], view)
    ref = R.render([world["cloud"]], T[None], RW.FCAM, RW.W, RW.H)
    assert_render_equals(ppf, r, ref, "world")
    rem, cr = ppf.mask_view(view, r, "remove")
    keep, ck = ppf.mask_view(view, r, "keep")
    z_o = z_of(ppf, view)
    assert cr["valid_in"] == ck["valid_in"] == cr["valid_out"] + ck["valid_out"] == int((z_o > 0).sum())
    assert ck["valid_out"] == ck["object_pixels"] == cr["object_pixels"] > 0.12 * cr["valid_in"]
    zr, zk = z_of(ppf, rem), z_of(ppf, keep)
    assert np.array_equal(bits(np.where(zk > 0, zk, zr)), bits(z_o)) and not ((zk > 0) & (zr > 0)).any()
    full, alone = model.verify(view, T), model.verify(keep, T)
    assert alone["conflict"] <= full["conflict"] and alone["supported"] > 0.8 * full["supported"], (full, alone)
    for x in (rem, keep, r, view, model):
        x.close()


def test_masking_the_moving_object_repairs_egomotion_and_fusion(built_lib, ppf, world):
    """(a) raw frames, (b) the object masked out with a render at its true pose, (c) frames without the object.
    On the CPU (tests/test_render_host.py): (a) 0.012513 m 0.0017324 rad, (b) 0.002205 m 0.0003007 rad, (c) 0.002281 m
    0.0003035 rad; measured on the MI355X: the same to every digit printed.  (b) must beat (a) and lie within
    MARGIN = 1.5 times (c) in both (the mask takes a fifth of the pixels: about 1 / sqrt(0.8) = 1.12 for a least-squares
    estimate, the rest is headroom for the silhouette; (a) is 5.5 times (c)).  DESIGN.md 7p holds the table."""
    import volume_ref
    RW = world["RW"]
    gp, gn, d = world["cloud"]
    model = ppf.Model(gp, gn, d_dist=d)
    raw, empty = world_views(ppf, world, "frames"), world_views(ppf, world, "empty")
    renders = [ppf.render([model], world["T_obj"][f][None], raw[f]) for f in range(2)]
    masked = [ppf.mask_view(raw[f], renders[f], "remove")[0] for f in range(2)]
    err = {}
    for name, pair in (("raw", raw), ("masked", masked), ("empty", empty)):
        T, res = ppf.egomotion(pair[0], pair[1])
        err[name] = ppf.ht_dist(T, world["truth"])
        print("%-6s %.6f m %.7f rad, overlap %.3f" % (name, err[name][0], err[name][1], res["overlap"]))
        assert res["ok"], (name, res)
    for k in (0, 1):
        assert err["masked"][k] < err["raw"][k], err
        assert err["masked"][k] <= MARGIN * err["empty"][k], err
    # fusion: the same two frames stepped into a volume with and without the object masked out.  Against the raw frame
    # the moving object costs the second step its overlap (restatement: 0.72 raw, 0.82 masked, below and above the
    # default min_overlap of 0.75); both runs take min_overlap 0.6 so that both integrate both frames.
    updated, pose_err = {}, {}
    p = ppf.default_egomotion_params(min_overlap=0.6)
    for name in ("all", "static"):
        vol = volume_ref.room_volume(0, cls=ppf.Volume)
        updated[name] = []
        for f in range(2):
            T, res = vol.step(raw[f], params=p, static=renders[f] if name == "static" else None)
            if name == "static":
                assert res["mask"]["object_pixels"] > 0 and res["mask"]["valid_out"] < res["mask"]["valid_in"], res
            else:
                assert res is None or "mask" not in res
            assert f == 0 or res["ok"], (name, res)
            updated[name].append(vol.last_integrate["updated"])
        pose_err[name] = ppf.ht_dist(np.linalg.inv(T.astype(np.float64)), world["truth"])
        vol.close()
    print("voxels updated per frame: all %s, static only %s; pose of frame 1: all %.6f m %.7f rad, static %.6f m %.7f rad"
          % (updated["all"], updated["static"], *pose_err["all"], *pose_err["static"]))
    assert all(s < a for s, a in zip(updated["static"], updated["all"])), updated
    assert pose_err["static"][0] < pose_err["all"][0] and pose_err["static"][1] < pose_err["all"][1], pose_err
    for x in masked + renders + raw + empty + [model]:
        x.close()
