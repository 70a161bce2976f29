"""The named inputs of the planes stage's tests (tests/test_planes_host.py, tests/test_gpu_planes.py): analytic depth
images at the smallest sizes at which the kernels can still go wrong (ragged tiles, lattice nodes that coincide, one
pixel with a normal, no normal at all, more than one workgroup), and three frames of the calibration room.

A case is dict(name, depth, cam, max_jump, params): depth uint16 (millimetres) or float32 (metres), cam a dict with
fx fy cx cy depth_scale z_min z_max, params the fields of oslam_planes_params that differ from the defaults.
"""
import numpy as np

import camera_ref as E
import planes_ref as PR
import volume_ref as V

MAX_JUMP = 0.5                  # of the analytic images: at these sizes a slanted surface steps decimetres per pixel
ROOM_FRAMES = (0, 3, 5, 9)


def camera(w, h, f=None, depth_scale=1.0):
    f = float(f if f is not None else 0.8 * max(w, 8))
    return dict(fx=f, fy=f, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, depth_scale=depth_scale, z_min=0.1, z_max=20.0)


def cast(w, h, cam, planes=(), spheres=()):
    """z [h,w] float64 of the nearest surface along each pixel's ray (0 = nothing): planes (n, d) with n . p + d = 0,
    spheres (centre, radius)."""
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], axis=2)
    z = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for n, dd in planes:
            t = -dd / (d @ np.asarray(n, np.float64))
            z = np.where((t > 0) & (t < z), t, z)
        for c, rad in spheres:
            c = np.asarray(c, np.float64)
            a, b, cc = (d * d).sum(axis=2), -2.0 * (d @ c), float(c @ c) - rad * rad
            disc = b * b - 4 * a * cc
            t = (-b - np.sqrt(disc)) / (2 * a)
            z = np.where((disc > 0) & (t > 0) & (t < z), t, z)
    return np.where(np.isfinite(z), z, 0.0)


def as_image(z, kind):
    """float32 metres, or uint16 millimetres."""
    return z.astype(np.float32) if kind == "f32" else np.clip(np.rint(z * 1000.0), 0, 65535).astype(np.uint16)


def unit(n):
    n = np.asarray(n, np.float64)
    return n / np.linalg.norm(n)


def tilted_plane(w, h, kind, tilt=(0.3, -0.2, -1.0), depth=2.0):
    cam = camera(w, h, depth_scale=1.0 if kind == "f32" else 0.001)
    n = unit(tilt)
    return as_image(cast(w, h, cam, planes=[(n, -n[2] * depth)]), kind), cam


def corner_33x9(kind):
    """Two planes that meet in the centre column, mirror images of each other: p, n and every gate of the left half are
    the right half's with x negated, bit for bit, and the lattice columns 1, 3, .., 31 are their own mirror image, so node
    (a, b) and node (15 - a, b) tie exactly.  The lowest index must win."""
    w, h = 33, 9
    cam = camera(w, h, f=24.0, depth_scale=1.0 if kind == "f32" else 0.001)
    x = np.abs((np.arange(w, dtype=np.float64) - cam["cx"]) / cam["fx"])
    z = np.repeat((3.0 / (1.0 + 0.3 * x))[None, :], h, axis=0)      # the planes z (1 + 0.3 |x'|) = 3: a roof, its ridge at x = 0
    return as_image(z, kind), cam


def room_corner(w, h, kind):
    """A floor, a back wall, a side wall and a sphere before them."""
    cam = camera(w, h, f=0.5 * w, depth_scale=1.0 if kind == "f32" else 0.001)
    planes = [((0.0, -1.0, 0.0), 0.6), ((0.0, 0.0, -1.0), 2.5), ((1.0, 0.0, 0.0), 1.2)]
    return as_image(cast(w, h, cam, planes=planes, spheres=[((0.3, 0.3, 1.8), 0.3)]), kind), cam


def staircase(kind, w=64, h=16, steps=9):
    """Nine fronto-parallel steps 0.6 m apart, each seven or eight columns wide: more planes than a call can hold."""
    cam = camera(w, h, depth_scale=1.0 if kind == "f32" else 0.001)
    z = np.repeat((2.0 + 0.6 * np.minimum(np.arange(w) // (w // steps), steps - 1))[None, :], h, axis=0).astype(np.float64)
    return as_image(z, kind), cam


def thin_strip(kind, w=64, h=16):
    """Three valid rows of a fronto-parallel plane: only the middle one has normals, a line of points."""
    cam = camera(w, h, depth_scale=1.0 if kind == "f32" else 0.001)
    z = np.zeros((h, w))
    z[6:9] = 2.5
    return as_image(z, kind), cam


def holes_and_step(kind, w=37, h=21):
    """A tilted plane with seeded holes whose right part lies 0.8 m farther."""
    img, cam = tilted_plane(w, h, "f32")
    z = img.astype(np.float64)
    z[:, 22:] += 0.8
    z[np.random.default_rng(7).uniform(size=z.shape) < 0.08] = 0.0
    cam = dict(cam, depth_scale=1.0 if kind == "f32" else 0.001)
    return as_image(z, kind), cam


def far_plane(kind, w=64, h=16):
    """A fronto-parallel plane at 5 m seen with a wide lens: with dist_tol 1e-4 the scale is 160000 per metre and the
    bound 2^17 lies 0.82 m from the winner's point, inside the 10 m the image spans."""
    cam = camera(w, h, f=32.0, depth_scale=1.0 if kind == "f32" else 0.001)
    return as_image(np.full((h, w), 5.0), kind), cam


def _case(name, img_cam, **params):
    return dict(name=name, depth=img_cam[0], cam=img_cam[1], max_jump=MAX_JUMP, params=params)


def winner_count(case):
    """The count of round 0's winner under the case's other parameters (the restatement's)."""
    kw = dict(case["params"], max_planes=1, min_pixels=1)
    res, _ = PR.find_in_depth(case["depth"], case["cam"], case["max_jump"], **kw)
    return int(res["counts"][0].max())


def small_cases():
    out = []
    for kind in ("f32", "u16"):
        out.append(_case("one_plane_37x21_" + kind, tilted_plane(37, 21, kind)))
        out.append(_case("tie_corner_33x9_" + kind, corner_33x9(kind), min_normal_dot=0.95))
        for mp in (1, 4, 8):
            for lmd in (0.0, 0.95):
                out.append(_case("room_corner_37x21_%s_max%d_dot%g" % (kind, mp, lmd), room_corner(37, 21, kind), max_planes=mp,
                                 label_min_dot=lmd, min_pixels=12))
        out.append(_case("staircase_64x16_" + kind, staircase(kind), max_planes=8))
        out.append(_case("thin_strip_64x16_" + kind, thin_strip(kind)))
        out.append(_case("holes_and_step_37x21_" + kind, holes_and_step(kind)))
        out.append(_case("far_plane_64x16_" + kind, far_plane(kind), dist_tol=1e-4))
        out.append(_case("one_plane_7x5_" + kind, tilted_plane(7, 5, kind)))
        out.append(_case("one_normal_3x3_" + kind, tilted_plane(3, 3, kind)))
        out.append(_case("no_normals_40x1_" + kind, tilted_plane(40, 1, kind)))
        out.append(_case("room_corner_64x16_" + kind, room_corner(64, 16, kind), max_planes=4, min_pixels=12))
    # a winner with exactly min_pixels inliers is a plane, one with min_pixels - 1 ends the search
    base = _case("exact", tilted_plane(37, 21, "f32"))
    k = winner_count(base)
    out.append(_case("min_pixels_exact_37x21", tilted_plane(37, 21, "f32"), min_pixels=k))
    out.append(_case("min_pixels_one_short_37x21", tilted_plane(37, 21, "f32"), min_pixels=k + 1))
    return out


_ROOM = {}


def room_frame(synth, frame, size="small"):
    """Frame `frame` of camera_ref's room (seed 0) -> (uint16 image, cam dict); size "small" = 320 x 240
    (volume_ref.SMALL), "full" = 640 x 480 (the stream camera)."""
    key = (frame, size)
    if key not in _ROOM:
        if "world" not in _ROOM:
            _ROOM["world"], _ROOM["traj"] = E.make_world(synth, 0), E.trajectory(synth, 0)
        if size == "small":
            _ROOM[key] = (E.render(synth, _ROOM["world"], _ROOM["traj"][frame], **V.SMALL), dict(V.SMALL_CAM))
        else:
            _ROOM[key] = (E.render(synth, _ROOM["world"], _ROOM["traj"][frame]), dict(E.CAM))
    return _ROOM[key]


def room_planes_only(synth, frame):
    """The planes_only render of the same pose at 320 x 240."""
    key = ("planes_only", frame)
    if key not in _ROOM:
        if "bare" not in _ROOM:
            _ROOM["bare"] = E.make_world(synth, 0, planes_only=True)
        room_frame(synth, frame)
        _ROOM[key] = E.render(synth, _ROOM["bare"], _ROOM["traj"][frame], **V.SMALL)
    return _ROOM[key]


def view_of(ppf, case):
    cam = case["cam"]
    return ppf.View(case["depth"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], depth_scale=cam["depth_scale"], z_min=cam["z_min"],
                    z_max=cam["z_max"], max_jump=case["max_jump"])


# ---------------------------------------------------------------- the recognition chain of the end-to-end test and the bench
E2E_MODEL_POINTS = 1500
E2E_DF = 4


def room_models(ppf, synth):
    """The room's three objects as models: synth models 0, 1, 2 at camera_ref.OBJECT_SCALE, 1500 points each, all with
    model 0's d_dist (the scene's leaf too, as in tests/test_gpu_database.py) -> (models, d_dist, truth poses in frame 0's
    camera, which is the world's frame)."""
    clouds = []
    for k in range(3):
        pts, nrm = synth.make_model(k, E2E_MODEL_POINTS)
        clouds.append((np.ascontiguousarray(pts * np.float32(E.OBJECT_SCALE)), nrm))
    d = synth.d_dist_for(clouds[0][0], 0.05)
    models = [ppf.Model(p, n, d_dist=d) for p, n in clouds]
    return models, d, [E.object_pose(synth, 0, k) for k in range(3)]


def chain(ppf, models, scene, view):
    """Align, refine and verify every model against the scene, the verification against the original view ->
    [dict(T refined, found, verify result)]."""
    out = []
    for m in models:
        T = m.ppf_lookup(scene, allow_no_votes=True).copy()
        if not T.any():
            out.append(dict(T=T, found=False, verify=None))
            continue
        Tr, _ = m.refine(scene, T)
        r = m.verify(view, Tr)
        out.append(dict(T=np.array(Tr, np.float32), found=bool(r["found"]), verify=r))
    return out


def room_cases(synth):
    out = [dict(name="room_f%d_320x240" % f, depth=room_frame(synth, f)[0], cam=room_frame(synth, f)[1], max_jump=E.MAX_JUMP,
                params={}) for f in (0, 5)]
    img, cam = room_frame(synth, 0, "full")
    out.append(dict(name="room_f0_640x480", depth=img, cam=cam, max_jump=E.MAX_JUMP, params={}))
    return out
