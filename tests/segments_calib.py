"""The calibration of the segments stage, on the CPU with tests/segments_ref.py.

Frames 0, 3, 5 and 9 of camera_ref's room at 320 x 240 (volume_ref.SMALL) and frame 0 at 640 x 480, each after planes_ref
with its defaults.  Object k's pixels are the in pixels whose point lies within 0.75 m of the translation of
camera_ref.object_pose(synth, 0, k), taken into the frame's camera.  Per frame and object the row gives the share of the
object's pixels in the segment that holds most of them (completeness) and the share of that segment's pixels that are
the object's (purity), and the number of segments that pass the default min_pixels.  The table varies the gate over
{0.02, 0.05, 0.08, 0.12} m and rel_step over {0, 0.01}.

`python tests/segments_calib.py` prints the table; tests/test_segments_host.py asserts on it.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import camera_ref as E  # noqa: E402
import planes_inputs as PI  # noqa: E402
import planes_ref as PR  # noqa: E402
import segments_ref as SR  # noqa: E402

FRAMES = tuple((f, "small") for f in PI.ROOM_FRAMES) + ((0, "full"),)
GATES = (0.02, 0.05, 0.08, 0.12)
REL_STEPS = (0.0, 0.01)
OBJECT_RADIUS = 0.75
MIN_OBJECT_PIXELS = 50          # fewer in pixels than this: the object is out of view


def _synth():
    import importlib
    return importlib.import_module("objective-slam_amd").synth


@functools.lru_cache(maxsize=None)
def frame(f, size):
    """-> (z, cam, plane labels, [object pixel mask] * 3) of frame f after planes_ref with its defaults."""
    synth = _synth()
    img, cam = PI.room_frame(synth, f, size)
    res, z = PR.find_in_depth(img, cam, E.MAX_JUMP)
    lab = res["labels"]
    inn = (z > 0) & (lab < 0)
    P = PR.points(z, cam).astype(np.float64)
    Tcw = np.linalg.inv(E.trajectory(synth, 0)[f])
    masks = []
    for k in range(3):
        c = Tcw[:3, :3] @ E.object_pose(synth, 0, k)[:3, 3] + Tcw[:3, 3]
        masks.append(inn & (np.linalg.norm(P - c, axis=2) <= OBJECT_RADIUS))
    return z, cam, lab, masks


@functools.lru_cache(maxsize=None)
def run(f, size, max_step=0.0, rel_step=0.0):
    """-> (result, [per object None (out of view) or dict(pixels, segment, completeness, purity)])."""
    z, cam, lab, masks = frame(f, size)
    res = SR.segments(z, cam, E.MAX_JUMP, lab, max_step=max_step, rel_step=rel_step, max_segments=SR.SEGMENTS_MAX)
    objs = []
    for m in masks:
        n = int(m.sum())
        if n < MIN_OBJECT_PIXELS:
            objs.append(None)
            continue
        ls = res["labels"][m]
        ls = ls[ls >= 0]
        if not len(ls):
            objs.append(dict(pixels=n, segment=-1, completeness=0.0, purity=0.0))
            continue
        seg = int(np.bincount(ls).argmax())
        inside = int((res["labels"][m] == seg).sum())
        objs.append(dict(pixels=n, segment=seg, completeness=inside / n, purity=inside / int(res["records"]["pixels"][seg])))
    return res, objs


@functools.lru_cache(maxsize=None)
def table():
    """Rows of dict(max_step, rel_step, components and segments per frame, worst completeness / purity of objects 1 and 2
    and of object 0 over the frames that show it)."""
    rows = []
    for g in GATES:
        for rs in REL_STEPS:
            comps, segs, w12, w0 = [], [], [1.0, 1.0], [1.0, 1.0]
            for f, size in FRAMES:
                res, objs = run(f, size, g, rs)
                comps.append(res["n_components"])
                segs.append(res["n_candidates"])
                for k, o in enumerate(objs):
                    if o is None:
                        continue
                    w = w0 if k == 0 else w12
                    w[0], w[1] = min(w[0], o["completeness"]), min(w[1], o["purity"])
            rows.append(dict(max_step=g, rel_step=rs, components=tuple(comps), segments=tuple(segs), obj12=tuple(w12),
                             obj0=tuple(w0)))
    return rows


def fmt(rows):
    out = ["| max_step | rel_step | components (frames 0 3 5 9, 0 full) | components of min_pixels or more | objects 1, 2: "
           "completeness / purity (worst) | object 0: completeness / purity (worst) |", "|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %g | %g | %s | %s | %.3f / %.3f | %.3f / %.3f |" % (
            r["max_step"], r["rel_step"], " ".join(map(str, r["components"])), " ".join(map(str, r["segments"])),
            r["obj12"][0], r["obj12"][1], r["obj0"][0], r["obj0"][1]))
    return "\n".join(out)


if __name__ == "__main__":
    import time
    t0 = time.time()
    for f, size in FRAMES:
        res, objs = run(f, size)
        print("frame %d %s: %d in pixels, %d components, %d of min_pixels or more; objects %s" % (
            f, size, res["valid_in"], res["n_components"], res["n_candidates"],
            [None if o is None else (o["pixels"], o["segment"], round(o["completeness"], 3), round(o["purity"], 3)) for o in objs]))
    print(fmt(table()))
    print("%.1f s" % (time.time() - t0))
