"""The calibration of the planes stage, on the CPU with tests/planes_ref.py.

Frames 0, 3, 5 and 9 of camera_ref's room at 320 x 240 (volume_ref.SMALL).  Plane pixels are those where the frame equals
the planes_only render of the same pose, object pixels those that differ from it by more than 40 mm.  The table varies
dist_tol over {0.01, 0.02, 0.03} and min_normal_dot over {0.8, 0.9, 0.95} under Gaussian depth noise of 0, 3 and 6 mm
(bilateral_calib.add_noise) and gives, per cell, the planes found per frame and the worst frame's share of plane pixels
labelled and of object pixels kept.

`python tests/planes_calib.py` prints the table; tests/test_planes_host.py asserts on it.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bilateral_calib as BC  # noqa: E402
import camera_ref as E  # noqa: E402
import planes_inputs as PI  # noqa: E402
import planes_ref as PR  # noqa: E402
import track_ref as K  # noqa: E402

FRAMES = PI.ROOM_FRAMES
DIST_TOL = (0.01, 0.02, 0.03)
MIN_NORMAL_DOT = (0.8, 0.9, 0.95)
NOISE_MM = (0.0, 3.0, 6.0)
NOISE_SEED = 11
OBJECT_MM = 40


def _synth():
    import importlib
    return importlib.import_module("objective-slam_amd").synth


@functools.lru_cache(maxsize=None)
def frame(f):
    """-> (uint16 image, cam, plane pixel mask, object pixel mask) of frame f at 320 x 240."""
    synth = _synth()
    img, cam = PI.room_frame(synth, f)
    bare = PI.room_planes_only(synth, f)
    valid = img > 0
    return img, cam, valid & (img == bare), valid & (np.abs(img.astype(np.int64) - bare.astype(np.int64)) > OBJECT_MM)


@functools.lru_cache(maxsize=None)
def run(f, noise_mm=0.0, **kw):
    """The restatement on frame f with noise -> (result, z, shares dict)."""
    img, cam, plane_px, object_px = frame(f)
    noisy = BC.add_noise(img, np.random.default_rng(NOISE_SEED + f), noise_mm)
    res, z = PR.find_in_depth(noisy, cam, E.MAX_JUMP, **kw)
    lab = res["labels"]
    return res, z, dict(planes=res["n_planes"], plane_labelled=float((lab >= 0)[plane_px].mean()),
                        object_kept=float((lab < 0)[object_px].mean()))


@functools.lru_cache(maxsize=None)
def table():
    """Rows of dict(noise_mm, dist_tol, min_normal_dot, planes (per frame), plane_labelled, object_kept (worst frame))."""
    rows = []
    for noise in NOISE_MM:
        for tol in DIST_TOL:
            for dot in MIN_NORMAL_DOT:
                s = [run(f, noise, dist_tol=tol, min_normal_dot=dot)[2] for f in FRAMES]
                rows.append(dict(noise_mm=noise, dist_tol=tol, min_normal_dot=dot, planes=tuple(x["planes"] for x in s),
                                 plane_labelled=min(x["plane_labelled"] for x in s),
                                 object_kept=min(x["object_kept"] for x in s)))
    return rows


def fmt(rows):
    out = ["| noise mm | dist_tol | min_normal_dot | planes (frames 0 3 5 9) | plane pixels labelled (worst) | object pixels kept (worst) |",
           "|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %g | %g | %g | %s | %.4f | %.4f |" % (r["noise_mm"], r["dist_tol"], r["min_normal_dot"],
                                                          " ".join(str(k) for k in r["planes"]), r["plane_labelled"], r["object_kept"]))
    return "\n".join(out)


@functools.lru_cache(maxsize=None)
def lost_normals(f):
    """The known limit on frame f with the defaults: of the object pixels that have a normal in the frame and keep their
    depth, the share that has none in the reduced view."""
    img, cam, _, object_px = frame(f)
    res, z, _ = run(f)
    zr, _ = PR.remove(z, res["labels"])
    cam1 = dict(cam, depth_scale=1.0)
    has0 = K.view_maps(img, cam, E.MAX_JUMP)[2]
    has1 = K.view_maps(zr, cam1, E.MAX_JUMP)[2]
    sel = object_px & has0 & (zr > 0)
    return float((~has1)[sel].mean()), int(sel.sum())


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(fmt(table()))
    for f in FRAMES:
        print("frame %d: defaults %s; object pixels that lose their normal %.4f of %d" % ((f, run(f)[2]) + lost_normals(f)))
    print("%.1f s" % (time.time() - t0))
