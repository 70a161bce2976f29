"""CPU calibration of the shifting window: the loop of ppf.Volume.step(view, follow=...) restated over
tests/volume_ref.py and tests/shift_ref.py, on the small stream of the calibration room with a volume narrower than the
camera's path, next to the same stream and volume without shifting.  Prints where the window moves, whether the
frame-to-model steps stay ok across the moves, and the pose error against the truth.  Findings, not thresholds.

    python tests/shift_calib.py [seed]
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_ref as R  # noqa: E402
import shift_ref as H  # noqa: E402
import volume_ref as V  # noqa: E402

# 6.4 x 4.8 x 6.4 m around the first camera's view; the room is 9.2 m wide and the camera turns 27 degrees over the stream
VOLUME = dict(nx=128, ny=96, nz=128, voxel=0.05, origin=[-3.2, -2.4, 0.3], mu=0.4, max_weight=128)
FOLLOW = dict(lookahead=3.5, threshold=4.0, granule=4)             # d = 0 at the identity; 3 degrees are 3.7 voxels there
# the window is narrower than the view as well: the ray cast covers less of a frame than oslam_view_egomotion's default
# min_overlap of 0.75 asks for (0.66 at frame 1), so the steps run with a lower one
MIN_OVERLAP = 0.4


def run(s, follow, frames, min_overlap):
    """-> [(frame, T, result or None, shift, offset, points that left)]"""
    vol = V.Volume(**VOLUME)
    T = np.eye(4, dtype=np.float32)
    vol.integrate(s["z"][0], V.SMALL_CAM, T)
    out = [(0, T, None, (0, 0, 0), (0, 0, 0), 0)]
    for f in frames[1:]:
        Tn, r = vol.track(s["maps"][f], V.SMALL_CAM, T, min_overlap=min_overlap)
        shift, left = (0, 0, 0), 0
        if r["ok"]:
            T = Tn
            vol.integrate(s["z"][f], V.SMALL_CAM, T)
            if follow is not None:
                shift = H.follow(vol, T, **follow)
                if any(shift):
                    left = len(H.leaving(vol, shift)[0])
                    vol = H.shifted(vol, shift)
        out.append((f, T, r, shift, H.state(vol)[1], left))
    return out


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    synth = importlib.import_module("objective-slam_amd").synth
    s = V.small_stream(synth, seed)
    frames = list(range(10))
    for name, follow, mo in (("fixed window", None, 0.75), ("fixed window", None, MIN_OVERLAP), ("following window", FOLLOW, MIN_OVERLAP)):
        print("%s, min_overlap %.2f, volume %s, follow %s" % (name, mo, VOLUME, follow))
        for f, T, r, shift, off, left in run(s, follow, frames, mo):
            rot, tr = R.pose_error(T, s["traj"][f])
            print("  frame %d: %s, %.4f deg %.4f m from the truth, shift %s -> offset %s, %d points left" % (
                f, "first" if r is None else "ok %d overlap %.3f" % (r["ok"], r["overlap"]), rot, tr, shift, off, left))


if __name__ == "__main__":
    main()
