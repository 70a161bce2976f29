"""A registered depth and colour pair of the room of tests/camera_ref.py: the depth frame camera_ref.render gives, and
for every pixel the colour of the world point that won its z-buffer.  The colour of a world point is a fixed function of
the thing it belongs to (back wall, floor, side wall, an object) and of its position, smooth on the scale of a voxel of
the calibration (5 cm), so that a fused colour can be compared with the function at the point.  numpy only; seeded."""
import numpy as np

import camera_ref as E

BACK, FLOOR, SIDE, OBJECT = 0, 1, 2, 3
# a base colour per thing and a slow wave over the position: periods of 2 to 3 metres, 40 to 60 voxels of the calibration
BASE = np.array([[150.0, 140.0, 120.0], [90.0, 120.0, 100.0], [110.0, 110.0, 160.0], [190.0, 90.0, 70.0]])
AMPLITUDE = 50.0
WAVES = np.array([[2.1, 0.7, 1.3], [0.9, 2.4, 1.7], [1.5, 1.1, 2.6]])          # radians per metre: row = channel
PLANE_TOL = 0.08                # metres: a point this near a plane belongs to it


def labels(points, seed=0):
    """The thing each world point [n, 3] belongs to: the planes of camera_ref.make_world(seed) by distance (the nearest
    wins within PLANE_TOL), an object otherwise.  Exact for make_world's own points, whose planes are exact."""
    p = np.asarray(points, np.float64)
    zw = E.WORLD_DEPTH + 0.4 * seed
    d = np.stack([np.abs(p[:, 2] - zw), np.abs(p[:, 1] - 1.5), np.abs(p[:, 0] + 2.5)], axis=1)
    near = d.argmin(axis=1)
    return np.where(d.min(axis=1) <= PLANE_TOL, near, OBJECT)


def colour(points, seed=0, label=None):
    """The colour function: float64 [n, 3] in 0..255 (never clipped: 20 <= value <= 240)."""
    p = np.asarray(points, np.float64)
    lab = labels(p, seed) if label is None else label
    return BASE[lab] + AMPLITUDE * np.sin(p @ WAVES.T + lab[:, None])


def world_colours(world, seed=0):
    """uint8 [n, 3]: the colour of every point of camera_ref.make_world(seed), rounded"""
    return np.rint(colour(world, seed)).astype(np.uint8)


def render(synth, world, rgb, T_world_cam, width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001):
    """-> (depth uint16 [h, w]: camera_ref.render's frame bit for bit; rgb uint8 [h, w, 3]; valid bool [h, w]).
    synth.render_depth's z-buffer (splat 1), kept as a minimum over raw << 32 | index so that the winning point is known:
    among points of one raw depth the lowest index wins."""
    Tc = np.linalg.inv(np.asarray(T_world_cam, np.float64))
    p = world @ Tc[:3, :3].T + Tc[:3, 3]
    z = p[:, 2]
    idx = np.flatnonzero(z > 1e-6)
    p, z = p[idx], z[idx]
    u = np.rint(p[:, 0] * fx / z + cx).astype(np.int64)
    v = np.rint(p[:, 1] * fy / z + cy).astype(np.int64)
    raw = np.clip(np.rint(z / depth_scale), 1, 65535).astype(np.int64)
    key = raw << 32 | idx
    none = np.int64(65536) << 32
    img = np.full(width * height, none, np.int64)
    for dv in (-1, 0, 1):
        for du in (-1, 0, 1):
            uu, vv = u + du, v + dv
            m = (uu >= 0) & (uu < width) & (vv >= 0) & (vv < height)
            np.minimum.at(img, vv[m] * width + uu[m], key[m])
    valid = img != none
    depth = np.where(valid, img >> 32, 0).astype(np.uint16).reshape(height, width)
    out = np.where(valid[:, None], rgb[np.where(valid, img & 0xffffffff, 0)], 0).astype(np.uint8).reshape(height, width, 3)
    return depth, out, valid.reshape(height, width)
