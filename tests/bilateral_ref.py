"""Numpy restatement of the bilateral depth filter (include/oslam.h at oslam_view_bilateral): the yardstick of the device
path.

float32 throughout.  The (2R + 1)^2 offsets of the window are walked in a loop in the header's order (dy outer, dx inner)
over shifted copies of the image, every operation is one numpy float32 operation (no fused multiply-add), and the weights
come from the generator's table (tools/gen_gauss_table.py), not from the compiled header, so the device can be asked for
the same bits.  numpy only.
"""
import os
import sys

import numpy as np

import view_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_gauss_table as GT  # noqa: E402

F = np.float32
G = np.array(GT.table(), np.float32)
MAX_RADIUS = 8


def default_params():
    """oslam_bilateral_params_default: KinFu's."""
    return dict(radius=6, sigma_space=4.5, sigma_depth=0.03)


def constants(sigma_space, sigma_depth):
    """-> (inv_s, inv_r) float32, from the float32 sigmas in double"""
    s, r = np.float64(F(sigma_space)), np.float64(F(sigma_depth))
    return F(1.0 / (s * s)), F(1.0 / (r * r))


def bilateral(z, z_min, z_max, radius=6, sigma_space=4.5, sigma_depth=0.03):
    """z float32 [h, w] in metres (0 = invalid) -> (z' float32 [h, w], valid, taps)."""
    z = np.ascontiguousarray(z, np.float32)
    assert z.ndim == 2 and 1 <= radius <= MAX_RADIUS
    h, w = z.shape
    R = int(radius)
    inv_s, inv_r = constants(sigma_space, sigma_depth)
    pad = np.zeros((h + 2 * R, w + 2 * R), np.float32)      # outside the image: z = 0 never takes part, which is the clipping
    pad[R:h + R, R:w + R] = z
    c = z
    live = c != 0
    sd = np.zeros((h, w), np.float32)
    sw = np.zeros((h, w), np.float32)
    taps = np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                zt = pad[R + dy:R + dy + h, R + dx:R + dx + w]
                d = zt - c
                t = F(dx * dx + dy * dy) * inv_s + (d * d) * inv_r
                m = live & (zt > 0) & (t < F(9.0))
                wgt = G[np.where(m, t * F(32.0), F(0)).astype(np.int32)]
                sd = np.where(m, sd + wgt * d, sd)
                sw = np.where(m, sw + wgt, sw)
                taps += m
        out = np.minimum(np.maximum(c + sd / sw, F(z_min)), F(z_max)).astype(np.float32)
    out = np.where(live, out, F(0)).astype(np.float32)
    assert sd.dtype == sw.dtype == np.float32
    return out, int((out > 0).sum()), int(taps.sum())


def bilateral_depth(depth, cam, **kw):
    """A depth image as oslam_view_create takes it (uint16 or float32 raw) with camera cam (depth_scale, z_min, z_max) ->
    what bilateral returns for its z image."""
    z = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    return bilateral(z, cam["z_min"], cam["z_max"], **kw)
