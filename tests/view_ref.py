"""Numpy restatement of the verification stage (include/oslam.h at oslam_verify): the yardstick of the device path.

Every class is computed in float32 with the header's operation order (the pose transform of tests/refine_ref.py, the
projection, the window tests), so the classes equal the device's bit for bit.  numpy only: it runs wherever the tests
do.
"""
import numpy as np

import refine_ref

BACK, OUT, SUPPORTED, OCCLUDED, CONFLICT, UNKNOWN = range(6)
NAMES = ("back", "out", "supported", "occluded", "conflict", "unknown")
F = np.float32


def default_params():
    """oslam_verify_params_default (the thresholds come from the calibration table of tests/test_verify_host.py)."""
    return dict(depth_tol=1.0, window=1, min_view_fitness=0.92, min_coverage=0.5, min_supported=50)


def view_z(depth, depth_scale=0.001, z_min=0.1, z_max=10.0):
    """The view's z image (k_view_z): z = raw * depth_scale in float32, 0 where z is outside [z_min, z_max]."""
    d = np.asarray(depth)
    assert d.dtype in (np.uint16, np.float32) and d.ndim == 2
    with np.errstate(invalid="ignore", over="ignore"):
        z = d.astype(np.float32) * F(depth_scale)
        ok = (z >= F(z_min)) & (z <= F(z_max))
    return np.where(ok, z, F(0)).astype(np.float32)


def tolerance(depth_tol, d_dist):
    """tol = (float)((double)depth_tol * d_dist)."""
    return F(np.float64(F(depth_tol)) * np.float64(F(d_dist)))


def classify(mp, mn, T, z, fx, fy, cx, cy, z_min, z_max, tol, window=1):
    """Class of every model point (uint8 [M], BACK .. UNKNOWN) under the float32 pose T against the z image."""
    q, m = refine_ref.transform_f32(T, mp, mn)
    h, w = z.shape
    M = len(q)
    cls = np.full(M, UNKNOWN, np.uint8)
    dot = (m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2]
    back = dot >= F(0)
    pz = q[:, 2]
    zin = (pz >= F(z_min)) & (pz <= F(z_max))
    with np.errstate(all="ignore"):
        fu = np.floor(((q[:, 0] * F(fx)) / pz + F(cx)) + F(0.5))
        fv = np.floor(((q[:, 1] * F(fy)) / pz + F(cy)) + F(0.5))
        inside = zin & (fu >= F(0)) & (fu < F(w)) & (fv >= F(0)) & (fv < F(h))
    u = np.where(inside, fu, 0).astype(np.int64)
    v = np.where(inside, fv, 0).astype(np.int64)
    tol = F(tol)
    lim = pz - tol
    sup = np.zeros(M, bool)
    near = np.zeros(M, bool)
    anyv = np.zeros(M, bool)
    for dv in range(-window, window + 1):
        for du in range(-window, window + 1):
            uu, vv = u + du, v + dv
            ok = inside & (uu >= 0) & (uu < w) & (vv >= 0) & (vv < h)
            zo = np.where(ok, z[np.clip(vv, 0, h - 1), np.clip(uu, 0, w - 1)], F(0))
            valid = ok & (zo > F(0))
            sup |= valid & (np.abs(zo - pz) <= tol)
            near |= valid & (zo < lim)
            anyv |= valid
    cls[anyv] = CONFLICT
    cls[near] = OCCLUDED
    cls[sup] = SUPPORTED
    cls[~inside] = OUT
    cls[back] = BACK
    return cls


def scores(cls, min_view_fitness=None, min_coverage=None, min_supported=None):
    """Counts, view_fitness, coverage and found of a class array (float32 divisions of the counts as floats)."""
    p = default_params()
    mvf = F(p["min_view_fitness"] if min_view_fitness is None else min_view_fitness)
    mcv = F(p["min_coverage"] if min_coverage is None else min_coverage)
    msu = p["min_supported"] if min_supported is None else min_supported
    c = np.bincount(np.asarray(cls, np.int64), minlength=6)
    r = {NAMES[k]: int(c[k]) for k in range(6)}
    s, o, x = r["supported"], r["occluded"], r["conflict"]
    r["view_fitness"] = float(F(s) / F(s + x)) if s + x else 0.0
    r["coverage"] = float(F(s) / F(s + o + x)) if s + o + x else 0.0
    r["found"] = bool(s >= msu and F(r["view_fitness"]) >= mvf and F(r["coverage"]) >= mcv)
    return r


def verify(mp, mn, T, depth, cam, d_dist, depth_tol=1.0, window=1, **kw):
    """classify + scores for one model; cam = dict(fx, fy, cx, cy, depth_scale, z_min, z_max)."""
    z = view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    cls = classify(mp, mn, T, z, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["z_min"], cam["z_max"],
                   tolerance(depth_tol, d_dist), window)
    return scores(cls, **kw), cls
