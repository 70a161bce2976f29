"""Numpy restatement of the render stage (include/oslam.h at oslam_render_create and oslam_view_mask): the yardstick of
the device path.

Splat, resolve and mask follow the header's float32 sequences literally (the pose transform of tests/refine_ref.py, the
projection of tests/view_ref.py, the half-width, the keys as 64-bit integers, the window test of the mask), so both
images, every counter and the masked image equal the device's bit for bit.  numpy only: it runs wherever the tests do.
"""
import numpy as np

import refine_ref
import view_ref as V

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_SPLAT = 8
REMOVE, KEEP = 0, 1


def default_params():
    """oslam_render_params_default (footprint: the calibration of tests/test_render_host.py)."""
    return dict(footprint=0.75, max_splat=8, depth_tol=1.0, keep_back=0)


def default_mask_params():
    """oslam_mask_params_default."""
    return dict(mode=REMOVE, dilate=2, only=-1)


def project(q, cam, w, h):
    """view_ref.classify's projection: (inside bool [M], u, v int64 [M], 0 where not inside)."""
    pz = q[:, 2]
    zin = (pz >= F(cam["z_min"])) & (pz <= F(cam["z_max"]))
    with np.errstate(all="ignore"):
        fu = np.floor(((q[:, 0] * F(cam["fx"])) / pz + F(cam["cx"])) + F(0.5))
        fv = np.floor(((q[:, 1] * F(cam["fy"])) / pz + F(cam["cy"])) + F(0.5))
        inside = zin & (fu >= F(0)) & (fu < F(w)) & (fv >= F(0)) & (fv < F(h))
    return inside, np.where(inside, fu, 0).astype(np.int64), np.where(inside, fv, 0).astype(np.int64)


def half_width(pz, d_dist, fx, footprint, max_splat):
    """k of every point: rho = (float)((double)footprint * d_dist), kf = floorf((rho * fx) / p'z + 0.5f), capped."""
    rho = F(np.float64(F(footprint)) * np.float64(F(d_dist)))
    with np.errstate(all="ignore"):
        kf = np.floor((rho * F(fx)) / pz + F(0.5))
    return np.where(kf < F(max_splat), kf, F(max_splat)).astype(np.int64)


def points(mp, mn, T, cam, w, h, d_dist, footprint=0.75, max_splat=8, keep_back=0):
    """What every model point of one hypothesis does: (draw bool [M], u, v, k int64 [M], pz float32 [M], back bool [M])."""
    q, m = refine_ref.transform_f32(T, mp, mn)
    dot = (m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2]
    back = dot >= F(0)
    inside, u, v = project(q, cam, w, h)
    draw = inside & (~back | bool(keep_back))
    k = half_width(q[:, 2], d_dist, cam["fx"], footprint, max_splat)
    return draw, u, v, np.where(draw, k, 0), q[:, 2], back


def splat(clouds, T, cam, w, h, footprint=0.75, max_splat=8, keep_back=0):
    """k_render_splat: clouds [H] of (points, normals, d_dist), T [H,4,4] float32 (all zero = skipped) -> (keys uint64
    [h, w], drawn int64 [H])."""
    assert 0 <= max_splat <= MAX_SPLAT
    keys = np.full((h, w), EMPTY, np.uint64)
    H = len(clouds)
    drawn = np.zeros(H, np.int64)
    T = np.asarray(T, np.float32).reshape(H, 4, 4)
    for hyp, (mp, mn, d) in enumerate(clouds):
        if not (T[hyp] != 0).any():
            continue
        draw, u, v, k, pz, _ = points(mp, mn, T[hyp], cam, w, h, d, footprint, max_splat, keep_back)
        drawn[hyp] = int(draw.sum())
        if not draw.any():
            continue
        key = (pz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(hyp)
        kmax = int(k[draw].max())
        for dv in range(-kmax, kmax + 1):
            for du in range(-kmax, kmax + 1):
                uu, vv = u + du, v + dv
                sel = draw & (k >= max(abs(du), abs(dv))) & (uu >= 0) & (uu < w) & (vv >= 0) & (vv < h)
                if sel.any():
                    np.minimum.at(keys, (vv[sel], uu[sel]), key[sel])
    return keys, drawn


def resolve(keys, H):
    """k_render_resolve: -> (z float32 [h, w], labels int32 [h, w], pixels int64 [H])."""
    drawn = keys != EMPTY
    z = np.where(drawn, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), F(0)).astype(np.float32)
    labels = np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    pixels = np.bincount(labels[drawn].astype(np.int64), minlength=H)
    return z, labels, pixels


def tolerances(clouds, T, depth_tol=1.0):
    """tol[h] = (float)((double)depth_tol * d_dist), 0 for a skipped hypothesis."""
    T = np.asarray(T, np.float32).reshape(len(clouds), 4, 4)
    return np.array([V.tolerance(depth_tol, d) if (T[hyp] != 0).any() else F(0) for hyp, (_, _, d) in enumerate(clouds)],
                    np.float32)


def render(clouds, T, cam, w, h, footprint=0.75, max_splat=8, depth_tol=1.0, keep_back=0):
    """oslam_render_create: -> dict(z, labels, drawn, pixels, tol)."""
    keys, drawn = splat(clouds, T, cam, w, h, footprint, max_splat, keep_back)
    z, labels, pixels = resolve(keys, len(clouds))
    return dict(z=z, labels=labels, drawn=drawn, pixels=pixels, tol=tolerances(clouds, T, depth_tol))


def object_pixels(z_o, z_r, labels, tol, dilate=2, only=-1):
    """The object pixels of the observed z image under a render (bool [h, w])."""
    z_o = np.asarray(z_o, np.float32)
    h, w = z_o.shape
    obj = np.zeros((h, w), bool)
    lab_ok = (labels >= 0) if only < 0 else (labels == only)
    tol_px = np.where(labels >= 0, np.asarray(tol, np.float32)[np.clip(labels, 0, None)], F(0))
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in range(-dilate, dilate + 1):
        for dx in range(-dilate, dilate + 1):
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
            with np.errstate(all="ignore"):
                near = np.abs(z_o - z_r[yc, xc]) <= tol_px[yc, xc]
            obj |= ok & lab_ok[yc, xc] & near
    return obj & (z_o > F(0))


def mask(z_o, r, mode=REMOVE, dilate=2, only=-1):
    """oslam_view_mask on the observed z image (view_ref.view_z of the frame) under r = render(...): -> (z float32
    [h, w], dict valid_in object_pixels valid_out)."""
    z_o = np.asarray(z_o, np.float32)
    obj = object_pixels(z_o, r["z"], r["labels"], r["tol"], dilate, only)
    out = np.where(obj if mode == KEEP else ~obj, z_o, F(0)).astype(np.float32)
    return out, dict(valid_in=int((z_o > 0).sum()), object_pixels=int(obj.sum()), valid_out=int((out > 0).sum()))


def holes(labels):
    """(holes, labelled): a hole is an unlabelled pixel whose four axis neighbours are labelled."""
    lab = labels >= 0
    inner = ~lab[1:-1, 1:-1] & lab[:-2, 1:-1] & lab[2:, 1:-1] & lab[1:-1, :-2] & lab[1:-1, 2:]
    return int(inner.sum()), int(lab.sum())
