"""Numpy restatement of the depth image pyramid (include/oslam.h at oslam_pyramid_create) and of coarse-to-fine camera
motion over two pyramids (oslam_pyramid_egomotion): the yardstick of the device path.

float32 throughout; the 25 taps of the window are added in a loop in the header's order (dy outer, dx inner), so the
device can be asked for the same bits.  The maps of a level are track_ref.view_maps of its z image with its camera and
max_jump; a schedule level is camera_ref.egomotion on the level's maps.  numpy only.
"""
import numpy as np

import camera_ref as E
import track_ref as K
import view_ref

F = np.float32
DEPTH_BAND = 0.09               # oslam_pyramid_params_default
MAX_LEVELS = 3


def pyr_down(z, cam, max_jump, depth_band=DEPTH_BAND):
    """z float32 [h, w] in metres (0 = invalid) with camera cam and max_jump -> (z', cam', max_jump') of the next level."""
    z = np.ascontiguousarray(z, np.float32)
    h, w = z.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    band = F(depth_band)
    c = z[::2, ::2]
    assert c.shape == (ho, wo)
    pad = np.zeros((h + 4, w + 4), np.float32)          # outside the image: z = 0 never takes part, which is the clipping
    pad[2:h + 2, 2:w + 2] = z
    s = np.zeros((ho, wo), np.float32)
    cnt = np.zeros((ho, wo), np.int32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            t = pad[2 + dy:2 + dy + 2 * ho - 1:2, 2 + dx:2 + dx + 2 * wo - 1:2]
            m = (t > 0) & (np.abs(t - c) <= band)
            s = np.where(m, s + t, s).astype(np.float32)
            cnt += m
    with np.errstate(all="ignore"):
        mean = (s / cnt.astype(np.float32)).astype(np.float32)
    out = np.minimum(np.maximum(mean, F(cam["z_min"])), F(cam["z_max"])).astype(np.float32)
    out = np.where(c != 0, out, F(0)).astype(np.float32)
    half = F(0.5)
    cam2 = dict(cam, fx=float(F(cam["fx"]) * half), fy=float(F(cam["fy"]) * half), cx=float(F(cam["cx"]) * half),
                cy=float(F(cam["cy"]) * half))
    return out, cam2, float(F(max_jump) * F(2.0))


def pyramid(depth, cam, max_jump, levels=MAX_LEVELS, depth_band=DEPTH_BAND):
    """A depth image (uint16 or float32 raw, as oslam_view_create takes it) -> [dict(z, cam, max_jump)] per level, level
    0 first.  Every level's z is in metres, so its cam carries depth_scale 1."""
    assert 1 <= levels <= MAX_LEVELS
    z = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    out = [dict(z=z, cam=dict(cam, depth_scale=1.0), max_jump=float(F(max_jump)))]
    for _ in range(levels - 1):
        a = out[-1]
        z, c, mj = pyr_down(a["z"], a["cam"], a["max_jump"], depth_band)
        out.append(dict(z=z, cam=c, max_jump=mj))
    return out


def level_maps(level):
    """track_ref.view_maps of one level of pyramid()."""
    return K.view_maps(level["z"], level["cam"], level["max_jump"])


def with_maps(pyr):
    for lv in pyr:
        if "maps" not in lv:
            lv["maps"] = level_maps(lv)
    return pyr


def egomotion_pyramid(src_pyr, dst_pyr, T_init=None, sums="f64", **kw):
    """oslam_pyramid_egomotion over two pyramid() lists: every schedule level {stride, n} is camera_ref.egomotion with
    the single level {1, n} on level log2(stride) of both, from the float32 pose the last one left.  -> (T, result dict)
    with the fields of camera_ref.egomotion (cond: of the first level that ran)."""
    p = E.default_params()
    p.update(kw)
    levels = list(p.pop("levels"))
    Tf = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32).reshape(4, 4).copy()
    iterations = [0] * len(levels)
    last, overlap, finest, cond = None, 0.0, None, 0.0
    for L, (stride, max_it) in enumerate(levels):
        k = {1: 0, 2: 1, 4: 2}[stride]
        if k >= len(src_pyr) or k >= len(dst_pyr):
            raise ValueError("a stride names a level the pyramid does not have")
        if max_it == 0:
            continue
        with_maps(src_pyr[k:k + 1])
        with_maps(dst_pyr[k:k + 1])
        Tf, r = E.egomotion(src_pyr[k]["maps"], dst_pyr[k]["maps"], dst_pyr[k]["cam"], Tf, sums=sums, levels=[(1, max_it)], **p)
        iterations[L] = r["iterations"][0]
        last = r
        cond = cond or r["cond"]
        if finest is None or stride <= finest:
            finest, overlap = stride, r["overlap"]
        if not r["converged"] and r["iterations"][0] < max_it:         # fewer than 6 correspondences or a failed solve
            break
    if last is None:
        return Tf, dict(iterations=iterations, correspondences=0, rmse=0.0, overlap=0.0, converged=0,
                        ok=int(0.0 >= F(p["min_overlap"])), cond=0.0)
    return Tf, dict(iterations=iterations, correspondences=last["correspondences"], rmse=last["rmse"], overlap=overlap,
                    converged=last["converged"], ok=int(overlap >= F(p["min_overlap"])), cond=cond)
