"""Numpy restatement of the arbitration stage (include/oslam.h at oslam_arbitrate): the yardstick of the device path.

Claims come from the classes of tests/view_ref.py (float32, the header's operation order), the table is integers, the
ownership comparison is done in Python integers and the shares are float32 divisions, so every field equals the
device's bit for bit.  numpy only.
"""
import math

import numpy as np

import instances_ref
import refine_ref
import view_ref

F = np.float32
MAX_HYPOTHESES = 1024


def default_params():
    """oslam_arbitrate_params_default (min_owned_share from the calibration table of tests/test_arbitrate_host.py)."""
    return dict(depth_tol=1.0, window=1, tile=0, tile_spacing=2.0, min_tiles=4, min_owned_share=0.52)


def is_skipped(T):
    return not np.asarray(T).any()


def residuals(mp, mn, T, z, cam, tol, window=1):
    """(class, fu, fv, r) of every model point: r = the smallest |z_o - p'z| (float32) over the valid pixels of the
    window, inf without one; fu, fv its pixel (0 where the point is BACK or OUT)."""
    cls = view_ref.classify(mp, mn, T, z, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["z_min"], cam["z_max"], tol, window)
    q, _ = refine_ref.transform_f32(T, mp, mn)
    h, w = z.shape
    pz = q[:, 2]
    inside = cls >= view_ref.SUPPORTED
    with np.errstate(all="ignore"):
        fu = np.floor(((q[:, 0] * F(cam["fx"])) / pz + F(cam["cx"])) + F(0.5))
        fv = np.floor(((q[:, 1] * F(cam["fy"])) / pz + F(cam["cy"])) + F(0.5))
    u = np.where(inside, fu, 0).astype(np.int64)
    v = np.where(inside, fv, 0).astype(np.int64)
    r = np.full(len(q), np.inf, np.float32)
    for dv in range(-window, window + 1):
        for du in range(-window, window + 1):
            uu, vv = u + du, v + dv
            ok = inside & (uu >= 0) & (uu < w) & (vv >= 0) & (vv < h)
            zo = np.where(ok, z[np.clip(vv, 0, h - 1), np.clip(uu, 0, w - 1)], F(0))
            valid = ok & (zo > F(0))
            r = np.where(valid, np.minimum(r, np.abs(zo - pz)), r).astype(np.float32)
    return cls, u, v, r


def choose_tile(models, T, fx, tile=0, tile_spacing=2.0):
    """The tile of a call: models = [(points, normals, d_dist)], T [H,4,4]."""
    if tile:
        return int(tile)
    d_max, z_near = F(0), F(0)
    for (mp, _, d), A in zip(models, T):
        if is_skipped(A):
            continue
        d_max = max(d_max, F(d))
        zc = instances_ref.transformed_centroid(A, instances_ref.centroid(mp))[2]
        if zc > 0 and (z_near == 0 or zc < z_near):
            z_near = zc
    if not z_near > 0:
        return 128
    t = math.ceil(((float(F(tile_spacing)) * float(d_max)) * float(F(fx))) / float(z_near))
    return 4 if not t >= 4 else 128 if t > 128 else int(t)


def claims(models, T, depth, cam, depth_tol=1.0, window=1, tile=0, tile_spacing=2.0):
    """-> (cnt int64 [H, n_tiles], sum int64 [H, n_tiles], tile, tol [H])."""
    z = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    h, w = z.shape
    tile = choose_tile(models, T, cam["fx"], tile, tile_spacing)
    tiles_x = -(-w // tile)
    n_tiles = tiles_x * -(-h // tile)
    H = len(models)
    cnt = np.zeros((H, n_tiles), np.int64)
    sm = np.zeros((H, n_tiles), np.int64)
    tols = np.zeros(H, np.float32)
    for k, ((mp, mn, d), A) in enumerate(zip(models, T)):
        if is_skipped(A):
            continue
        tol = view_ref.tolerance(depth_tol, d)
        tols[k] = tol
        cls, u, v, r = residuals(mp, mn, np.asarray(A, np.float32), z, cam, tol, window)
        s = cls == view_ref.SUPPORTED
        with np.errstate(all="ignore"):
            x = r[s] * (F(65535.0) / tol)
        q = np.where(x < F(65535.0), x, F(65535.0)).astype(np.uint32).astype(np.int64)
        t = (v[s] // tile) * tiles_x + u[s] // tile
        np.add.at(cnt[k], t, 1)
        np.add.at(sm[k], t, q)
    return cnt, sm, tile, tols


def owners(cnt, sm, live):
    """Owner of every tile among the live claimants (-1: none): the smallest mean residual, compared exactly as
    sum_a * cnt_b < sum_b * cnt_a; ties to the lower index."""
    H, n = cnt.shape
    own = np.full(n, -1, np.int64)
    for t in np.flatnonzero((cnt[np.asarray(live, bool)] > 0).any(axis=0)) if any(live) else []:
        best, bs, bc = -1, 0, 0
        for h in range(H):
            c = int(cnt[h, t])
            if not live[h] or c == 0:
                continue
            s = int(sm[h, t])
            if best < 0 or s * bc < bs * c:
                best, bs, bc = h, s, c
        own[t] = best
    return own


def eliminate(cnt, sm, skipped, tols, min_tiles=4, min_owned_share=0.52, order=None):
    """The elimination over a claims table -> (list of result dicts, rounds).  order: a list that receives the
    suppressed hypotheses in the order they leave."""
    H = cnt.shape[0]
    claimed = (cnt > 0).sum(axis=1)
    live = [bool(not skipped[h] and claimed[h] >= 1 and claimed[h] >= min_tiles) for h in range(H)]
    res = []
    for h in range(H):
        n, s = int(cnt[h].sum()), int(sm[h].sum())
        mr = F(((np.float64(s) / np.float64(n)) / 65535.0) * np.float64(tols[h])) if n else F(0)
        res.append(dict(claimed=0 if skipped[h] else int(claimed[h]), owned=0, share=F(0), mean_residual=F(0) if skipped[h] else mr,
                        kept=False, suppressed_by=-1))
    rounds = 0
    for _ in range(H):
        if not any(live):
            break
        own = owners(cnt, sm, live)
        rounds += 1
        loser, ls = -1, None
        for h in range(H):
            if not live[h]:
                continue
            o = int((own == h).sum())
            sh = F(o) / F(claimed[h])
            res[h]["owned"], res[h]["share"] = o, sh
            if loser < 0 or sh <= ls:
                loser, ls = h, sh
        if not ls < F(min_owned_share):
            break
        mine = cnt[loser] > 0
        by, bb = -1, 0
        for h in range(H):
            b = int(((own == h) & mine).sum()) if live[h] and h != loser else 0
            if b > bb:
                by, bb = h, b
        res[loser]["suppressed_by"] = by
        live[loser] = False
        if order is not None:
            order.append(loser)
    for h in range(H):
        res[h]["kept"] = live[h]
    return res, rounds


def arbitrate(models, T, depth, cam, depth_tol=1.0, window=1, tile=0, tile_spacing=2.0, min_tiles=4, min_owned_share=0.52):
    """models = [(points, normals, d_dist)] [H], T [H,4,4] (all zeros: skipped), cam as in view_ref.verify.
    -> (list of result dicts with claimed, owned, share, mean_residual, kept, suppressed_by, tile, rounds; kept bool [H])."""
    T = [np.asarray(A, np.float32).reshape(4, 4) for A in T]
    skipped = [is_skipped(A) for A in T]
    cnt, sm, tile, tols = claims(models, T, depth, cam, depth_tol, window, tile, tile_spacing)
    if all(skipped):
        res, rounds = [dict(claimed=0, owned=0, share=F(0), mean_residual=F(0), kept=False, suppressed_by=-1) for _ in T], 0
    else:
        res, rounds = eliminate(cnt, sm, skipped, tols, min_tiles, min_owned_share)
    for r in res:
        r["tile"], r["rounds"] = tile, rounds
    return res, np.array([r["kept"] for r in res], dtype=bool)
