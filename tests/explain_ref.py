"""Numpy restatement of the explain stage (include/oslam.h at oslam_explain): the yardstick of the device path.

Every hypothesis is rendered alone by tests/render_ref.py into the full image (the device's rectangles are containers,
not part of the rule), compared with the observed z image of tests/view_ref.py in float32 with the header's operation
order, and the claims table goes through the elimination of tests/arbitrate_ref.py unchanged.  Integers are Python or
int64 integers, the scores float32 divisions, so every field equals the device's bit for bit.  numpy only.
"""
import numpy as np

import arbitrate_ref
import render_ref
import view_ref

F = np.float32
AGREE, OCCLUDED, THROUGH, UNKNOWN = range(4)
NAMES = ("agree", "occluded", "through", "unknown")
MAX_HYPOTHESES = arbitrate_ref.MAX_HYPOTHESES


def default_params():
    """oslam_explain_params_default: the render's footprint, max_splat and keep_back, the arbitration's tile,
    tile_spacing and min_tiles; min_owned_share from the calibration table of tests/test_explain_host.py."""
    r, a = render_ref.default_params(), arbitrate_ref.default_params()
    return dict(footprint=r["footprint"], max_splat=r["max_splat"], keep_back=r["keep_back"], depth_tol=1.0, tile=a["tile"],
                tile_spacing=a["tile_spacing"], min_tiles=a["min_tiles"], min_owned_share=0.52)


def solo_z(cloud, T, cam, w, h, footprint=0.75, max_splat=8, keep_back=0):
    """Z_h: the z image of the render of the one-element list -> (z float32 [h, w], drawn)."""
    r = render_ref.render([cloud], np.asarray(T, np.float32).reshape(1, 4, 4), cam, w, h, footprint, max_splat, 1.0, keep_back)
    return r["z"], int(r["drawn"][0])


def classify(z_h, z_o, tol):
    """-> (class int8 [h, w], -1 where Z_h == 0; r int64 [h, w], the quantised residual of the AGREE pixels, 0 elsewhere)."""
    tol = F(tol)
    cls = np.full(z_h.shape, -1, np.int8)
    on = z_h > F(0)
    with np.errstate(all="ignore"):
        dz = np.abs(z_o - z_h)
        x = dz * (F(65535.0) / tol)
    unknown = on & (z_o == F(0))
    agree = on & ~unknown & (dz <= tol)
    occluded = on & ~unknown & ~agree & (z_o < z_h)
    through = on & ~unknown & ~agree & ~occluded
    cls[unknown], cls[agree], cls[occluded], cls[through] = UNKNOWN, AGREE, OCCLUDED, THROUGH
    xq = np.where(agree, x, F(0)).astype(np.float32)
    r = np.where(xq < F(65535.0), xq, F(65535.0)).astype(np.uint32).astype(np.int64)
    return cls, np.where(agree, r, 0)


def scores(cls, r, tol):
    """The counters and scores of one hypothesis from its classes."""
    c = {n: int((cls == k).sum()) for k, n in enumerate(NAMES)}
    a, o, t = c["agree"], c["occluded"], c["through"]
    c["pixels"] = a + o + t + c["unknown"]
    c["resid_sum"] = int(r.sum())
    c["explained"] = F(a) / F(a + t) if a + t else F(0)
    c["visible"] = F(a) / F(a + o + t) if a + o + t else F(0)
    c["mean_residual"] = F(((np.float64(c["resid_sum"]) / np.float64(a)) / 65535.0) * np.float64(F(tol))) if a else F(0)
    c["conflict_q"] = (65535 * t) // (a + t) if a else 0
    return c


def zero_result():
    r = dict(drawn=0, pixels=0, agree=0, occluded=0, through=0, unknown=0, resid_sum=0, explained=F(0), visible=F(0),
             mean_residual=F(0), conflict_q=0)
    r.update(claimed=0, owned=0, share=F(0), kept=False, suppressed_by=-1)
    return r


def explain(models, T, depth, cam, footprint=0.75, max_splat=8, keep_back=0, depth_tol=1.0, tile=0, tile_spacing=2.0,
            min_tiles=4, min_owned_share=0.52, z=None, taps=None):
    """models = [(points, normals, d_dist)] [H], T [H,4,4] (all zeros: skipped), cam as in view_ref.verify; z: the
    observed z image instead of view_z(depth).  -> list of result dicts (the fields of oslam_explain_result but launches
    and ms_total).  taps: a dict that receives z [H] (the solo z images), cnt and sum [H, n_tiles]."""
    T = [np.asarray(A, np.float32).reshape(4, 4) for A in T]
    H = len(models)
    assert 1 <= H <= MAX_HYPOTHESES and len(T) == H
    z_o = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"]) if z is None else np.asarray(z, np.float32)
    h, w = z_o.shape
    skipped = [arbitrate_ref.is_skipped(A) for A in T]
    tile = arbitrate_ref.choose_tile(models, T, cam["fx"], tile, tile_spacing)
    tiles_x = -(-w // tile)
    n_tiles = tiles_x * -(-h // tile)
    cnt = np.zeros((H, n_tiles), np.int64)
    sm = np.zeros((H, n_tiles), np.int64)
    tols = np.zeros(H, np.float32)
    res = [zero_result() for _ in range(H)]
    zs = []
    ys, xs = np.mgrid[0:h, 0:w]
    tile_of = (ys // tile) * tiles_x + xs // tile
    for k, (cloud, A) in enumerate(zip(models, T)):
        if skipped[k]:
            zs.append(np.zeros((h, w), np.float32))
            continue
        tols[k] = view_ref.tolerance(depth_tol, cloud[2])
        z_h, drawn = solo_z(cloud, A, cam, w, h, footprint, max_splat, keep_back)
        zs.append(z_h)
        cls, r = classify(z_h, z_o, tols[k])
        res[k].update(scores(cls, r, tols[k]), drawn=drawn)
        np.add.at(cnt[k], tile_of[cls == AGREE], 1)
        sm[k] = cnt[k] * res[k]["conflict_q"]
    if taps is not None:
        taps.update(z=zs, cnt=cnt, sum=sm)
    rounds = 0
    if not all(skipped):
        arb, rounds = arbitrate_ref.eliminate(cnt, sm, skipped, tols, min_tiles, min_owned_share)
        for k in range(H):
            if not skipped[k]:
                res[k].update({f: arb[k][f] for f in ("claimed", "owned", "share", "kept", "suppressed_by")})
    for r in res:
        r["tile"], r["rounds"] = tile, rounds
    return res


def kept(res):
    return [k for k, r in enumerate(res) if r["kept"]]
