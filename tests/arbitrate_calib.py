"""The calibration of the arbitration defaults on the CPU (tests/test_arbitrate_host.py): the seeded depth frames of
tests/verify_calib.py, an 11-member database (synthetic models 0..9 and 36, the near twin of model 0), every member's
voting pose from the oracle (df 4), refined by tests/refine_ref.py, verified by tests/view_ref.py, then arbitrated by
tests/arbitrate_ref.py over the members verification found."""
import numpy as np

import arbitrate_ref
import refine_ref
import verify_calib
import view_ref

MEMBERS = list(range(10)) + [36]
TWIN = len(MEMBERS) - 1            # index of model 36 in the database
SPACINGS = (1.0, 2.0, 3.0)
CAM = verify_calib.CAM


def models(synth, oracle):
    raw = [synth.make_model(k, 1500) for k in MEMBERS]
    d = synth.d_dist_for(raw[0][0], 0.05)
    return [oracle.voxel_grid(p, n, d) for p, n in raw], d


def table(synth, oracle, n_frames=6, seed=211, min_owned_share=0.0):
    """One row per frame: found = the members verification found; per tile_spacing the arbitration results of model 0
    (`present`), of 36 (`twin`) and the largest share of the rest, first with min_owned_share 0 (nothing is
    suppressed: the raw shares of one round) and the kept set under `min_owned_share`."""
    grids, d = models(synth, oracle)
    rows = []
    for img, truth, occluded in verify_calib.frames(synth, n_frames, seed):
        sp, sn = oracle.depth_to_cloud(img, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["depth_scale"], CAM["z_min"],
                                       CAM["z_max"], verify_calib.MAX_JUMP)
        sp, sn = oracle.voxel_grid(sp, sn, d)
        T = np.zeros((len(grids), 4, 4), np.float32)
        found = []
        for j, (gp, gn) in enumerate(grids):
            cells, _ = oracle.votes_fused(gp, gn, sp, sn, 4, d, 0.4)
            _, T0 = oracle.pose_from_cells(cells, gp, gn, sp, sn, d)
            if not T0.any():
                continue
            T1, _ = refine_ref.refine(gp, gn, sp, sn, T0, d)
            r, _ = view_ref.verify(gp, gn, T1, img, CAM, d)
            if r["found"]:
                T[j] = T1
                found.append(j)
        row = dict(occluded=occluded, found=found, spacing={})
        hyp = [(gp, gn, d) for gp, gn in grids]
        for ts in SPACINGS:
            raw, _ = arbitrate_ref.arbitrate(hyp, T, img, CAM, tile_spacing=ts, min_owned_share=0.0)
            res, kept = arbitrate_ref.arbitrate(hyp, T, img, CAM, tile_spacing=ts, min_owned_share=min_owned_share)
            rest = [raw[j]["share"] for j in found if j not in (0, TWIN)]
            row["spacing"][ts] = dict(tile=raw[0]["tile"], present=raw[0], twin=raw[TWIN],
                                      rest_share=float(max(rest)) if rest else None,
                                      kept=[int(j) for j in np.flatnonzero(kept)],
                                      present_final=res[0], twin_final=res[TWIN])
        rows.append(row)
    return rows


def format_rows(rows):
    out = []
    for f, row in enumerate(rows):
        for ts, c in row["spacing"].items():
            p, t = c["present"], c["twin"]
            out.append("%d %-3s found %-12s spacing %.0f tile %3d   0: share %.3f resid %.4f   36: share %.3f resid %.4f   rest %s  kept %s"
                       % (f, "occ" if row["occluded"] else "", row["found"], ts, c["tile"], p["share"], p["mean_residual"],
                          t["share"], t["mean_residual"], c["rest_share"], c["kept"]))
    return "\n".join(out)
