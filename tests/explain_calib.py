"""The calibration of the explain stage on the CPU (tests/test_explain_host.py): the seeded depth frames of
tests/verify_calib.py, the 11-member database of tests/arbitrate_calib.py (synthetic models 0..9 and 36, the near twin
of model 0), every member's voting pose from the oracle (df 4), refined by tests/refine_ref.py and verified by
tests/view_ref.py, then judged by tests/explain_ref.py and, for comparison, tests/arbitrate_ref.py."""
import numpy as np

import arbitrate_calib
import explain_ref
import refine_ref
import verify_calib
import view_ref

MEMBERS = arbitrate_calib.MEMBERS
CAM = verify_calib.CAM
DEPTH_TOLS = (1.0, 0.5)
TILES = (0, 8)


def grids(synth, oracle, members=MEMBERS):
    """[(points, normals)] of the members, voxel-gridded at model 0's d_dist as arbitrate_calib.models does, and d."""
    raw = [synth.make_model(k, 1500) for k in members]
    d = synth.d_dist_for(synth.make_model(0, 1500)[0], 0.05)
    return [oracle.voxel_grid(p, n, d) for p, n in raw], d


def frames(synth, oracle, members=MEMBERS, n_frames=6, seed=211):
    """One dict per frame: img, truth, occluded, T [len(members), 4, 4] (the refined pose of every member that got a
    voting pose, zeros otherwise), verify (its result, None without a pose) and found (indices into members)."""
    gs, d = grids(synth, oracle, members)
    out = []
    for img, truth, occluded in verify_calib.frames(synth, n_frames, seed):
        sp, sn = oracle.depth_to_cloud(img, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["depth_scale"], CAM["z_min"],
                                       CAM["z_max"], verify_calib.MAX_JUMP)
        sp, sn = oracle.voxel_grid(sp, sn, d)
        T = np.zeros((len(gs), 4, 4), np.float32)
        ver, found = [None] * len(gs), []
        for j, (gp, gn) in enumerate(gs):
            cells, _ = oracle.votes_fused(gp, gn, sp, sn, 4, d, 0.4)
            _, T0 = oracle.pose_from_cells(cells, gp, gn, sp, sn, d)
            if not T0.any():
                continue
            T[j], _ = refine_ref.refine(gp, gn, sp, sn, T0, d)
            ver[j], _ = view_ref.verify(gp, gn, T[j], img, CAM, d)
            ver[j]["rot_err"] = refine_ref.pose_error(T[j], truth)[0]
            if ver[j]["found"]:
                found.append(j)
        out.append(dict(img=img, truth=truth, occluded=occluded, T=T, verify=ver, found=found))
    return out, [(gp, gn, d) for gp, gn in gs]


def only(T, keep):
    """T with every pose but those of `keep` zeroed: the hypotheses that compete."""
    out = np.zeros_like(T)
    for j in keep:
        out[j] = T[j]
    return out


def judge(hyp, frame, keep, depth_tol=1.0, tile=0, min_owned_share=0.52):
    """explain_ref.explain over the members `keep` of a frame: -> (first-round results with min_owned_share 0, final
    results under min_owned_share)."""
    T = only(frame["T"], keep)
    raw = explain_ref.explain(hyp, T, frame["img"], CAM, depth_tol=depth_tol, tile=tile, min_owned_share=0.0)
    res = explain_ref.explain(hyp, T, frame["img"], CAM, depth_tol=depth_tol, tile=tile, min_owned_share=min_owned_share)
    return raw, res


def rate(r):
    """through / (agree + through) of a result, None without either."""
    n = r["agree"] + r["through"]
    return r["through"] / n if n else None
