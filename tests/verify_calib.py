"""The calibration of the verification defaults on the CPU (tests/test_verify_host.py): seeded depth frames like the
db50 stream, every model's voting pose from the oracle, refined by tests/refine_ref.py, scored by tests/view_ref.py."""
import numpy as np

import refine_ref
import view_ref

CAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=12.0)
MAX_JUMP = 0.08
N_MODELS = 10
OCCLUDER = 12          # a synthetic object outside the database


def frames(synth, n_frames=6, seed=211):
    """[(depth image, ground-truth pose of model 0, occluded?)]: model 0 at a random rotation in front of a wall at
    9 m; every other frame a second object (not a database member) partly covers it."""
    dense, _ = synth.make_model(0, 120000)
    occ, _ = synth.make_model(OCCLUDER, 60000)
    rng = synth.SplitMix64(seed)
    out = []
    for f in range(n_frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.9 * f), 0.3 * np.sin(0.9 * f), 5.5 + 0.15 * f]
        pts = dense @ T[:3, :3].T + T[:3, 3]
        occluded = f % 2 == 1
        if occluded:
            Ro = synth.random_rotation(rng)
            side = 1.0 if f % 4 == 1 else -1.0
            po = (0.6 * occ) @ Ro.T + (T[:3, 3] + np.array([side * 0.8, 0.2, -1.6]))
            pts = np.concatenate([pts, po])
        out.append((synth.render_depth(pts, background_z=9.0, splat=1), T, occluded))
    return out


def models(synth, oracle):
    raw = [synth.make_model(k, 1500) for k in range(N_MODELS)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    return [oracle.voxel_grid(p, n, d) for p, n in raw], d


def table(synth, oracle, n_frames=6, seed=211):
    """One row per frame: the present model's scores and the largest absent scores (each maximum taken over the
    absent members on its own), plus the refine fitness for comparison."""
    grids, d = models(synth, oracle)
    rows = []
    for img, truth, occluded in frames(synth, n_frames, seed):
        sp, sn = oracle.depth_to_cloud(img, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["depth_scale"], CAM["z_min"],
                                       CAM["z_max"], MAX_JUMP)
        sp, sn = oracle.voxel_grid(sp, sn, d)
        res = []
        for gp, gn in grids:
            cells, _ = oracle.votes_fused(gp, gn, sp, sn, 4, d, 0.4)
            _, T0 = oracle.pose_from_cells(cells, gp, gn, sp, sn, d)
            if not T0.any():
                res.append(None)
                continue
            T1, info = refine_ref.refine(gp, gn, sp, sn, T0, d)
            r, _ = view_ref.verify(gp, gn, T1, img, CAM, d)
            r["fitness"] = info["fitness"]
            r["rot_err"] = refine_ref.pose_error(T1, truth)[0]
            res.append(r)
        p = res[0]
        ab = [r for r in res[1:] if r is not None]
        rows.append(dict(occluded=occluded, present=p,
                         absent={k: max(r[k] for r in ab) for k in ("supported", "view_fitness", "coverage", "fitness")},
                         absent_found_pairs=[(r["supported"], round(r["view_fitness"], 3), round(r["coverage"], 3)) for r in ab]))
    return rows
