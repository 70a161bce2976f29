"""Numpy restatement of the camera motion stage (include/oslam.h at oslam_view_egomotion) and the static world of its
tests: the yardstick of the device path.

The maps are track_ref.view_maps.  The correspondence rule is computed in float32 with the header's operation order, so
the tap can be compared exactly.  The sums of the step exist twice: "f64" (float64 products of the float32 Jacobian) and
"f32" (the 29 float32 terms of every lattice index through the header's pinned order: the tree over 64, the four 64s of a
block, then double over chunks, slots and strands).  numpy only: it runs wherever the tests do.
"""
import math

import numpy as np

import refine_ref
import track_ref as K

F = np.float32
THREADS, MAX_SLOTS, STRANDS = 256, 256, 8
CAM = K.STREAM_CAM
MAX_JUMP = K.STREAM_MAX_JUMP


def default_params():
    """oslam_egomotion_params_default."""
    return dict(levels=[(4, 4), (2, 5), (1, 10)], max_corr_dist=0.30, min_normal_dot=float(F(0.93969262)), stop_rot=1e-5,
                stop_trans=1e-5, min_overlap=0.75)


# the bounds of tests/test_camera_host.py (its calibration table: three times the largest value measured over three seeds)
ROT_BOUND, TRANS_BOUND = 0.037, 0.0024                  # frame to frame: degrees, metres
CHAIN_ROT_BOUND, CHAIN_TRANS_BOUND = 0.29, 0.0192       # chained over 9 frames
OVERLAP_CONSECUTIVE_MIN, OVERLAP_UNRELATED_MAX = 0.80, 0.70


# ---------------------------------------------------------------- the rule
def lattice(maps, stride):
    """The selected pixels of a level, row-major over the lattice: (p [n,3], n [n,3], has [n])."""
    V, N, ok = maps
    return V[::stride, ::stride].reshape(-1, 3), N[::stride, ::stride].reshape(-1, 3), ok[::stride, ::stride].reshape(-1)


def correspondences(src_maps, dst_maps, T, dst_cam, radius, min_dot, stride=1):
    """-> (pixel int32 [n]: v * w + u in dst of every lattice index, -1 none; q: the transformed points; has: the source
    pixel has a normal)."""
    p, n, has = lattice(src_maps, stride)
    V, N, ok = dst_maps
    h, w = ok.shape
    q, m = refine_ref.transform_f32(T, p, n)
    pz = q[:, 2]
    with np.errstate(all="ignore"):
        fu = np.floor(((q[:, 0] * F(dst_cam["fx"])) / pz + F(dst_cam["cx"])) + F(0.5))
        fv = np.floor(((q[:, 1] * F(dst_cam["fy"])) / pz + F(dst_cam["cy"])) + F(0.5))
        inside = has & (pz >= F(dst_cam["z_min"])) & (pz <= F(dst_cam["z_max"])) & (fu >= F(0)) & (fu < F(w)) & \
            (fv >= F(0)) & (fv < F(h))
    u = np.where(inside, fu, 0).astype(np.int64)
    v = np.where(inside, fv, 0).astype(np.int64)
    a, b = V[v, u], N[v, u]
    r = F(radius)
    d = a - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    nd = (m[:, 0] * b[:, 0] + m[:, 1] * b[:, 1]) + m[:, 2] * b[:, 2]
    good = inside & ok[v, u] & (d2 <= r * r) & (nd >= F(min_dot))
    return np.where(good, v * w + u, -1).astype(np.int32), q, has


def pinned_sums(terms):
    """terms float32 [n, k] (zeros where an index has no correspondence) -> float64 [k] in the header's order."""
    n, k = terms.shape
    nb = (n + THREADS - 1) // THREADS
    blocks = refine_ref.block_sums_f32(terms).astype(np.float64)          # the tree over 64, the four 64s of a block
    chunk = (nb + MAX_SLOTS - 1) // MAX_SLOTS
    G = (nb + chunk - 1) // chunk
    slots = np.zeros((G, k))
    for g in range(G):
        for b in range(g * chunk, min((g + 1) * chunk, nb)):
            slots[g] = slots[g] + blocks[b]
    strands = np.zeros((STRANDS, k))
    for j in range(STRANDS):
        for g in range(j, G, STRANDS):
            strands[j] = strands[j] + slots[g]
    s = strands[0]
    for j in range(1, STRANDS):
        s = s + strands[j]
    return s


def egomotion(src_maps, dst_maps, dst_cam, T_init=None, sums="f64", **kw):
    """-> (T float32 4x4, dict iterations [per level] correspondences rmse overlap converged ok cond: the condition
    number of J^T J of the first step, undamped)."""
    assert sums in ("f64", "f32")
    p = default_params()
    p.update(kw)
    Vd, Nd = dst_maps[0].reshape(-1, 3), dst_maps[1].reshape(-1, 3)
    Tf = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32).reshape(4, 4).copy()
    T = Tf.astype(np.float64)
    levels = list(p["levels"])
    iterations = [0] * len(levels)
    corr, nsrc, ran = [0] * len(levels), [0] * len(levels), [False] * len(levels)
    n_corr, rmse, converged, done, cond = 0, 0.0, False, False, 0.0
    for L, (stride, max_it) in enumerate(levels):
        if done:
            break
        T = Tf.astype(np.float64)                         # a level starts from the float32 pose the last one left
        it = 0
        while it < max_it:
            pix, q, has = correspondences(src_maps, dst_maps, Tf, dst_cam, p["max_corr_dist"], p["min_normal_dot"], stride)
            ok = pix >= 0
            sel = np.where(ok, pix, 0)
            Q, Nq = Vd[sel], Nd[sel]
            c = T[:3, 3].astype(np.float32)
            e = q - Q
            r = (Nq[:, 0] * e[:, 0] + Nq[:, 1] * e[:, 1]) + Nq[:, 2] * e[:, 2]
            Jf = np.concatenate([np.cross(q - c, Nq), Nq], axis=1).astype(np.float32)
            if sums == "f32":
                cols = [Jf[:, a] * Jf[:, b] for a in range(6) for b in range(a, 6)] + [Jf[:, a] * r for a in range(6)] + \
                    [np.ones(len(r), np.float32), r * r]
                terms = np.stack(cols, axis=1).astype(np.float32)
                terms[~ok] = 0
                S = pinned_sums(terms)
            else:
                J, rr = Jf[ok].astype(np.float64), r[ok].astype(np.float64)
                JtJ = J.T @ J
                S = np.concatenate([[JtJ[a, b] for a in range(6) for b in range(a, 6)], J.T @ rr, [float(ok.sum()), rr @ rr]])
            n_corr = int(S[27])
            assert n_corr == int(ok.sum())
            rmse = float(np.sqrt(F(S[28] / S[27]))) if n_corr else 0.0
            corr[L], nsrc[L], ran[L] = n_corr, int(has.sum()), True
            if n_corr < 6:
                done = True
                converged = False
                break
            A = np.zeros((6, 6))
            k = 0
            for a in range(6):
                for b in range(a, 6):
                    A[a, b] = A[b, a] = S[k]
                    k += 1
            g = S[21:27]
            if cond == 0.0:
                cond = float(np.linalg.cond(A))
            A = A + 1e-6 * np.trace(A) / 6.0 * np.eye(6)
            try:
                Lc = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                done = True
                converged = False
                break
            x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g))
            dR, th = refine_ref.rodrigues(x[:3])
            R, t = T[:3, :3], T[:3, 3]
            Rn = refine_ref.gram_schmidt_columns(dR @ R)
            tn = dR @ t + (t - dR @ t + x[3:])
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rn, tn
            Tf = T.astype(np.float32)
            Tf[3] = [0, 0, 0, 1]
            it += 1
            iterations[L] = it
            converged = bool(th < F(p["stop_rot"]) and np.linalg.norm(x[3:]) < F(p["stop_trans"]))
            if converged:
                break
    finest = -1
    for L, (stride, _) in enumerate(levels):
        if ran[L] and (finest < 0 or stride <= levels[finest][0]):
            finest = L
    overlap = float(F(corr[finest]) / F(nsrc[finest])) if finest >= 0 and nsrc[finest] else 0.0
    return Tf, dict(iterations=iterations, correspondences=n_corr, rmse=rmse, overlap=overlap, converged=int(converged),
                    ok=int(overlap >= F(p["min_overlap"])), cond=cond)


# ---------------------------------------------------------------- the static world and the moving camera
WORLD_DEPTH = 6.0               # the back wall, metres before the first camera
OBJECT_SCALE = 0.3              # the synth models are about 4 units wide


def make_world(synth, seed=0, planes_only=False, one_plane=False):
    """A static world in the coordinates of the first camera (x right, y down, z forward), densely sampled: a floor at
    y = 1.5, a back wall at z = WORLD_DEPTH (+ 0.4 * seed, so that another seed is another world), a side wall at
    x = -2.5 and three synth objects standing before the wall.  -> float64 [n, 3].  one_plane: the back wall alone, the
    degenerate case (three of the six degrees of freedom slide)."""
    zw = WORLD_DEPTH + 0.4 * seed
    gx, gy = np.meshgrid(np.arange(-6.0, 6.0, 0.01), np.arange(-4.5, 1.5, 0.01))
    parts = [np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, zw)], axis=1)]
    if one_plane:
        return parts[0]
    # the floor, sampled evenly in the image of the first camera: x = a z, z = 1 / s
    a, s = np.meshgrid(np.linspace(-1.1, 1.1, 1800), np.linspace(1.0 / zw, 1.0 / 1.6, 700))
    parts.append(np.stack([(a / s).ravel(), np.full(a.size, 1.5), (1.0 / s).ravel()], axis=1))
    gz, gy = np.meshgrid(np.arange(1.5, zw, 0.008), np.arange(-4.5, 1.5, 0.008))
    parts.append(np.stack([np.full(gz.size, -2.5), gy.ravel(), gz.ravel()], axis=1))
    if not planes_only:
        rng = synth.SplitMix64(500 + seed)
        for k, (x, z) in enumerate(((-1.6, 4.2), (0.2, 3.6), (1.7, 4.6))):
            pts, _ = synth.make_model(k + 3 * seed, 150000)
            R = synth.random_rotation(rng)
            parts.append(OBJECT_SCALE * (pts.astype(np.float64) @ R.T) + np.array([x, 0.9, z]))
    return np.concatenate(parts)


def object_pose(synth, seed, k):
    """The pose (model k of make_world's objects -> world) as make_world places it, with the scale left to the caller:
    the world's objects are OBJECT_SCALE times the synth model."""
    rng = synth.SplitMix64(500 + seed)
    R = None
    for _ in range(k + 1):
        R = synth.random_rotation(rng)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = [(-1.6, 0.2, 1.7)[k], 0.9, (4.2, 3.6, 4.6)[k]]
    return T


def trajectory(synth, seed=0, frames=10, deg=3.0, step=0.03):
    """Camera poses T_world_cam [frames] (float64 4x4), seeded and smooth: per frame `deg` degrees about a tilted axis
    near the vertical and `step` metres along a seeded direction; frame 0 is the world's frame."""
    rng = synth.SplitMix64(700 + seed)
    u = rng.uniform(6) * 2 - 1
    axis = np.array([0.3 * u[0], 1.0, 0.3 * u[1]]) * (1.0 if u[2] >= 0 else -1.0)
    dR = K.axis_rotation(axis, deg)
    dt = np.array([u[3], 0.3 * u[4], u[5]])
    dt = step * dt / np.linalg.norm(dt)
    out, T = [], np.eye(4)
    for _ in range(frames):
        out.append(T.copy())
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = dR, dt
        T = T @ D
    return out


def render(synth, world, T_world_cam, cam=None, **size):
    """uint16 depth frame of the world from the camera pose (pixels nothing projects to are invalid).  size: width,
    height and intrinsics of synth.render_depth for another camera."""
    Tc = np.linalg.inv(np.asarray(T_world_cam, np.float64))
    return synth.render_depth(world @ Tc[:3, :3].T + Tc[:3, 3], background_z=None, splat=1, **size)


def truth(T_wc_src, T_wc_dst):
    """Source camera coordinates -> destination camera coordinates (float64 4x4)."""
    return np.linalg.inv(T_wc_dst) @ T_wc_src


def mean_depth(maps):
    return float(maps[0][..., 2][maps[2]].astype(np.float64).mean())
