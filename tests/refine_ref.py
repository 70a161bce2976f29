"""Numpy restatement of the refinement stage (include/oslam.h at oslam_refine): the yardstick of the device path.

Correspondences are computed in float32 with the header's operation order by brute force over the scene points whose
x lies within the radius (the rest cannot qualify), so they equal the device's bit for bit.  The step sums in float64
(the device sums in float per workgroup of 256 model points, then in double), so poses agree to rounding, not to
the bit.  numpy only: it runs wherever the tests do.
"""
import numpy as np

BIG = np.iinfo(np.int32).max


def default_params():
    return dict(max_iterations=30, max_corr_dist=2.0, min_normal_dot=0.8, inlier_dist=0.5, min_fitness=0.3,
                stop_rot=1e-5, stop_trans=1e-4)


def transform_f32(T, p, n):
    """p' = ((R00 x + R01 y) + R02 z) + t0 ... and n' without t, all in float32."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    p = np.asarray(p, np.float32)
    n = np.asarray(n, np.float32)
    q = np.empty_like(p)
    m = np.empty_like(n)
    for a in range(3):
        q[:, a] = ((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3]
        m[:, a] = (T[a, 0] * n[:, 0] + T[a, 1] * n[:, 1]) + T[a, 2] * n[:, 2]
    return q, m


def correspondences(q, m, sp, sn, radius, min_dot):
    """(idx int32 [M], d2 float32 [M]) of transformed model points q (normals m); idx -1 = none."""
    sp = np.asarray(sp, np.float32)
    sn = np.asarray(sn, np.float32)
    r = np.float32(radius)
    r2 = r * r
    md = np.float32(min_dot)
    order = np.argsort(sp[:, 0], kind="stable")
    sx = sp[order, 0].astype(np.float64)
    spo, sno = sp[order], sn[order]
    qo = np.argsort(q[:, 0], kind="stable")
    idx = np.full(len(q), -1, np.int32)
    d2o = np.full(len(q), np.inf, np.float32)
    margin = float(r) * 1.001 + 1e-30
    i = 0
    while i < len(q):
        k = 256
        while True:
            rows = qo[i:i + k]
            lo = np.searchsorted(sx, float(q[rows, 0].min()) - margin, "left")
            hi = np.searchsorted(sx, float(q[rows, 0].max()) + margin, "right")
            if k <= 4 or (hi - lo) * len(rows) <= 4_000_000:
                break
            k //= 2
        i += len(rows)
        if hi <= lo:
            continue
        cp, cn, ci = spo[lo:hi], sno[lo:hi], order[lo:hi]
        qq, mm = q[rows], m[rows]
        dx = cp[None, :, 0] - qq[:, None, 0]
        dy = cp[None, :, 1] - qq[:, None, 1]
        dz = cp[None, :, 2] - qq[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        dot = (mm[:, None, 0] * cn[None, :, 0] + mm[:, None, 1] * cn[None, :, 1]) + mm[:, None, 2] * cn[None, :, 2]
        ok = (d2 <= r2) & (dot >= md)
        d2m = np.where(ok, d2, np.float32(np.inf))
        best = d2m.min(axis=1)
        tie = ok & (d2m == best[:, None])
        bi = np.where(tie, ci[None, :], BIG).min(axis=1)
        has = np.isfinite(best)
        idx[rows[has]] = bi[has]
        d2o[rows[has]] = best[has]
    return idx, d2o


def score(mp, mn, sp, sn, Tf, radius, min_dot):
    q, m = transform_f32(Tf, mp, mn)
    idx, d2 = correspondences(q, m, sp, sn, radius, min_dot)
    ok = idx >= 0
    n_in = int(ok.sum())
    rmse = float(np.sqrt(d2[ok].astype(np.float64).sum() / n_in)) if n_in else 0.0
    return n_in / float(len(mp)), n_in, rmse


def rodrigues(w):
    th = float(np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))
    if th <= 0.0:
        return np.eye(3), th
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * np.outer(k, k), th


def gram_schmidt_columns(R):
    R = R.copy()
    for c in range(3):
        for p in range(c):
            R[:, c] -= (R[:, p] @ R[:, c]) * R[:, p]
        R[:, c] /= np.sqrt(R[:, c] @ R[:, c])
    return R


def refine(mp, mn, sp, sn, T_in, d_dist, **kw):
    """-> (T_out float32 4x4, dict fitness_in fitness rmse inliers correspondences iterations converged found)."""
    p = default_params()
    p.update(kw)
    mp = np.asarray(mp, np.float32)
    mn = np.asarray(mn, np.float32)
    d = np.float32(d_dist)
    rc = np.float32(p["max_corr_dist"]) * d
    rs = np.float32(p["inlier_dist"]) * d
    md = p["min_normal_dot"]
    cm = mp.astype(np.float64).mean(axis=0)
    T = np.asarray(T_in, np.float32).reshape(4, 4).astype(np.float64)
    Tf = np.asarray(T_in, np.float32).reshape(4, 4).copy()
    fit_in = score(mp, mn, sp, sn, Tf, rs, md)[0]
    it, converged, n_corr = 0, False, 0
    while it < p["max_iterations"]:
        q, m = transform_f32(Tf, mp, mn)
        idx, _ = correspondences(q, m, sp, sn, rc, md)
        ok = idx >= 0
        n_corr = int(ok.sum())
        if n_corr < 6:
            break
        P, Q, N = q[ok], np.asarray(sp, np.float32)[idx[ok]], np.asarray(sn, np.float32)[idx[ok]]
        c = (T[:3, :3] @ cm + T[:3, 3]).astype(np.float32)
        e = P - Q
        r = (N[:, 0] * e[:, 0] + N[:, 1] * e[:, 1]) + N[:, 2] * e[:, 2]
        J = np.concatenate([np.cross(P - c, N), N], axis=1).astype(np.float64)
        A = J.T @ J
        g = J.T @ r.astype(np.float64)
        A = A + 1e-6 * np.trace(A) / 6.0 * np.eye(6)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            break
        x = np.linalg.solve(L.T, np.linalg.solve(L, -g))
        dR, th = rodrigues(x[:3])
        R, t = T[:3, :3], T[:3, 3]
        cd = R @ cm + t
        Rn = gram_schmidt_columns(dR @ R)
        tn = dR @ t + (cd - dR @ cd + x[3:])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rn, tn
        Tf = T.astype(np.float32)
        Tf[3] = [0, 0, 0, 1]
        it += 1
        if th < p["stop_rot"] and np.linalg.norm(x[3:]) < p["stop_trans"] * float(d):
            converged = True
            break
    fit, n_in, rmse = score(mp, mn, sp, sn, Tf, rs, md)
    return Tf, dict(fitness_in=fit_in, fitness=fit, rmse=rmse, inliers=n_in, correspondences=n_corr, iterations=it,
                    converged=converged, found=fit >= p["min_fitness"])


def pose_error(T, truth):
    """(rotation error in degrees, translation error) of a 4x4 against the ground truth, float64."""
    T = np.asarray(T, np.float64)
    G = np.asarray(truth, np.float64)
    Rd = T[:3, :3] @ G[:3, :3].T
    # atan2 of the skew and symmetric parts: arccos of the trace alone loses small angles to rounding
    s = np.linalg.norm([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]) / 2
    ang = np.degrees(np.arctan2(s, (np.trace(Rd) - 1) / 2))
    return float(ang), float(np.linalg.norm(T[:3, 3] - G[:3, 3]))
