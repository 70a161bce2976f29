"""Numpy restatement of the refinement stage (include/oslam.h at oslam_refine): the yardstick of the device path.

Correspondences are computed in float32 with the header's operation order by brute force over the scene points whose
x lies within the radius (the rest cannot qualify), so they equal the device's bit for bit.  The step sums in float64
(the device sums in float per workgroup of 256 model points, then in double), so poses agree to rounding, not to
the bit; with sums="f32" the 29 (step) or 2 (score) float32 terms of every model index go through the device's own order
(block_sums_f32, then double over the workgroups) and the step is oslam_refine_step's operation by operation
(step_pinned), which leaves the device nothing to differ in but the last bit of sin and cos.  grid_shape, cell_of and
grid_walk restate the scene grid (scene_grid of oslam_refine.c, grid_axis and the 27-cell walk of oslam_refine.hip).
numpy only: it runs wherever the tests do.
"""
import math

import numpy as np

BIG = np.iinfo(np.int32).max
F = np.float32
THREADS = 256                   # OSLAMK_REFINE_THREADS: model points per workgroup
SCAN_ITEMS = 4096               # OSLAMK_SCAN_ITEMS: grid cells per workgroup of k_scan_local
SCAN_TOP_THREADS = 1024         # k_scan_top: one workgroup, ceil(nb / 1024) block totals per thread
GRID_MAX_CELLS = 1 << 24        # OSLAMK_GRID_MAX_CELLS


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


# ---------------------------------------------------------------- the scene grid
def grid_shape(sp, radius):
    """scene_grid of oslam_refine.c for a scene's points and a radius, in float64 with its expressions: dict(dims,
    n_cells, nb = workgroups of k_scan_local over n_cells + 1 items, per = block totals per thread of k_scan_top, edge,
    inv_edge, clamped: the edge was enlarged to stay within GRID_MAX_CELLS, lo)."""
    sp = np.asarray(sp, np.float32).astype(np.float64)
    lo, hi = sp.min(axis=0), sp.max(axis=0)
    edge0 = float(F(radius)) * (1.0 + 1e-4)
    edge = edge0
    while True:
        cells = 1.0
        for a in range(3):
            cells *= math.floor((hi[a] - lo[a]) / edge) + 1.0
        if cells <= float(GRID_MAX_CELLS):
            break
        edge *= float(np.cbrt(cells / float(GRID_MAX_CELLS))) * 1.01
    inv = 1.0 / edge
    dims = tuple(int(math.floor((hi[a] - lo[a]) * inv)) + 1 for a in range(3))
    n_cells = dims[0] * dims[1] * dims[2]
    nb = (n_cells + 1 + SCAN_ITEMS - 1) // SCAN_ITEMS
    return dict(dims=dims, n_cells=n_cells, nb=nb, per=(nb + SCAN_TOP_THREADS - 1) // SCAN_TOP_THREADS, edge=edge,
                inv_edge=inv, clamped=edge != edge0, lo=lo)


def cell_of(x, shape):
    """grid_axis of every coordinate: int64 [n, 3], floor((x - lo) * inv_edge) in float64 clamped to [-2, dim + 1]
    (NaN -> -2, as fmax does).  A query walks the cells max(c - 1, 0) .. min(c + 1, dim - 1) of every axis."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        f = np.floor((x - shape["lo"]) * shape["inv_edge"])
        f = np.minimum(np.maximum(f, -2.0), np.asarray(shape["dims"], np.float64) + 1.0)
    return np.where(np.isnan(f), -2.0, f).astype(np.int64)


def cell_index(x, shape):
    """The linear cell (z, y, x order) k_grid_count puts a scene point into: cell_of clamped into the grid."""
    c = np.clip(cell_of(x, shape), 0, np.asarray(shape["dims"]) - 1)
    return (c[:, 2] * shape["dims"][1] + c[:, 1]) * shape["dims"][0] + c[:, 0]


def grid_walk(q, m, sp, sn, radius, min_dot, shape, rule="lowest"):
    """The correspondences as k_refine_corr finds them: the 27-cell walk over the grid `shape` in z, y, x cell order,
    the points of a cell in index order (the device: in the order they arrived).  -> (idx int32 [M], first int32 [M]:
    the first candidate met among those tied for the smallest distance).  rule: "lowest" is the device's; the others are
    wrong on purpose, for the tests that show the inputs tell them apart: "first" keeps the first tied candidate met,
    "open" tests d2 < r2, "inside" walks nothing when a cell coordinate is -1 or dim."""
    sp, sn = np.asarray(sp, np.float32), np.asarray(sn, np.float32)
    dims = shape["dims"]
    r = F(radius)
    r2, md = r * r, F(min_dot)
    cells = {}
    for i, c in enumerate(cell_index(sp, shape)):
        cells.setdefault(int(c), []).append(i)
    cq = cell_of(q, shape)
    idx = np.full(len(q), -1, np.int32)
    first = np.full(len(q), -1, np.int32)
    for i in range(len(q)):
        if rule == "inside" and any(cq[i, a] in (-1, dims[a]) for a in range(3)):
            continue
        rng = [range(max(int(cq[i, a]) - 1, 0), min(int(cq[i, a]) + 1, dims[a] - 1) + 1) for a in range(3)]
        cand = [k for zz in rng[2] for yy in rng[1] for xx in rng[0] for k in cells.get((zz * dims[1] + yy) * dims[0] + xx, ())]
        if not cand:
            continue
        cand = np.asarray(cand)
        d = sp[cand] - q[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        b = sn[cand]
        dot = (m[i, 0] * b[:, 0] + m[i, 1] * b[:, 1]) + m[i, 2] * b[:, 2]
        ok = ((d2 < r2) if rule == "open" else (d2 <= r2)) & (dot >= md)
        if not ok.any():
            continue
        tied = cand[ok & (d2 == d2[ok].min())]
        first[i] = tied[0]
        idx[i] = tied[0] if rule == "first" else tied.min()
    return idx, first


# ---------------------------------------------------------------- the pinned sums
def block_sums_f32(terms):
    """terms float32 [n, k] (zeros where an index has no correspondence) -> float32 [ceil(n / 256), k]: every block of
    256 indices summed in the order of oslam_icp_block_sums, the shfl_down tree over each 64, then the four 64s in
    index order."""
    terms = np.asarray(terms, np.float32)
    n, k = terms.shape
    nb = (n + THREADS - 1) // THREADS
    t = np.zeros((nb * THREADS, k), np.float32)
    t[:n] = terms
    t = t.reshape(nb, THREADS // 64, 64, k)
    for off in (32, 16, 8, 4, 2, 1):
        t[:, :, :off] = t[:, :, :off] + t[:, :, off:2 * off]
    wv = t[:, :, 0]                                       # [nb, 4, k]
    return ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]


def member_sums(terms):
    """float64 [k]: block_sums_f32, then a running float64 sum over the blocks in order (k_refine_solve, and the host
    loop of oslam_refine_members over the score slabs)."""
    S = np.zeros(terms.shape[1], np.float64)
    for b in block_sums_f32(terms).astype(np.float64):
        S = S + b
    return S


def score(mp, mn, sp, sn, Tf, radius, min_dot, sums="f64"):
    """-> (fitness, inliers, rmse).  sums="f32": the device's sums and the host's float32 roundings, bit for bit."""
    assert sums in ("f64", "f32")
    q, m = transform_f32(Tf, mp, mn)
    idx, d2 = correspondences(q, m, sp, sn, radius, min_dot)
    ok = idx >= 0
    if sums == "f32":
        terms = np.zeros((len(q), 2), np.float32)
        terms[ok, 0] = 1.0
        terms[ok, 1] = d2[ok]
        n, s = member_sums(terms)
        return float(F(n / float(len(q)))), int(n), (float(F(math.sqrt(s / n))) if n > 0.0 else 0.0)
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


def step_terms(q, Q, N, c, ok):
    """The 29 float32 terms of oslam_refine_point_sums for every model index (zeros where not ok): transformed points q,
    their correspondences Q with normals N, the transformed centroid c."""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        e = q - Q
        r = (N[:, 0] * e[:, 0] + N[:, 1] * e[:, 1]) + N[:, 2] * e[:, 2]
        u = q - c
        J = [u[:, 1] * N[:, 2] - u[:, 2] * N[:, 1], u[:, 2] * N[:, 0] - u[:, 0] * N[:, 2],
             u[:, 0] * N[:, 1] - u[:, 1] * N[:, 0], N[:, 0], N[:, 1], N[:, 2]]
        cols = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + \
            [np.ones(len(r), np.float32), r * r]
    terms = np.stack(cols, axis=1).astype(np.float32)
    terms[~ok] = 0
    return terms


def terms_at(mp, mn, sp, sn, Tf, d_dist, **kw):
    """(step_terms, ok) of one correspondence pass at the float32 pose Tf, as the first iteration of refine computes them"""
    p = default_params()
    p.update(kw)
    mp, mn = np.asarray(mp, np.float32), np.asarray(mn, np.float32)
    sp, sn = np.asarray(sp, np.float32), np.asarray(sn, np.float32)
    Tf = np.asarray(Tf, np.float32).reshape(4, 4)
    cm = [float(v) / float(len(mp)) for v in np.cumsum(mp.astype(np.float64), axis=0)[-1]]
    q, m = transform_f32(Tf, mp, mn)
    idx, _ = correspondences(q, m, sp, sn, F(p["max_corr_dist"]) * F(d_dist), p["min_normal_dot"])
    ok = idx >= 0
    sel = np.where(ok, idx, 0)
    return step_terms(q, sp[sel], sn[sel], centre_f32([[float(v) for v in Tf[a]] for a in range(3)], cm), ok), ok


def _rot(R, x):
    return [(R[a][0] * x[0] + R[a][1] * x[1]) + R[a][2] * x[2] for a in range(3)]


def centre_f32(T, cm):
    """float32 of T cm in the order of set_pose and of the step's last lines; T: rows of [R | t] in float64"""
    return np.array([F(v + T[a][3]) for a, v in enumerate(_rot(T, cm))], np.float32)


def system_of(S):
    """the 29 sums -> (A 6x6 symmetric, undamped; g = the sums of J^T r)"""
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = S[k]
            k += 1
    return A, np.asarray(S[21:27], np.float64)


def step_pinned(S, T, cm):
    """oslam_refine_step in Python floats (IEEE double, nothing contracted), operation by operation: the damped Cholesky,
    Rodrigues, the update about the transformed centroid, Gram-Schmidt.  T: 3 rows of [R | t].  -> None when fewer than 6
    correspondences or a failed factorisation stop the member, else (T stepped, |omega|, |v|)."""
    if S[27] < 6.0:
        return None
    A = [[float(v) for v in row] for row in system_of(S)[0]]
    mu = 1e-6 * (((((A[0][0] + A[1][1]) + A[2][2]) + A[3][3]) + A[4][4]) + A[5][5]) / 6.0
    for u in range(6):
        A[u][u] += mu
    L = [[0.0] * 6 for _ in range(6)]
    for u in range(6):
        for v in range(u + 1):
            t = A[u][v]
            for k in range(v):
                t -= L[u][k] * L[v][k]
            if u == v:
                if not t > 0.0:
                    return None
                L[u][u] = math.sqrt(t)
            else:
                L[u][v] = t / L[v][v]
    y, x = [0.0] * 6, [0.0] * 6
    for u in range(6):
        t = -float(S[21 + u])
        for k in range(u):
            t -= L[u][k] * y[k]
        y[u] = t / L[u][u]
    for u in range(5, -1, -1):
        t = y[u]
        for k in range(u + 1, 6):
            t -= L[k][u] * x[k]
        x[u] = t / L[u][u]
    th = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    dR = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if th > 0.0:
        kx, ky, kz = x[0] / th, x[1] / th, x[2] / th
        cs, sn = math.cos(th), math.sin(th)
        vc = 1.0 - cs
        dR = [[cs + kx * kx * vc, kx * ky * vc - kz * sn, kx * kz * vc + ky * sn],
              [ky * kx * vc + kz * sn, cs + ky * ky * vc, ky * kz * vc - kx * sn],
              [kz * kx * vc - ky * sn, kz * ky * vc + kx * sn, cs + kz * kz * vc]]
    R = [[T[a][0], T[a][1], T[a][2]] for a in range(3)]
    t = [T[a][3] for a in range(3)]
    c = [v + t[a] for a, v in enumerate(_rot(R, cm))]
    dRc, dRt = _rot(dR, c), _rot(dR, t)
    Rn = [[(dR[a][0] * R[0][b] + dR[a][1] * R[1][b]) + dR[a][2] * R[2][b] for b in range(3)] for a in range(3)]
    tn = [dRt[a] + ((c[a] - dRc[a]) + x[3 + a]) for a in range(3)]
    for col in range(3):
        for prev in range(col):
            p = (Rn[0][prev] * Rn[0][col] + Rn[1][prev] * Rn[1][col]) + Rn[2][prev] * Rn[2][col]
            for a in range(3):
                Rn[a][col] -= p * Rn[a][prev]
        nrm = math.sqrt((Rn[0][col] * Rn[0][col] + Rn[1][col] * Rn[1][col]) + Rn[2][col] * Rn[2][col])
        for a in range(3):
            Rn[a][col] /= nrm
    return [Rn[a] + [tn[a]] for a in range(3)], th, math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])


def _refine_f32(mp, mn, sp, sn, T_in, d, p):
    """refine with the device's sums, step and float32 roundings (oslam_refine_members, k_refine_corr, k_refine_solve)"""
    sp, sn = np.asarray(sp, np.float32), np.asarray(sn, np.float32)
    rc, rs, md = F(p["max_corr_dist"]) * d, F(p["inlier_dist"]) * d, p["min_normal_dot"]
    stop_rot, stop_trans = float(F(p["stop_rot"])), float(F(p["stop_trans"]) * d)
    cm = [float(v) / float(len(mp)) for v in np.cumsum(mp.astype(np.float64), axis=0)[-1]]      # summed in index order
    Tf = np.asarray(T_in, np.float32).reshape(4, 4).copy()
    T = [[float(v) for v in Tf[a]] for a in range(3)]
    c = centre_f32(T, cm)
    fit_in = score(mp, mn, sp, sn, Tf, rs, md, "f32")[0]
    it, converged, n_corr, cond = 0, False, 0, 0.0
    while it < p["max_iterations"]:
        q, m = transform_f32(Tf, mp, mn)
        idx, _ = correspondences(q, m, sp, sn, rc, md)
        ok = idx >= 0
        sel = np.where(ok, idx, 0)
        S = member_sums(step_terms(q, sp[sel], sn[sel], c, ok))
        n_corr = int(S[27])
        assert n_corr == int(ok.sum())
        if cond == 0.0 and n_corr >= 6:
            cond = float(np.linalg.cond(system_of(S)[0]))
        stepped = step_pinned(S, T, cm)
        if stepped is None:
            break
        T, th, vn = stepped
        Tf = np.eye(4, dtype=np.float32)
        Tf[:3] = np.asarray(T, np.float64).astype(np.float32)
        c = centre_f32(T, cm)
        it += 1
        if th < stop_rot and vn < stop_trans:
            converged = True
            break
    fit, n_in, rmse = score(mp, mn, sp, sn, Tf, rs, md, "f32")
    return Tf, dict(fitness_in=fit_in, fitness=fit, rmse=rmse, inliers=n_in, correspondences=n_corr, iterations=it,
                    converged=converged, found=bool(F(fit) >= F(p["min_fitness"])), cond=cond)


def refine(mp, mn, sp, sn, T_in, d_dist, sums="f64", **kw):
    """-> (T_out float32 4x4, dict fitness_in fitness rmse inliers correspondences iterations converged found cond: the
    condition number of J^T J of the first step, undamped).  sums="f32": every float sequence of the device."""
    assert sums in ("f64", "f32")
    p = default_params()
    p.update(kw)
    if sums == "f32":
        return _refine_f32(np.asarray(mp, np.float32), np.asarray(mn, np.float32), sp, sn, T_in, np.float32(d_dist), p)
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
    it, converged, n_corr, cond = 0, False, 0, 0.0
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
        if cond == 0.0:
            cond = float(np.linalg.cond(A))
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
                    converged=converged, found=fit >= p["min_fitness"], cond=cond)


def pose_error(T, truth):
    """(rotation error in degrees, translation error) of a 4x4 against the ground truth, float64."""
    T = np.asarray(T, np.float64)
    G = np.asarray(truth, np.float64)
    Rd = T[:3, :3] @ G[:3, :3].T
    # atan2 of the skew and symmetric parts: arccos of the trace alone loses small angles to rounding
    s = np.linalg.norm([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]) / 2
    ang = np.degrees(np.arctan2(s, (np.trace(Rd) - 1) / 2))
    return float(ang), float(np.linalg.norm(T[:3, 3] - G[:3, 3]))
