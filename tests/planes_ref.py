"""The rule of oslam_view_planes and oslam_view_remove_planes (include/oslam.h) restated in numpy, on top of
track_ref.view_maps: the yardstick of the device path.

Every float32 step is a separate numpy float32 operation with the header's grouping, every sum is a whole number and
the refit runs in Python floats (IEEE doubles; + - * / sqrt and comparisons only, each correctly rounded), so the plane
records, labels, per-round counts and moments equal the device's byte for byte.  A trace counts which branches of the
rule a call took.  numpy only: it runs wherever the tests do.
"""
import math

import numpy as np

import track_ref as K
import view_ref

F = np.float32
PLANES_MAX = 8
CANDIDATES = 256
SWEEPS = 4                      # OSLAM_NORMALS_SWEEPS
BOUND = F(131072.0)             # 2^17
LINE_RATIO = float(F(0.01))

PLANE_DTYPE = np.dtype([("normal", "<f4", 3), ("d", "<f4"), ("support", "<u4"), ("pixels", "<u4"), ("candidate", "<u4"),
                        ("rms", "<f4")])

TRACE_KEYS = ("end_min_pixels", "end_max_planes", "end_degenerate", "end_no_candidate", "node_no_normal", "node_labelled",
              "nodes_coincident", "winner_ties", "labelled_without_normal", "refused_by_label_dot", "out_of_moment_range")


def default_params():
    """oslam_planes_params_default."""
    return dict(dist_tol=0.02, min_normal_dot=0.9, label_min_dot=0.0, max_planes=4, min_pixels=0)


def new_trace():
    return {k: 0 for k in TRACE_KEYS}


def lattice(w, h):
    """(u [256], v [256]) of the lattice nodes, index 16 b + a."""
    a = np.arange(16)
    u, v = ((2 * a + 1) * w) // 32, ((2 * a + 1) * h) // 32
    return np.tile(u, 16), np.repeat(v, 16)


def points(z, cam):
    """p of every pixel from the z image: back_project, float32 with the header's grouping (0 where z is 0)."""
    h, w = z.shape
    u = np.arange(w, dtype=np.float32)[None, :]
    v = np.arange(h, dtype=np.float32)[:, None]
    z = np.ascontiguousarray(z, np.float32)
    P = np.stack([((u - F(cam["cx"])) * z) / F(cam["fx"]), ((v - F(cam["cy"])) * z) / F(cam["fy"]), z], axis=2)
    assert P.dtype == np.float32
    return P


def _rotate(A, V, p, q, r):
    """One Jacobi rotation on scalars: A a dict of the six elements by sorted pair, V[k][c] (oslam.h, normals step 4)."""
    key = lambda a, b: (a, b) if a < b else (b, a)
    apq = A[(p, q)]
    if apq == 0.0:
        return
    app, aqq = A[(p, p)], A[(q, q)]
    theta = (aqq - app) / (2.0 * apq)
    at = -theta if theta < 0.0 else theta
    tt = 1.0 / (at + math.sqrt(theta * theta + 1.0))
    t = -tt if theta < 0.0 else tt
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    hh = t * apq
    A[(p, p)] = app - hh
    A[(q, q)] = aqq + hh
    A[(p, q)] = 0.0
    x, y = A[key(r, p)], A[key(r, q)]
    A[key(r, p)] = c * x - s * y
    A[key(r, q)] = s * x + c * y
    for k in range(3):
        x, y = V[k][p], V[k][q]
        V[k][p] = c * x - s * y
        V[k][q] = s * x + c * y


def fit(m, p0, scale):
    """Step 3 after the sums: the ten integers m, the winner's point p0 (float32 [3]) and scale (float32) -> None for a
    degenerate fit, otherwise (normal float32 [3], d float32, rms float32)."""
    n = int(m[0])
    if n < 3:
        return None
    dn = float(n)
    mx, my, mz = float(int(m[1])) / dn, float(int(m[2])) / dn, float(int(m[3])) / dn
    A = {(0, 0): float(int(m[4])) / dn - mx * mx, (0, 1): float(int(m[5])) / dn - mx * my,
         (0, 2): float(int(m[6])) / dn - mx * mz, (1, 1): float(int(m[7])) / dn - my * my,
         (1, 2): float(int(m[8])) / dn - my * mz, (2, 2): float(int(m[9])) / dn - mz * mz}
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    a0, a1, a2 = A[(0, 0)], A[(1, 1)], A[(2, 2)]
    lo01, hi01 = (a0, a1) if a0 < a1 else (a1, a0)
    lmin = lo01 if lo01 < a2 else a2
    lmax = a2 if hi01 < a2 else hi01
    h2 = hi01 if hi01 < a2 else a2
    lmid = h2 if lo01 < h2 else lo01
    if lmid <= LINE_RATIO * lmax:
        return None
    col = 0 if (a0 <= a1 and a0 <= a2) else (1 if a1 <= a2 else 2)
    nx, ny, nz = V[0][col], V[1][col], V[2][col]
    ln = math.sqrt((nx * nx + ny * ny) + nz * nz)
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    sc = float(scale)
    cx, cy, cz = float(p0[0]) + mx / sc, float(p0[1]) + my / sc, float(p0[2]) + mz / sc
    if (nx * cx + ny * cy) + nz * cz > 0.0:
        nx, ny, nz = -nx, -ny, -nz
    d = -((nx * cx + ny * cy) + nz * cz)
    rms = math.sqrt(0.0 if lmin < 0.0 else lmin) / sc
    return np.array([nx, ny, nz]).astype(np.float32), F(d), F(rms)


def find(z, V, N, has, cam, dist_tol=0.02, min_normal_dot=0.9, label_min_dot=0.0, max_planes=4, min_pixels=0, trace=None):
    """oslam_view_planes on the z image [h,w] with its maps (track_ref.view_maps' V, N, has) -> dict(planes
    PLANE_DTYPE [n_planes], labels int32 [h,w], counts uint32 [max_planes,256], moments int64 [max_planes,10], n_planes,
    valid_in, labelled, end)."""
    assert 1 <= max_planes <= PLANES_MAX
    tr = trace if trace is not None else new_trace()
    z = np.ascontiguousarray(z, np.float32)
    h, w = z.shape
    tol, mnd, lmd = F(dist_tol), F(min_normal_dot), F(label_min_dot)
    scale = F(16.0) / tol
    minpix = int(min_pixels) if min_pixels else (w * h) // 50
    valid = z > 0
    P = points(z, cam)
    labels = np.full((h, w), -1, np.int32)
    counts = np.zeros((max_planes, CANDIDATES), np.uint32)
    moments = np.zeros((max_planes, 10), np.int64)
    planes = np.zeros(0, PLANE_DTYPE)
    lu, lv = lattice(w, h)
    assert lu.max() < w and lv.max() < h
    node_pix = lv * w + lu
    tr["nodes_coincident"] += CANDIDATES - len(np.unique(node_pix))
    end = "max_planes"
    with np.errstate(all="ignore"):
        for r in range(max_planes):
            free = valid & (labels < 0)
            fh = free & has
            node_lab = labels[lv, lu] >= 0
            ok = fh[lv, lu]
            tr["node_labelled"] += int(node_lab.sum())
            tr["node_no_normal"] += int((~node_lab & ~ok).sum())
            if not ok.any():
                end = "no_candidate"
                break
            px, py, pz = V[fh][:, 0], V[fh][:, 1], V[fh][:, 2]
            nx, ny, nz = N[fh][:, 0], N[fh][:, 1], N[fh][:, 2]
            seen = {}
            inl = None
            for c in np.flatnonzero(ok):
                if node_pix[c] in seen:                         # a coincident node: the same plane, the same count
                    counts[r, c] = counts[r, seen[node_pix[c]]]
                    continue
                seen[node_pix[c]] = c
                n0, p0 = N[lv[c], lu[c]], V[lv[c], lu[c]]
                d0 = -((n0[0] * p0[0] + n0[1] * p0[1]) + n0[2] * p0[2])
                dist = ((n0[0] * px + n0[1] * py) + n0[2] * pz) + d0
                dot = (n0[0] * nx + n0[1] * ny) + n0[2] * nz
                counts[r, c] = int(((np.abs(dist) <= tol) & (dot >= mnd)).sum())
            score = np.where(ok, counts[r].astype(np.int64), -1)
            win = int(np.argmax(score))                         # the first of the largest: the lowest index
            best = int(score[win])
            tr["winner_ties"] += int((score == best).sum() > 1)
            if best < minpix:
                end = "min_pixels"
                break
            n0, p0 = N[lv[win], lu[win]], V[lv[win], lu[win]]
            d0 = -((n0[0] * p0[0] + n0[1] * p0[1]) + n0[2] * p0[2])
            dist = ((n0[0] * px + n0[1] * py) + n0[2] * pz) + d0
            dot = (n0[0] * nx + n0[1] * ny) + n0[2] * nz
            inl = (np.abs(dist) <= tol) & (dot >= mnd)
            f = np.stack([(px[inl] - p0[0]) * scale, (py[inl] - p0[1]) * scale, (pz[inl] - p0[2]) * scale], axis=1)
            assert f.dtype == np.float32
            inb = (np.abs(f) <= BOUND).all(axis=1)
            tr["out_of_moment_range"] += int((~inb).sum())
            q = np.rint(f[inb]).astype(np.int64)
            qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
            m = [len(q), qx.sum(), qy.sum(), qz.sum(), (qx * qx).sum(), (qx * qy).sum(), (qx * qz).sum(), (qy * qy).sum(),
                 (qy * qz).sum(), (qz * qz).sum()]
            moments[r] = [int(x) for x in m]
            got = fit(moments[r], p0, scale)
            if got is None:
                end = "degenerate"
                break
            pn, pd, rms = got
            dist = ((pn[0] * P[..., 0] + pn[1] * P[..., 1]) + pn[2] * P[..., 2]) + pd
            dot = (pn[0] * N[..., 0] + pn[1] * N[..., 1]) + pn[2] * N[..., 2]
            near = free & (np.abs(dist) <= tol)
            facing = dot >= lmd
            hit = near & (~has | facing)
            tr["labelled_without_normal"] += int((hit & ~has).sum())
            tr["refused_by_label_dot"] += int((near & has & ~facing).sum())
            labels[hit] = r
            rec = np.zeros(1, PLANE_DTYPE)
            rec["normal"], rec["d"], rec["support"], rec["pixels"] = pn, pd, int(moments[r, 0]), int(hit.sum())
            rec["candidate"], rec["rms"] = win, rms
            planes = np.concatenate([planes, rec])
    tr["end_" + end] += 1
    return dict(planes=planes, labels=labels, counts=counts, moments=moments, n_planes=len(planes),
                valid_in=int(valid.sum()), labelled=int(planes["pixels"].sum()), end=end)


def find_in_depth(depth, cam, max_jump, **kw):
    """find() on a raw depth image (uint16 or float32) under cam (a dict with depth_scale, z_min, z_max): the view's z
    image and maps first -> (result, z)."""
    z = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    V, N, has = K.view_maps(depth, cam, max_jump)
    return find(z, V, N, has, cam, **kw), z


def remove(z, labels, mode="remove", only=-1):
    """oslam_view_remove_planes -> (z image, (valid_in, object_pixels, valid_out))."""
    valid = z > 0
    obj = valid & (labels >= 0) & ((labels == only) if only >= 0 else True)
    kept = valid & (obj if mode == "keep" else ~obj)
    return np.where(kept, z, F(0)).astype(np.float32), (int(valid.sum()), int(obj.sum()), int(kept.sum()))


def launches(max_planes, built):
    """The launch count of a call: four kernels per round for every round, plus the maps' kernel when they were built."""
    return 4 * int(max_planes) + (1 if built else 0)
