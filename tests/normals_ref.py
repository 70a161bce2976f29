"""The rule of oslam_cloud_normals and oslam_mesh_normals (include/oslam.h) restated in numpy.

Every float32 step is a separate numpy float32 operation and every double step a separate float64 operation, in the
operation order the header pins, so the device (built with -ffp-contract=off, correctly rounded / and sqrt) agrees bit
for bit.  The neighbour search is a grid of its own; the moments do not depend on it (they are whole numbers).
"""
import numpy as np

F = np.float32
SWEEPS = 4                      # OSLAM_NORMALS_SWEEPS
LINE_RATIO = 0.01               # oslam_normals_params_default
MIN_NEIGHBOURS = 5


def _pairs(xyz, radius, chunk=1 << 15):
    """Yields (i, j) index arrays that cover every pair of finite points less than two cells apart, i in chunks."""
    p = np.asarray(xyz, F)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    if len(fin) == 0:
        return
    q = p[fin].astype(np.float64)
    edge = float(radius) * 1.001
    lo = q.min(axis=0)
    span = q.max(axis=0) - lo
    while np.prod(np.floor(span / edge) + 3.0) > 2.0 ** 40:
        edge *= 2.0
    cell = np.floor((q - lo) / edge).astype(np.int64) + 1
    dim = cell.max(axis=0) + 2
    key = (cell[:, 2] * dim[1] + cell[:, 1]) * dim[0] + cell[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    for b in range(0, len(fin), chunk):
        e = min(len(fin), b + chunk)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                # the three cells of a row are adjacent keys
                k0 = key[b:e] + (dz * dim[1] + dy) * dim[0] - 1
                s = np.searchsorted(skey, k0, "left")
                t = np.searchsorted(skey, k0 + 2, "right")
                cnt = t - s
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                i = np.repeat(np.arange(b, e), cnt)
                first = np.repeat(s - (np.cumsum(cnt) - cnt), cnt)
                j = order[first + np.arange(tot)]
                yield fin[i], fin[j]


def moments(xyz, radius):
    """[n,10] int64: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of steps 1 and 2."""
    p = np.ascontiguousarray(xyz, F)
    n = len(p)
    r = F(radius)
    r2 = r * r
    scale = F(16384.0) / r
    out = np.zeros((n, 10), np.int64)
    for i, j in _pairs(p, radius):
        d = p[j] - p[i]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = d2 <= r2
        i = i[ok]
        q = np.rint(d[ok] * scale).astype(np.int64)
        cols = [np.ones(len(i), np.int64), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
                q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]]
        for c, w in enumerate(cols):           # bincount sums in double: exact, every partial sum is below 2^53
            out[:, c] += np.bincount(i, weights=w.astype(np.float64), minlength=n).astype(np.int64)
    return out


def _rotate(A, V, p, q, r):
    """One Jacobi rotation over every point at once; A: dict of the six elements by sorted index pair, V[k][c]."""
    key = lambda a, b: (a, b) if a < b else (b, a)
    app, aqq, apq = A[(p, p)], A[(q, q)], A[(p, q)]
    arp, arq = A[key(r, p)], A[key(r, q)]
    go = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        tt = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(theta < 0.0, -tt, tt)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        A[(p, p)] = np.where(go, app - h, app)
        A[(q, q)] = np.where(go, aqq + h, aqq)
        A[(p, q)] = np.where(go, 0.0, apq)
        A[key(r, p)] = np.where(go, c * arp - s * arq, arp)
        A[key(r, q)] = np.where(go, s * arp + c * arq, arq)
        for k in range(3):
            x, y = V[k][p], V[k][q]
            V[k][p] = np.where(go, c * x - s * y, x)
            V[k][q] = np.where(go, s * x + c * y, y)


def from_moments(m, xyz, viewpoint=(0, 0, 0), min_neighbours=MIN_NEIGHBOURS, orient=1, line_ratio=LINE_RATIO, sweeps=SWEEPS):
    """Steps 3 to 6 -> (normals [n,3] f32, curvature [n] f32, valid [n] bool)."""
    m = np.asarray(m, np.int64)
    p = np.ascontiguousarray(xyz, F)
    n = len(m)
    enough = m[:, 0] >= int(min_neighbours)
    with np.errstate(all="ignore"):
        dn = m[:, 0].astype(np.float64)
        mx, my, mz = m[:, 1].astype(np.float64) / dn, m[:, 2].astype(np.float64) / dn, m[:, 3].astype(np.float64) / dn
        A = {(0, 0): m[:, 4].astype(np.float64) / dn - mx * mx, (0, 1): m[:, 5].astype(np.float64) / dn - mx * my,
             (0, 2): m[:, 6].astype(np.float64) / dn - mx * mz, (1, 1): m[:, 7].astype(np.float64) / dn - my * my,
             (1, 2): m[:, 8].astype(np.float64) / dn - my * mz, (2, 2): m[:, 9].astype(np.float64) / dn - mz * mz}
        for k in A:
            A[k] = np.where(enough, A[k], 0.0)
        one, zero = np.ones(n), np.zeros(n)
        V = [[one.copy(), zero.copy(), zero.copy()], [zero.copy(), one.copy(), zero.copy()], [zero.copy(), zero.copy(), one.copy()]]
        for _ in range(int(sweeps)):
            _rotate(A, V, 0, 1, 2)
            _rotate(A, V, 0, 2, 1)
            _rotate(A, V, 1, 2, 0)
        a0, a1, a2 = A[(0, 0)], A[(1, 1)], A[(2, 2)]
        lo01, hi01 = np.where(a0 < a1, a0, a1), np.where(a0 < a1, a1, a0)
        lmin = np.where(lo01 < a2, lo01, a2)
        lmax = np.where(hi01 < a2, a2, hi01)
        h2 = np.where(hi01 < a2, hi01, a2)
        lmid = np.where(lo01 < h2, h2, lo01)
        valid = enough & (lmid > np.float64(F(line_ratio)) * lmax)
        c0 = (a0 <= a1) & (a0 <= a2)
        c1 = ~c0 & (a1 <= a2)
        pick = lambda k: np.where(c0, V[k][0], np.where(c1, V[k][1], V[k][2]))
        nx, ny, nz = pick(0), pick(1), pick(2)
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        if orient:
            v = np.asarray(viewpoint, F).astype(np.float64)
            pd = p.astype(np.float64)
            dot = (nx * (v[0] - pd[:, 0]) + ny * (v[1] - pd[:, 1])) + nz * (v[2] - pd[:, 2])
            flip = dot < 0.0
            nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
        ssum = (a0 + a1) + a2
        curv = np.where(ssum == 0.0, 0.0, lmin / ssum).astype(F)
        nrm = np.stack([nx, ny, nz], axis=1).astype(F)
    nrm[~valid] = 0
    curv[~valid] = 0
    return nrm, curv, valid


def estimate(xyz, radius, viewpoint=(0, 0, 0), **kw):
    return from_moments(moments(xyz, radius), xyz, viewpoint, **kw)


def mesh_normals(xyz, tri):
    """oslam_mesh_normals: (normals [nv,3] f32, valid [nv] bool); the triangles are added in order."""
    p = np.asarray(xyz, F).astype(np.float64)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(p)):
        raise ValueError("vertex index out of range")
    e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    acc = np.zeros_like(p)
    for k in range(len(t)):         # in order: np.add.at's order is not documented
        for c in range(3):
            acc[t[k, c]] += cr[k]
    with np.errstate(all="ignore"):
        ln = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        valid = (ln > 0.0) & np.isfinite(ln)
        nrm = (acc / ln[:, None]).astype(F)
    nrm[~valid] = 0
    return nrm, valid


def angle_deg(a, b, unsigned=False):
    """Angle between unit vectors row by row, degrees (unsigned: up to sign)."""
    d = np.einsum("ij,ij->i", np.asarray(a, np.float64), np.asarray(b, np.float64))
    if unsigned:
        d = np.abs(d)
    return np.degrees(np.arccos(np.clip(d, -1.0, 1.0)))


def median_spacing(xyz, sample=2000, seed=1):
    """Median distance to the nearest other point, from a seeded sample of the cloud."""
    p = np.asarray(xyz, np.float64)
    idx = np.random.default_rng(seed).choice(len(p), size=min(sample, len(p)), replace=False)
    best = np.full(len(idx), np.inf)
    for b in range(0, len(p), 1 << 14):
        d2 = ((p[idx, None, :] - p[None, b:b + (1 << 14), :]) ** 2).sum(axis=2)
        d2[d2 == 0.0] = np.inf
        best = np.minimum(best, d2.min(axis=1))
    return float(np.median(np.sqrt(best)))


def icosphere(subdivisions=2):
    """Unit icosphere, counter-clockwise seen from outside -> (points f32 [nv,3], triangles uint32 [nt,3])."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            k = (a, b) if a < b else (b, a)
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, F), np.array(f, np.uint32)


# ---------------------------------------------------------------- the end-to-end case of the host and device tests
E2E_CAM = dict(width=96, height=72, fx=100.0, fy=100.0, cx=47.5, cy=35.5)
E2E_TAU_D = 0.05
E2E_RADIUS_SPACINGS = 3.0


def grid_mesh(synth, k=0, nu=24, nv=16):
    """Surface k of synth as a (u, v)-grid mesh, counter-clockwise seen from outside -> (points f32, triangles uint32)."""
    u, v = np.meshgrid(np.linspace(0.0, 2 * np.pi, nu, endpoint=False), np.linspace(0.2, 2.9, nv), indexing="ij")
    p, _ = synth._surface(u.ravel(), v.ravel(), k)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)])
    return np.ascontiguousarray(p, F), np.ascontiguousarray(tri, np.uint32)


def e2e_case(synth, oracle, k=0, seed=11):
    """A model as a grid mesh and the single-view cloud of a rendered frame that contains it before a wall, points only
    -> dict(mp, tri, sp, radius, d_dist, diameter, truth)."""
    mp, tri = grid_mesh(synth, k)
    rng = synth.SplitMix64(seed)
    T = np.eye(4)
    T[:3, :3] = synth.random_rotation(rng)
    T[:3, 3] = (0.3, -0.2, 8.0)
    dense, _ = synth.make_model(k, 200000)
    obj = dense.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    gx, gy = np.meshgrid(np.arange(-8.0, 8.0, 0.02), np.arange(-6.0, 6.0, 0.02))
    wall = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 12.0)], axis=1)
    img = synth.render_depth(np.concatenate([obj, wall]), splat=1, **E2E_CAM)
    cam = {q: E2E_CAM[q] for q in ("fx", "fy", "cx", "cy")}
    sp, _ = oracle.depth_to_cloud(img, depth_scale=0.001, z_min=0.1, z_max=20.0, max_jump=0.5, **cam)
    diameter = synth.bbox_extent(mp)
    return dict(mp=mp, tri=tri, sp=sp, radius=E2E_RADIUS_SPACINGS * median_spacing(sp), d_dist=synth.d_dist_for(mp, E2E_TAU_D),
                diameter=diameter, truth=T)


def accepted(oracle, T, case):
    """The reference's acceptance test (alignment.cpp:141-144): translation below 0.1 diameters, rotation below 12 degrees."""
    dt, dr = oracle.ht_dist(np.asarray(T, F), case["truth"].astype(F))
    return dt < 0.1 * case["diameter"] and dr < np.radians(12.0), dt, dr


# ---------------------------------------------------------------- inputs the host and the device tests share
def lattice(nx=9, ny=9, z=1.0, step=0.25):
    gx, gy = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], axis=1).astype(F)


def degenerate_cloud():
    """One cloud with every degenerate input at least 100 radii from the next; radius 0.5 -> (points, expectations)"""
    parts, at = {}, 0
    cloud = []

    def add(name, pts):
        nonlocal at
        parts[name] = slice(at, at + len(pts))
        cloud.append(np.asarray(pts, F))
        at += len(pts)
    add("plane", lattice(7, 7, 0.0))                                                   # z = 0: the tangent viewpoint's
    add("few", [[100.0, 0, 0], [100.25, 0, 0], [100.0, 0.25, 0], [100.25, 0.25, 0]])   # 4 < min_neighbours
    add("coincident", [[200.0, 1.0, 2.0]] * 6)
    add("collinear", [[300.0 + 0.25 * k, 0, 0] for k in range(9)])
    add("nonfinite", [[np.nan, 0, 0], [0.5, np.inf, 0.0], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan]])
    return np.concatenate(cloud), parts


def write_ply_plain(path, points, triangles=None):
    """A binary PLY with x y z only (no normals), and a face element when triangles are given."""
    p = np.ascontiguousarray(points, "<f4")
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(p)
    if triangles is not None:
        head += "element face %d\nproperty list uchar int vertex_indices\n" % len(triangles)
    with open(path, "wb") as f:
        f.write((head + "end_header\n").encode())
        f.write(p.tobytes())
        if triangles is not None:
            rec = np.zeros(len(triangles), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
            rec["n"], rec["i"] = 3, np.asarray(triangles)
            f.write(rec.tobytes())
