"""Deterministic inputs at the edges of the refinement stage (oslam_refine.hip, oslam_refine.c): scene grids whose scan
sits on the borders of k_scan_local and k_scan_top and on the cell limit, a lattice of exact ties that span grid cells,
queries on and one ulp beyond the closed ball and one or two cells outside every face of the box, and a database of
members around the wave and workgroup sizes with skipped, stopped, converged and far members among them.

tests/test_refine_edge_inputs.py asserts on the restatement alone (refine_ref) that the inputs reach the paths they are
named for; tests/test_gpu_refine_edges.py compares the device with the same restatement.  numpy only; seeded
(synth.SplitMix64)."""
import functools

import numpy as np

import edge_inputs
import fusion_edge_inputs
import refine_ref as R

F = np.float32
GATES = (0.8, -2.0)

# ---------------------------------------------------------------- scene grids
GRID_POINTS = 4096
BOX_RADIUS = 0.01
# name -> (dims of the box at BOX_RADIUS, radius of the call, then what the grid of the call must be: dims, n_cells, nb,
# per, clamped).  n_cells + 1 items are scanned: 4096 items fill one workgroup of k_scan_local, 1024 workgroups give
# every thread of k_scan_top one block total, 1025 give it two, and the cell limit gives it four.
GRID_CASES = {
    "1x1x1": ((1, 1, 1), 0.01, (1, 1, 1), 1, 1, 1, False),
    "13x15x21": ((13, 15, 21), 0.01, (13, 15, 21), 4095, 1, 1, False),
    "16x16x16": ((16, 16, 16), 0.01, (16, 16, 16), 4096, 2, 1, False),
    "4097x1x1": ((4097, 1, 1), 0.01, (4097, 1, 1), 4097, 2, 1, False),
    "69x89x683": ((69, 89, 683), 0.01, (69, 89, 683), 4194303, 1024, 1, False),
    "128x128x256": ((128, 128, 256), 0.01, (128, 128, 256), 4194304, 1025, 2, False),
    "128x128x256 r 0.002": ((128, 128, 256), 0.002, (201, 201, 403), 16281603, 3976, 4, True),
}
GRID_BLOCKS = (0, 1, 127, 128, 511, 512, 513)          # and the last: their first and last cells are occupied
GRID_SHIFT = (0.2, -0.2, 0.1)                          # times the radius: a translation of 0.3 radius


def grid_blocks(shape):
    """[(first cell, last cell)] of every workgroup of k_scan_local that holds a cell (the last item is the end mark)"""
    return [(b * R.SCAN_ITEMS, min((b + 1) * R.SCAN_ITEMS, shape["n_cells"]) - 1) for b in range(shape["nb"])
            if b * R.SCAN_ITEMS < shape["n_cells"]]


def grid_case(synth, name):
    """A scene of GRID_POINTS points with unit random normals: the eight corners of the box pin the dims, every other
    point lies on the centre of a cell of the call's grid (on the middle of what the box leaves of a last cell).  Every
    block of 4096 cells holds a point; the first and last cells of GRID_BLOCKS and of the last block hold one.  The model
    is the scene's own cloud.  -> dict(sp, sn, radius, d, shape, want, blocks, poses)"""
    box, radius, dims, n_cells, nb, per, clamped = GRID_CASES[name]
    rng = synth.SplitMix64(9100 + sum(ord(ch) for ch in name))
    e_box = float(F(BOX_RADIUS)) * (1.0 + 1e-4)
    top = np.array([(n - 0.5) * e_box for n in box])
    corners = np.array([[(k >> a & 1) * top[a] for a in range(3)] for k in range(8)]).astype(np.float32)
    shape = R.grid_shape(corners, radius)
    hi = corners.max(axis=0).astype(np.float64)
    blocks = grid_blocks(shape)
    cells = []
    for b in sorted(set(k for k in GRID_BLOCKS if k < len(blocks)) | {len(blocks) - 1}):
        cells += list(blocks[b])
    u = rng.uniform(len(blocks))
    cells += [first + int(x * (last - first + 1)) for (first, last), x in zip(blocks, u)]
    n_rest = GRID_POINTS - 8 - len(cells)
    assert n_rest >= 0
    if shape["n_cells"] >= n_rest:                                     # distinct cells where there are enough
        rest = np.argsort(rng.u64(shape["n_cells"]), kind="stable")[:n_rest] if shape["n_cells"] <= 1 << 16 else \
            (rng.uniform(n_rest) * shape["n_cells"]).astype(np.int64)
    else:
        rest = np.arange(n_rest) % shape["n_cells"]
    cells = np.array(cells + [int(x) for x in rest], np.int64)
    dx, dy = shape["dims"][0], shape["dims"][1]
    k3 = np.stack([cells % dx, (cells // dx) % dy, cells // (dx * dy)], axis=1).astype(np.float64)
    centre = (k3 + 0.5) * shape["edge"]
    pts = np.where(centre <= hi, centre, 0.5 * (k3 * shape["edge"] + hi))
    pts = np.concatenate([corners.astype(np.float64), pts])
    nrm = rng.normal(3 * GRID_POINTS).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    order = np.argsort(rng.u64(GRID_POINTS), kind="stable")            # index order is not cell order
    sp = np.ascontiguousarray(pts[order], np.float32)
    sn = np.ascontiguousarray(nrm[order], np.float32)
    r = float(F(radius))
    poses = {"identity": edge_inputs.rigid(), "shift": edge_inputs.rigid(t=[r * s for s in GRID_SHIFT])}
    return dict(name=name, sp=sp, sn=sn, radius=radius, d=synth.d_dist_for(sp, 0.05), shape=R.grid_shape(sp, radius),
                want=dict(dims=dims, n_cells=n_cells, nb=nb, per=per, clamped=clamped), blocks=blocks, poses=poses)


CLAMPED = "128x128x256 r 0.002"


def clamped_call(case):
    """(keywords of the refine parameters, the radius they give) with which oslam_refine asks for the clamped grid of the
    case CLAMPED: max_corr_dist * d_dist in float32 is its radius to a rounding"""
    mcd = F(case["radius"] / case["d"])
    return dict(max_corr_dist=float(mcd), inlier_dist=float(F(0.5) * mcd), max_iterations=1), float(mcd * F(case["d"]))


# ---------------------------------------------------------------- the grid cache
CACHE_RADII = (0.4, 1.0, 2.2, 5.0, 11.0, 0.4)         # times d_dist on the members' scene: five grids for GRID_SLOTS = 4


# ---------------------------------------------------------------- the tie lattice
H = 2.0 ** -4                   # the lattice step and the radius: every coordinate and distance below is exact in float
LATTICE_N = 9
N_DUPLICATES = 60
TIE_SHIFT = (2.0 ** -4, -2.0 ** -3, 2.0 ** -5)        # one cell, two cells, half a cell: cell centres become face centres


def tie_scene(synth):
    """The 9^3 points at multiples of H with normals +z and N_DUPLICATES copies of seeded lattice points, every third
    copy with a normal that fails the gate 0.8 against +z; all in one seeded shuffled order, so that a copy can carry a
    lower index than its original.  -> (sp, sn, is_copy bool [n])"""
    rng = synth.SplitMix64(9200)
    g = np.arange(LATTICE_N, dtype=np.float64) * H
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    lat = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    pick = (rng.uniform(N_DUPLICATES) * len(lat)).astype(np.int64)
    nrm = np.tile([[0.0, 0.0, 1.0]], (len(lat) + N_DUPLICATES, 1))
    nrm[len(lat)::3] = [0.8, 0.0, 0.6]                                 # dot 0.6 with +z
    pts = np.concatenate([lat, lat[pick]])
    copy = np.arange(len(pts)) >= len(lat)
    order = np.argsort(rng.u64(len(pts)), kind="stable")
    return np.ascontiguousarray(pts[order], np.float32), np.ascontiguousarray(nrm[order], np.float32), copy[order]


def tie_queries():
    """(points float32 [n, 3] with normals +z, kind int [n]: 8 = the 512 cell centres (8 tied corners), 4 = the face
    centres, 2 = the edge midpoints)"""
    out, kind = [], []
    n = LATTICE_N - 1
    for half in ((1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        ax = [np.arange(n) + 0.5 if h else np.arange(n + 1.0) for h in half]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        out.append(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) * H)
        kind += [2 ** sum(half)] * x.size
    q = np.ascontiguousarray(np.concatenate(out), np.float32)
    return q, np.tile(F([0.0, 0.0, 1.0]), (len(q), 1)), np.array(kind)


def tie_poses():
    return {"identity": edge_inputs.rigid(), "shift": edge_inputs.rigid(t=TIE_SHIFT)}


# ---------------------------------------------------------------- queries off the faces and corners of the lattice's box
FACE_OFFSETS = ("0.5 r", "r", "r + ulp", "1.5 r", "2.5 r")
FACE_POSES = {"identity": (0.0, 0.0, 0.0), "x 1e30": (1e30, 0.0, 0.0), "y -1e30": (0.0, -1e30, 0.0), "z 3e38": (0.0, 0.0, 3e38),
              "xyz 3e38": (3e38, -3e38, 3e38)}


def _beyond(face, sign, name):
    """the float32 coordinate at an offset outside the face at coordinate `face` (sign -1: below it)"""
    r = F(H)
    if name == "r + ulp":                 # one ulp of the coordinate itself: the difference to the face exceeds r
        x = F(face) + F(sign) * r
        return np.nextafter(x, F(sign) * F(np.inf))
    return F(face) + F(sign) * F({"0.5 r": 0.5, "r": 1.0, "1.5 r": 1.5, "2.5 r": 2.5}[name]) * r


def face_queries():
    """Off each of the six faces of the box [0, 8 H]^3: a query straight out of the lattice points (3 H, 5 H), (0, 0) and
    (8 H, 8 H) of the face, at every offset of FACE_OFFSETS; the nearest scene point is the face point, at exactly the
    offset.  Off each of the eight corners: the same offsets along all three axes at once.  -> (points, normals +z,
    labels [(what, offset name)])"""
    top = (LATTICE_N - 1) * H
    out, labels = [], []
    for a in range(3):
        for sign, face in ((-1, 0.0), (1, top)):
            for u, v in ((3 * H, 5 * H), (0.0, 0.0), (top, top)):
                for name in FACE_OFFSETS:
                    p = [0.0, 0.0, 0.0]
                    p[a], p[(a + 1) % 3], p[(a + 2) % 3] = _beyond(face, sign, name), u, v
                    out.append(p)
                    labels.append(("face %s%s" % ("-+"[sign > 0], "xyz"[a]), name))
    for k in range(8):
        for name in FACE_OFFSETS:
            out.append([_beyond(top if k >> a & 1 else 0.0, 1 if k >> a & 1 else -1, name) for a in range(3)])
            labels.append(("corner %d" % k, name))
    q = np.ascontiguousarray(out, np.float32)
    return q, np.tile(F([0.0, 0.0, 1.0]), (len(q), 1)), labels


def face_poses():
    return {k: edge_inputs.rigid(t=t) for k, t in FACE_POSES.items()}


# ---------------------------------------------------------------- members of one database call
MEMBER_SIZES = edge_inputs.MODEL_SIZES[1:]             # 2 .. 1025: prefixes of one synth model
MEMBER_SCENE = (5000, 77)                              # points of the scene that holds the model, and its seed
# (points, kind) in database order.  "near": the truth perturbed by about 3 degrees and 0.5 d_dist (every third of them by
# two and every fourth by three times that: they take the most iterations); "zero": an all-zero pose, skipped; "truth":
# the exact ground truth; "far": the truth moved 40 units away.
MEMBERS = [(2, "near"), (5, "near"), (6, "near"), (300, "zero"), (7, "near"), (63, "near"), (64, "near"), (65, "near"),
           (255, "near"), (256, "near"), (64, "zero"), (257, "near"), (511, "near"), (512, "near"), (513, "truth"),
           (513, "near"), (257, "far"), (1025, "near")]
assert [n for n, k in MEMBERS if k == "near"] == MEMBER_SIZES
MEMBER_SCHEDULES = (30, 1, 4, 5)                       # max_iterations: the default, one step, either side of CHECK_EVERY (4)

# Up to this condition number of J^T J of the first step the device's pose is held to the bits of refine(sums="f32").  It is
# fusion_edge_inputs.COND_STREAM_640, chosen there as the largest cond of a stream whose poses an existing test already holds
# to the bits; the step it bounds is the same code (oslam_refine_step.h) against a restatement that differs from it in no
# more (here in less: step_pinned repeats the device's factorisation, there numpy's is used).  Above it the pose is held to
# max(0.01 degrees, 8 x spread) only; the integer fields, fitness and rmse are held bit for bit everywhere.  On an MI355X
# every member of BITS_HELD held the bits at all four MEMBER_SCHEDULES (tests/test_gpu_refine_edges.py asserts it).
COND_BITS = fusion_edge_inputs.COND_STREAM_640
# the members (index into MEMBERS) that step and whose cond lies below COND_BITS; tests/test_refine_edge_inputs.py
# recomputes the list
BITS_HELD = (2, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 17)


def member_case(synth):
    """The scene holds the model's own 1025 points under the ground truth (so that the truth is a fixed point of the
    step and a member there converges at once) among the clutter, the plane and the other object of a synth scene, in a
    seeded shuffled order.  -> dict(mp, mn: the 1025-point model, d, sp, sn, truth, T_in float32 [n, 4, 4])"""
    mp, mn = synth.make_model(0, max(MEMBER_SIZES))
    d = synth.d_dist_for(mp, 0.05)
    rng = synth.SplitMix64(9300)
    truth = np.eye(4)
    truth[:3, :3] = synth.random_rotation(rng)
    truth[:3, 3] = [1.5, -2.0, 3.0]
    cp, cn, _ = synth.make_scene([3], MEMBER_SCENE[0] - len(mp), MEMBER_SCENE[1], instance_points=600)
    tp, tn = synth.transform_cloud(mp, mn, truth)
    order = np.argsort(rng.u64(MEMBER_SCENE[0]), kind="stable")
    sp = np.ascontiguousarray(np.concatenate([tp, cp])[order])
    sn = np.ascontiguousarray(np.concatenate([tn, cn])[order])
    T_in = np.zeros((len(MEMBERS), 4, 4), np.float32)
    for j, (n, kind) in enumerate(MEMBERS):
        u = rng.uniform(6) * 2 - 1
        if kind == "zero":
            continue
        T = truth.copy()
        if kind == "near":
            far = 3.0 if j % 4 == 0 else 2.0 if j % 3 == 0 else 1.0
            D = np.eye(4)
            D[:3, :3] = R.rodrigues(np.radians(3.0 * far) * u[:3] / np.linalg.norm(u[:3]))[0]
            c = truth[:3, :3] @ mp[:n].astype(np.float64).mean(axis=0) + truth[:3, 3]
            D[:3, 3] = c - D[:3, :3] @ c + 0.5 * far * d * u[3:] / np.linalg.norm(u[3:])  # turned about the member's centre
            T = D @ truth
        elif kind == "far":
            T[:3, 3] += [40.0, 0.0, 0.0]
        T_in[j] = T.astype(np.float32)
    return dict(mp=mp, mn=mn, d=d, sp=sp, sn=sn, truth=truth, T_in=T_in)


@functools.lru_cache(maxsize=None)
def member_answers(synth, max_iterations=30, sums="f64"):
    """[(T float32 4x4, info)] of refine_ref.refine for every member, None for the skipped ones; computed once"""
    c = member_case(synth)
    out = []
    for j, (n, kind) in enumerate(MEMBERS):
        out.append(None if kind == "zero" else
                   R.refine(c["mp"][:n], c["mn"][:n], c["sp"], c["sn"], c["T_in"][j], c["d"], sums=sums, max_iterations=max_iterations))
    return out
