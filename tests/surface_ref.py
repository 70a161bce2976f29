"""Numpy restatement of the surface extraction (include/oslam.h at oslam_volume_surface): the yardstick of the device
path, and the builders of the volumes both test files load.

float32 with the header's operation order, vectorised over the crossings, so points, normals, their order and the two
counts equal the device's bit for bit.  The trilinear read is volume_ref.Volume._trilinear, the ray cast's.  numpy only.
"""
import numpy as np

import volume_ref as V

F = np.float32
AXES = "xyz"


def _edges(vol, a, min_weight):
    """Axis a: (seen0, seen1, q0, q1, w0, w1) over the legal edges, each shaped like the volume minus one along a."""
    ax = 2 - a                                                  # the arrays are [nz, ny, nx]
    lo = tuple(slice(None, -1) if d == ax else slice(None) for d in range(3))
    hi = tuple(slice(1, None) if d == ax else slice(None) for d in range(3))
    return (vol.w[lo] >= min_weight, vol.w[hi] >= min_weight, vol.q[lo], vol.q[hi], vol.w[lo], vol.w[hi])


def surface(vol, min_weight=1, trace=None):
    """-> (xyz float32 [n, 3], nrm float32 [n, 3], crossings).  vol: a volume_ref.Volume.
    trace: a dict that receives counts of the inputs that reached each branch (added to what it holds); see the keys
    below.  The result does not depend on it."""
    nx, ny, nz = vol.n
    tr = {}
    keys, idx, q0s, q1s = [], [], [], []
    for a in range(3):
        s0, s1, q0, q1, w0, w1 = _edges(vol, a, min_weight)
        change = (q0 < 0) != (q1 < 0)
        cross = s0 & s1 & change
        k, j, i = np.nonzero(cross)
        keys.append(3 * (i + nx * (j + ny * k)) + a)
        idx.append(np.stack([i, j, k], axis=1))
        q0s.append(q0[cross])
        q1s.append(q1[cross])
        if trace is not None:
            both = s0 & s1
            ax = AXES[a]
            for name, m in (("zero_negative", cross & ((q0 == 0) | (q1 == 0))),
                            ("zero_positive", both & ~change & ((q0 == 0) | (q1 == 0))),
                            ("q_max", cross & ((q0 == 32767) | (q1 == 32767))),
                            ("q_min", cross & ((q0 == -32767) | (q1 == -32767))),
                            ("sign_change_unseen", change & ~both),
                            ("w_below_min_0", change & (w0 == min_weight - 1)), ("w_below_min_1", change & (w1 == min_weight - 1)),
                            ("w_at_min_0", cross & (w0 == min_weight)), ("w_at_min_1", cross & (w1 == min_weight)),
                            ("w_65535_0", cross & (w0 == 65535)), ("w_65535_1", cross & (w1 == 65535))):
                tr[name] = tr.get(name, 0) + int(m.sum())
            tr["last_edge_" + ax] = int((idx[-1][:, a] == vol.n[a] - 2).sum())
            # what a read at +stride would see from the voxels that have no edge on this axis (modulo the volume)
            lin = np.arange(nx * ny * nz).reshape(nz, ny, nx)
            last = tuple(slice(-1, None) if d == 2 - a else slice(None) for d in range(3))
            src = lin[last].ravel()
            dst = (src + (1, nx, nx * ny)[a]) % (nx * ny * nz)
            qf, wf = vol.q.ravel(), vol.w.ravel()
            tr["wrap_" + ax] = int(((wf[src] >= min_weight) & (wf[dst] >= min_weight) & ((qf[src] < 0) != (qf[dst] < 0))).sum())
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    assert np.all(np.diff(key[order]) > 0)
    ijk = np.concatenate(idx)[order]
    axis = (key[order] % 3).astype(np.int64)
    q0, q1 = np.concatenate(q0s)[order], np.concatenate(q1s)[order]
    n = len(key)
    with np.errstate(all="ignore"):
        F0, F1 = q0.astype(np.float32) / F(32767.0), q1.astype(np.float32) / F(32767.0)
        t = F0 / (F0 - F1)
        P = [vol.origin[b] + (ijk[:, b].astype(np.float32) + F(0.5)) * vol.voxel for b in range(3)]
        for a in range(3):
            P[a] = np.where(axis == a, P[a] + t * vol.voxel, P[a])
        g, ok = [], np.ones(n, bool)
        low, high, unseen = np.zeros((3, n), bool), np.zeros((3, n), bool), np.zeros(n, bool)
        for b in range(3):
            hi_p = [P[c] + vol.voxel if c == b else P[c] for c in range(3)]
            lo_p = [P[c] - vol.voxel if c == b else P[c] for c in range(3)]
            v1, ok1 = vol._trilinear(*hi_p)
            v0, ok0 = vol._trilinear(*lo_p)
            ok &= ok1 & ok0
            g.append(v1 - v0)
            if trace is not None:
                for p, okp in ((hi_p, ok1), (lo_p, ok0)):
                    inside = np.ones(n, bool)
                    for c in range(3):
                        base = np.floor((p[c] - vol.origin[c]) * vol.inv_voxel - F(0.5))
                        low[c] |= base < F(0)
                        high[c] |= base > F(vol.n[c] - 2)
                        inside &= (base >= F(0)) & (base <= F(vol.n[c] - 2))
                    unseen |= inside & ~okp
        ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(np.float32)
        has = ok & (ln > F(0)) & (ln <= F(3.0e38))
        nrm = np.stack([g[b] / ln for b in range(3)], axis=1).astype(np.float32)
    xyz = np.stack(P, axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    assert xyz.dtype == np.float32 and nrm.dtype == np.float32 and t.dtype == np.float32
    if trace is not None:
        tr.update(crossings=n, points=int(has.sum()), drop_unseen_corner=int(unseen.sum()), drop_len_zero=int((ok & (ln == F(0))).sum()))
        for c in range(3):
            tr["drop_low_" + AXES[c]] = int(low[c].sum())
            tr["drop_high_" + AXES[c]] = int(high[c].sum())
        for name, val in tr.items():
            trace[name] = trace.get(name, 0) + val
    return np.ascontiguousarray(xyz[has]), np.ascontiguousarray(nrm[has].reshape(-1, 3)), n


# ---------------------------------------------------------------- volumes written directly
def blank(nx, ny, nz, voxel=0.05, origin=(0.0, 0.0, 0.0), **kw):
    return V.Volume(nx, ny, nz, voxel, list(origin), **kw)


def put(vol, i, j, k, q, w):
    vol.q[k, j, i], vol.w[k, j, i] = q, w


def checkerboard(nx=16, ny=16, nz=16):
    """Signs that alternate with i + j + k, every voxel seen: every legal edge is a crossing (3 * 16 * 16 * 15 = 11 520
    at 16^3), each at its edge's midpoint, where the six reads are midpoints of edges too, 0.5 * 1 + 0.5 * -1 = 0.  Where
    the float32 coordinates make the fractions exactly 0.5 the gradient vanishes (len == 0); elsewhere it is rounding
    noise of some 1e-7, which still has a direction: the normals there test every rounding of the read."""
    vol = blank(nx, ny, nz)
    k, j, i = np.indices((nz, ny, nx))
    vol.q[:] = np.where((i + j + k) % 2 == 0, 8000, -8000)
    vol.w[:] = 1
    return vol


def single_crossings(nx=16, ny=16, nz=16):
    """One volume per axis whose only seen voxels are the two ends of one edge, the last legal one of that axis (from
    n_a - 2 to n_a - 1): one crossing, and no normal for it."""
    out = []
    for a in range(3):
        vol = blank(nx, ny, nz)
        at = [5, 6, 7]
        at[a] = vol.n[a] - 2
        put(vol, at[0], at[1], at[2], 3000, 2)
        at[a] = vol.n[a] - 1
        put(vol, at[0], at[1], at[2], -1000, 2)
        out.append(vol)
    return out


def wrap_bait(nx=16, ny=16, nz=16):
    """Three pairs of seen voxels of opposite sign in an unseen volume, each pair one wrapping read apart and no legal
    edge apart: the last voxel of a row and the first of the next (+1), the last row of a slab and the first of the next
    slab (+nx), the last slab and, modulo the volume, the first (+nx*ny).  No crossing."""
    vol = blank(nx, ny, nz)
    put(vol, nx - 1, 3, 3, -500, 9)
    put(vol, 0, 4, 3, 500, 9)
    put(vol, 5, ny - 1, 6, -500, 9)
    put(vol, 5, 0, 7, 500, 9)
    put(vol, 9, 9, nz - 1, -500, 9)
    put(vol, 9, 9, 0, 500, 9)
    return vol


def edge_inputs(nx=16, ny=16, nz=16, min_weight=1):
    """A seen, positive volume with the inputs of the issue's list placed apart from each other (see the trace keys of
    surface())."""
    vol = blank(nx, ny, nz)
    vol.q[:] = 2000
    vol.w[:] = 10 + min_weight
    lo, hi = min_weight - 1, min_weight
    put(vol, 4, 4, 4, 0, 20)                       # q0 == 0 with a negative neighbour on +x, positive ones elsewhere
    put(vol, 5, 4, 4, -500, 20)
    put(vol, 4, 9, 4, 0, 20)                       # q == 0 among positive voxels: no crossing
    put(vol, 9, 4, 4, -32767, 20)                  # q = -32767 next to q = +32767
    put(vol, 10, 4, 4, 32767, 20)
    put(vol, 4, 4, 9, -500, lo)                    # w = min_weight - 1: not seen, on either end of its six edges
    put(vol, 9, 4, 9, -500, hi)                    # w = min_weight: seen
    put(vol, 9, 9, 9, -500, 65535)
    put(vol, 12, 12, 4, -500, 0)                   # never seen, next to a negative voxel: the normals there lack a corner
    put(vol, 12, 11, 4, -500, 20)
    put(vol, nx - 1, 4, 12, -500, 20)              # crossings in the last legal edge of each axis ...
    put(vol, 4, ny - 1, 12, -500, 20)
    put(vol, 9, 9, nz - 1, -500, 20)
    put(vol, 0, 9, 12, -500, 20)                   # ... and in the first: the reads leave the volume at the low faces
    put(vol, 12, 0, 12, -500, 20)
    put(vol, 12, 12, 0, -500, 20)
    put(vol, nx - 1, 13, 13, -500, 20)             # wrap bait inside a seen volume: (0, 14, 13) is positive
    return vol


def sparse_random(nx, ny, nz, seed, share=0.04):
    """Seeded blobs of seen voxels with random signs and weights in an unseen volume: most runs of 1024 voxels are
    empty, the others hold varying numbers of crossings."""
    rng = np.random.default_rng(seed)
    vol = blank(nx, ny, nz)
    seen = np.zeros((nz, ny, nx), bool)
    for _ in range(max(1, int(share * nx * ny * nz / 125))):
        c = [int(rng.integers(0, n)) for n in (nz, ny, nx)]
        seen[max(0, c[0] - 2):c[0] + 3, max(0, c[1] - 2):c[1] + 3, max(0, c[2] - 2):c[2] + 3] = True
    vol.q[seen] = rng.integers(-32767, 32768, int(seen.sum())).astype(np.int16)
    vol.w[seen] = rng.integers(1, 6, int(seen.sum())).astype(np.uint16)
    return vol


# ---------------------------------------------------------------- a scanned object: four views around a synth model
OBJECT = dict(nx=64, ny=64, nz=64, voxel=0.02, origin=[-0.64, -0.64, 1.36], mu=0.08, max_weight=128)
OBJECT_SIZE = dict(width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5)      # a pixel is 3.8 mm at 2 m: 0.19 voxels
OBJECT_CAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.1, z_max=10.0)
OBJECT_SCALE = 0.3


def object_views(synth, k=0, seed=41):
    """Synth model k at OBJECT_SCALE in the middle of the OBJECT volume, 2 m before the first camera, and four cameras a
    quarter turn apart on a circle around it.  -> dict: T_obj (model -> volume frame, float32 4x4), poses (T_vol_cam,
    float32 4x4 each), imgs (uint16 640 x 480 depth frames, invalid where the object is not).
    The synth surface is an open sheet without thickness (a slit along u = 0, openings at the poles), and a TSDF holds
    solids: where a sheet is seen from both sides the two views' distances cancel.  So the frames show the solid that the
    model's outward normals describe: points whose normal faces away from the camera are not drawn (back-face culling),
    and no camera sees the sheet's inner side, which the model cloud does not have either."""
    dense, dense_n = synth.make_model(k, 300000)
    T_obj = np.eye(4)
    T_obj[:3, :3] = synth.random_rotation(synth.SplitMix64(seed))
    centre = np.array([0.0, 0.0, 2.0])
    T_obj[:3, 3] = centre
    world = OBJECT_SCALE * dense.astype(np.float64) @ T_obj[:3, :3].T + centre
    world_n = dense_n.astype(np.float64) @ T_obj[:3, :3].T
    poses, imgs = [], []
    for quarter in range(4):
        a = 0.5 * np.pi * quarter
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, centre - R @ centre
        Tc = np.linalg.inv(T)
        p, n = world @ Tc[:3, :3].T + Tc[:3, 3], world_n @ Tc[:3, :3].T
        poses.append(T.astype(np.float32))
        imgs.append(synth.render_depth(p[(n * p).sum(axis=1) < 0], background_z=None, splat=1, **OBJECT_SIZE))
    return dict(T_obj=T_obj.astype(np.float32), poses=poses, imgs=imgs)


def coverage(model_pts, T_obj, xyz, radius):
    """The share of the model's points (placed by T_obj) that have a point of the cloud xyz within radius."""
    p = model_pts.astype(np.float64) @ np.asarray(T_obj, np.float64)[:3, :3].T + np.asarray(T_obj, np.float64)[:3, 3]
    near = np.zeros(len(p), bool)
    s = xyz.astype(np.float64)
    for lo in range(0, len(p), 256):
        d2 = ((p[lo:lo + 256, None, :] - s[None, :, :]) ** 2).sum(axis=2)
        near[lo:lo + 256] = d2.min(axis=1) <= radius * radius
    return float(near.mean())
