"""Numpy restatement of the tracking stage and the tracker (include/oslam.h at oslam_track and oslam_tracker_step): the
yardstick of the device path.

The vertex and normal maps, the projection, the gates and the classes are computed in float32 with the header's
operation order, so maps, correspondences and the judgement equal the device's bit for bit.  The step sums in float64
(the device sums in float per block of 256 model points, then in double), so poses agree to rounding, not to the bit.
numpy only: it runs wherever the tests do.
"""
import math

import numpy as np

import arbitrate_ref
import instances_ref
import refine_ref
import view_ref

F = np.float32
MAX_HYPOTHESES = 1024


def default_params():
    """oslam_track_params_default; verify: the defaults of view_ref."""
    return dict(max_iterations=10, max_corr_dist=2.0, min_normal_dot=0.8, stop_rot=1e-5, stop_trans=1e-4,
                verify=view_ref.default_params())


def default_tracker_params():
    return dict(max_misses=2, detect_every=10, assoc_min_separation=0.5, assoc_max_angle=math.pi)


# ---------------------------------------------------------------- part 1: the maps of a view
def view_maps(depth, cam, max_jump):
    """(vertex [h,w,3], normal [h,w,3], has bool [h,w]) of a depth image: per pixel what oslam_depth_to_cloud produces
    (oracle/oracle_depth.c), zeros where the pixel has no normal.  cam: dict(fx, fy, cx, cy, depth_scale, z_min, z_max)."""
    z = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    h, w = z.shape
    fx, fy, cx, cy, mj = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"]), F(max_jump)
    u = np.arange(w, dtype=np.float32)[None, :]
    v = np.arange(h, dtype=np.float32)[:, None]
    with np.errstate(all="ignore"):
        P = np.stack([((u - cx) * z) / fx, ((v - cy) * z) / fy, z], axis=2).astype(np.float32)
        ok = np.zeros((h, w), bool)
        c = z[1:-1, 1:-1]
        zl, zr, zu, zd = z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
        ok[1:-1, 1:-1] = ((c > 0) & (zl > 0) & (zr > 0) & (zu > 0) & (zd > 0) & (np.abs(zl - c) <= mj) & (np.abs(zr - c) <= mj) &
                          (np.abs(zu - c) <= mj) & (np.abs(zd - c) <= mj))
        A = np.zeros((h, w, 3), np.float32)
        B = np.zeros((h, w, 3), np.float32)
        A[1:-1, 1:-1] = P[1:-1, 2:] - P[1:-1, :-2]
        B[1:-1, 1:-1] = P[2:, 1:-1] - P[:-2, 1:-1]
        nx = A[..., 1] * B[..., 2] - A[..., 2] * B[..., 1]
        ny = A[..., 2] * B[..., 0] - A[..., 0] * B[..., 2]
        nz = A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz).astype(np.float32)
        ok &= (ln > 0) & (ln <= F(3.0e38))
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        flip = ((nx * P[..., 0] + ny * P[..., 1]) + nz * P[..., 2]) > 0
    N = np.stack([np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)], axis=2).astype(np.float32)
    N[~ok] = 0
    V = P.copy()
    V[~ok] = 0
    return V, N, ok


def cloud_of_maps(V, N, ok):
    """The maps' pixels that have a normal in row-major order: what oslam_depth_to_cloud returns."""
    return V[ok], N[ok]


# ---------------------------------------------------------------- part 2: correspondences, the step, the judgement
def correspondences(mp, mn, T, maps, cam, radius, min_dot):
    """-> (pixel int32 [M]: v * w + u, -1 none; q, m: the transformed points and normals)."""
    V, N, ok = maps
    h, w = ok.shape
    q, m = refine_ref.transform_f32(T, mp, mn)
    dot = (m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2]
    pz = q[:, 2]
    with np.errstate(all="ignore"):
        fu = np.floor(((q[:, 0] * F(cam["fx"])) / pz + F(cam["cx"])) + F(0.5))
        fv = np.floor(((q[:, 1] * F(cam["fy"])) / pz + F(cam["cy"])) + F(0.5))
        inside = (~(dot >= F(0))) & (pz >= F(cam["z_min"])) & (pz <= F(cam["z_max"])) & (fu >= F(0)) & (fu < F(w)) & \
            (fv >= F(0)) & (fv < F(h))
    u = np.where(inside, fu, 0).astype(np.int64)
    v = np.where(inside, fv, 0).astype(np.int64)
    a, b = V[v, u], N[v, u]
    r = F(radius)
    d = a - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    nd = (m[:, 0] * b[:, 0] + m[:, 1] * b[:, 1]) + m[:, 2] * b[:, 2]
    good = inside & ok[v, u] & (d2 <= r * r) & (nd >= F(min_dot))
    return np.where(good, v * w + u, -1).astype(np.int32), q, m


def track(mp, mn, T_prev, depth, cam, d_dist, max_jump, maps=None, sums="f64", **kw):
    """One hypothesis followed into the image -> (T_out float32 4x4, dict verify iterations correspondences converged
    found, cond: the condition number of the last damped 6x6 system).  The loop is refine_ref.refine's with the
    correspondences above.  sums: the precision and order of the step's sums -- "f64" (float64 products of the float32
    terms), or "f32" (float32 products summed in float32 in index order, the device's terms in another order); the
    spread between the two is the step's own sensitivity to the summation."""
    assert sums in ("f64", "f32")
    p = default_params()
    p.update(kw)
    mp = np.asarray(mp, np.float32)
    mn = np.asarray(mn, np.float32)
    if maps is None:
        maps = view_maps(depth, cam, max_jump)
    V, N, _ = maps
    Vf, Nf = V.reshape(-1, 3), N.reshape(-1, 3)
    d = F(d_dist)
    rc = F(p["max_corr_dist"]) * d
    cm = mp.astype(np.float64).mean(axis=0)
    T = np.asarray(T_prev, np.float32).reshape(4, 4).astype(np.float64)
    Tf = np.asarray(T_prev, np.float32).reshape(4, 4).copy()
    it, converged, n_corr, A_last = 0, False, 0, None
    while it < p["max_iterations"]:
        pix, q, _ = correspondences(mp, mn, Tf, maps, cam, rc, p["min_normal_dot"])
        ok = pix >= 0
        n_corr = int(ok.sum())
        if n_corr < 6:
            break
        P, Q, Nq = q[ok], Vf[pix[ok]], Nf[pix[ok]]
        c = (T[:3, :3] @ cm + T[:3, 3]).astype(np.float32)
        e = P - Q
        r = (Nq[:, 0] * e[:, 0] + Nq[:, 1] * e[:, 1]) + Nq[:, 2] * e[:, 2]
        Jf = np.concatenate([np.cross(P - c, Nq), Nq], axis=1).astype(np.float32)
        if sums == "f32":
            A, g = np.zeros((6, 6)), np.zeros(6)
            for a in range(6):
                for b in range(a, 6):
                    A[a, b] = A[b, a] = np.cumsum(Jf[:, a] * Jf[:, b], dtype=np.float32)[-1]
                g[a] = np.cumsum(Jf[:, a] * r, dtype=np.float32)[-1]
        else:
            J = Jf.astype(np.float64)
            A = J.T @ J
            g = J.T @ r.astype(np.float64)
        A = A + 1e-6 * np.trace(A) / 6.0 * np.eye(6)
        A_last = A
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            break
        x = np.linalg.solve(L.T, np.linalg.solve(L, -g))
        dR, th = refine_ref.rodrigues(x[:3])
        R, t = T[:3, :3], T[:3, 3]
        cd = R @ cm + t
        Rn = refine_ref.gram_schmidt_columns(dR @ R)
        tn = dR @ t + (cd - dR @ cd + x[3:])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rn, tn
        Tf = T.astype(np.float32)
        Tf[3] = [0, 0, 0, 1]
        it += 1
        if th < F(p["stop_rot"]) and np.linalg.norm(x[3:]) < float(F(p["stop_trans"]) * d):
            converged = True
            break
    vp = dict(p["verify"])
    ver, _ = view_ref.verify(mp, mn, Tf, depth, cam, d_dist, depth_tol=vp.pop("depth_tol"), window=vp.pop("window"), **vp)
    cond = float(np.linalg.cond(A_last)) if A_last is not None else 0.0
    return Tf, dict(verify=ver, iterations=it, correspondences=n_corr, converged=converged, found=ver["found"], cond=cond)


# ---------------------------------------------------------------- part 3: the tracker
class Tracker:
    """models = [(points, normals, d_dist)] (the database members).  Tracks are dicts id, model, T, age, hits, misses,
    found."""

    def __init__(self, models, cam=None, max_jump=0.05, track_params=None, arbitrate_params=None, **kw):
        self.models = models
        self.cam, self.max_jump = cam, max_jump
        self.tp = track_params or {}
        self.ap = arbitrate_params or {}
        self.p = default_tracker_params()
        self.p.update(kw)
        self.centroid = [instances_ref.centroid(m[0]) for m in models]
        self.extent = [instances_ref.extent(m[0]) for m in models]
        self.tracks, self.next_id, self.frame = [], 0, 0

    @classmethod
    def from_shapes(cls, centroids, extents, **kw):
        self = cls([], **kw)
        self.centroid = [np.asarray(c, np.float32) for c in centroids]
        self.extent = [F(e) for e in extents]
        return self

    def update(self, detections):
        """detections: dicts with model and T.  Association by the same-instance test, birth for the rest."""
        for det in detections:
            j = int(det["model"])
            A = np.asarray(det["T"], np.float32).reshape(4, 4)
            sep2, cos_thr, rot_on = instances_ref.thresholds(self.p["assoc_min_separation"], self.p["assoc_max_angle"],
                                                             self.extent[j])
            pd = instances_ref.transformed_centroid(A, self.centroid[j])
            matched = any(t["model"] == j and instances_ref.same_instance(
                pd, A, instances_ref.transformed_centroid(t["T"], self.centroid[j]), t["T"], sep2, cos_thr, rot_on)
                for t in self.tracks)
            if matched:
                continue
            self.tracks.append(dict(id=self.next_id, model=j, T=A.copy(), age=0, hits=1, misses=0, found=1))
            self.next_id += 1
        return self.tracks

    def step(self, depth, detect=None):
        """One frame; detect: a callable returning the frame's detections (the search), or None.
        -> (live tracks, searched)."""
        if self.tracks:
            maps = view_maps(depth, self.cam, self.max_jump)
            out = [track(*self.models[t["model"]][:2], t["T"], depth, self.cam, self.models[t["model"]][2], self.max_jump,
                         maps=maps, **self.tp) for t in self.tracks]
            Tz = [o[0] if o[1]["found"] else np.zeros((4, 4), np.float32) for o in out]
            kept = [False] * len(out)
            if any(o[1]["found"] for o in out):
                _, kept = arbitrate_ref.arbitrate([self.models[t["model"]] for t in self.tracks], Tz, depth, self.cam, **self.ap)
            live = []
            for t, o, k in zip(self.tracks, out, kept):
                t["age"] += 1
                t["found"] = int(bool(o[1]["found"] and k))
                t["track"] = o[1]
                if t["found"]:
                    t["T"], t["hits"], t["misses"] = o[0], t["hits"] + 1, 0
                else:
                    t["misses"] += 1
                    if t["misses"] > self.p["max_misses"]:
                        continue
                live.append(t)
            self.tracks = live
        searched = False
        if detect is not None and (not self.tracks or self.frame % self.p["detect_every"] == 0):
            self.update(detect())
            searched = True
        self.frame += 1
        return self.tracks, searched


# ---------------------------------------------------------------- the smooth-motion stream of the tests
STREAM_CAM = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=0.001, z_min=0.5, z_max=12.0)
STREAM_MAX_JUMP = 0.08
STREAM_WALL = 9.0


def axis_rotation(axis, deg):
    k = np.asarray(axis, np.float64)
    return refine_ref.rodrigues(k / np.linalg.norm(k) * np.radians(deg))[0]


def smooth_poses(synth, d_dist, frames=10, **kw):
    """The object's ground-truth poses on the smooth-motion stream (synth.smooth_motion_poses)."""
    return synth.smooth_motion_poses(d_dist, frames=frames, **kw)


def render(synth, dense, T, wall=STREAM_WALL):
    """uint16 depth frame of the dense model cloud under T before the wall; T None: the wall alone."""
    pts = np.zeros((0, 3)) if T is None else dense @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]
    return synth.render_depth(pts, background_z=wall, splat=1)
