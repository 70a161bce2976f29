"""Numpy restatement of the fusion stage (include/oslam.h at oslam_volume_integrate and oslam_volume_raycast): the
yardstick of the device path.

Everything is float32 with the header's operation order, vectorised over voxels and over rays (with a mask for the rays
that are finished), so the volume's words, the ray-cast z image, its maps and the pinned counts equal the device's bit
for bit.  The frame-to-model tracking is the header's glue over camera_ref.egomotion.  numpy only: it runs wherever the
tests do.
"""
import numpy as np

import camera_ref as E
import track_ref as K
import view_ref

F = np.float32
MAX_STEPS = 1024


def invert_pose(T):
    """[R^T | -(R^T t)] formed in double and rounded to float32 (4x4)."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    D = T.astype(np.float64)
    inv = np.eye(4, dtype=np.float32)
    inv[:3, :3] = T[:3, :3].T
    for a in range(3):
        inv[a, 3] = F(-((D[0, a] * D[0, 3] + D[1, a] * D[1, 3]) + D[2, a] * D[2, 3]))
    return inv


def compose(A, B):
    """float32(double(A) * double(B)) with the element order of oslam_tracker_step_cam."""
    A = np.asarray(A, np.float32).reshape(4, 4).astype(np.float64)
    B = np.asarray(B, np.float32).reshape(4, 4).astype(np.float64)
    out = np.eye(4, dtype=np.float32)
    for a in range(3):
        for b in range(4):
            x = (A[a, 0] * B[0, b] + A[a, 1] * B[1, b]) + A[a, 2] * B[2, b]
            if b == 3:
                x = x + A[a, 3]
            out[a, b] = F(x)
    return out


def records(maps):
    """(V, N, has) -> the device's 8 floats per pixel: x y z has | nx ny nz 0."""
    V, N, has = maps
    out = np.zeros(has.shape + (8,), np.float32)
    out[..., :3], out[..., 3], out[..., 4:7] = V, has.astype(np.float32), N
    return out


class Volume:
    def __init__(self, nx, ny, nz, voxel, origin, mu=None, max_weight=128):
        self.n = (int(nx), int(ny), int(nz))
        self.voxel = F(voxel)
        self.inv_voxel = F(1.0) / self.voxel
        self.origin = np.asarray(origin, np.float32)
        self.mu = F(4.0) * self.voxel if mu is None else F(mu)
        self.max_weight = int(max_weight)
        self.reset()

    def reset(self):
        nx, ny, nz = self.n
        self.q = np.zeros((nz, ny, nx), np.int16)
        self.w = np.zeros((nz, ny, nx), np.uint16)

    # ------------------------------------------------------------ integration
    def integrate(self, z, cam, T_vol_cam, trace=None):
        """z: the view's z image (view_ref.view_z), float32 [h, w], 0 = not valid.  -> voxels updated.
        trace: a dict that receives the number of voxels per skip reason and per kind of update (added to what it
        holds); the volume and the return value do not depend on it."""
        T = invert_pose(T_vol_cam)
        h, w = z.shape
        nx, ny, nz = self.n
        fx, fy, cx, cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
        g = [self.origin[a] + (np.arange(self.n[a], dtype=np.float32) + F(0.5)) * self.voxel for a in range(3)]
        gx, gy, gz = g[0][None, None, :], g[1][None, :, None], g[2][:, None, None]
        with np.errstate(all="ignore"):
            px = ((T[0, 0] * gx + T[0, 1] * gy) + T[0, 2] * gz) + T[0, 3]
            py = ((T[1, 0] * gx + T[1, 1] * gy) + T[1, 2] * gz) + T[1, 3]
            pz = ((T[2, 0] * gx + T[2, 1] * gy) + T[2, 2] * gz) + T[2, 3]
            fu = np.floor(((px * fx) / pz + cx) + F(0.5))
            fv = np.floor(((py * fy) / pz + cy) + F(0.5))
            ok = (pz > F(0)) & (fu >= F(0)) & (fu < F(w)) & (fv >= F(0)) & (fv < F(h))
            ui = np.where(ok, fu, 0).astype(np.int64)
            vi = np.where(ok, fv, 0).astype(np.int64)
            zo = z[vi, ui]
            ok &= zo > F(0)
            sdf = zo - pz
            ok &= sdf >= -self.mu
            f = np.minimum(F(1.0), sdf / self.mu)
            wf = self.w.astype(np.float32)
            Fo = self.q.astype(np.float32) / F(32767.0)
            Fn = ((Fo * wf) + f) / (wf + F(1.0))
            qn = np.rint(np.where(ok, Fn, 0) * F(32767.0)).astype(np.int16)
        wn = np.minimum(self.w.astype(np.int32) + 1, self.max_weight).astype(np.uint16)
        assert px.dtype == np.float32 and Fn.dtype == np.float32
        if trace is not None:
            with np.errstate(all="ignore"):
                front = pz > F(0)
                in_u, in_v = (fu >= F(0)) & (fu < F(w)), (fv >= F(0)) & (fv < F(h))
                inside = front & in_u & in_v
                seen = inside & (zo > F(0))
                near = seen & (sdf >= -self.mu)
                counts = dict(behind=~front, outside=front & ~(in_u & in_v), off_left=front & (fu == F(-1)) & in_v,
                              off_right=front & (fu == F(w)) & in_v, off_top=front & (fv == F(-1)) & in_u,
                              off_bottom=front & (fv == F(h)) & in_u, hole=inside & ~seen, far=seen & ~near,
                              at_minus_mu=near & (sdf == -self.mu), clamped=near & (sdf / self.mu > F(1.0)),
                              band=near & (f > F(-1.0)) & (f < F(1.0)), updated=ok, w_max=ok & (wn == self.max_weight),
                              w_256=ok & (self.w == 255) & (wn == 256), q_max=ok & (qn == 32767), q_neg=ok & (qn < 0),
                              q_min=ok & (qn == -32767))
            for key, m in counts.items():
                trace[key] = trace.get(key, 0) + int(m.sum())
        self.q[ok] = qn[ok]
        self.w[ok] = wn[ok]
        return int(ok.sum())

    # ------------------------------------------------------------ reads
    def _nearest(self, x, y, z):
        """(F, w) of the voxel that holds each volume-frame point; w = 0 outside."""
        nx, ny, nz = self.n
        c = [np.floor((p - self.origin[a]) * self.inv_voxel) for a, p in enumerate((x, y, z))]
        inr = np.ones(x.shape, bool)
        for a in range(3):
            inr &= (c[a] >= F(0)) & (c[a] < F(self.n[a]))
        i, j, k = (np.where(inr, c[a], 0).astype(np.int64) for a in range(3))
        w = np.where(inr, self.w[k, j, i], 0)
        return self.q[k, j, i].astype(np.float32) / F(32767.0), w

    def _trilinear(self, x, y, z):
        """(value, has a value) at each volume-frame point."""
        c = [(p - self.origin[a]) * self.inv_voxel - F(0.5) for a, p in enumerate((x, y, z))]
        b = [np.floor(v) for v in c]
        ok = np.ones(x.shape, bool)
        for a in range(3):
            ok &= (b[a] >= F(0)) & (b[a] <= F(self.n[a] - 2))
        f = [c[a] - b[a] for a in range(3)]
        i, j, k = (np.where(ok, b[a], 0).astype(np.int64) for a in range(3))
        one = F(1.0)

        def corner(di, dj, dk):
            nonlocal ok
            ok &= self.w[k + dk, j + dj, i + di] > 0
            return self.q[k + dk, j + dj, i + di].astype(np.float32) / F(32767.0)

        def lerp(p, q, t):
            return p * (one - t) + q * t

        c00 = lerp(corner(0, 0, 0), corner(1, 0, 0), f[0])
        c10 = lerp(corner(0, 1, 0), corner(1, 1, 0), f[0])
        c01 = lerp(corner(0, 0, 1), corner(1, 0, 1), f[0])
        c11 = lerp(corner(0, 1, 1), corner(1, 1, 1), f[0])
        val = lerp(lerp(c00, c10, f[1]), lerp(c01, c11, f[1]), f[2])
        assert val.dtype == np.float32
        return val, ok

    # ------------------------------------------------------------ ray cast
    def raycast(self, T_vol_cam, cam, width, height, trace=None):
        """-> (z float32 [h, w], (V, N, has) as track_ref.view_maps, dict hits normals).
        trace: a dict that receives the number of rays per exit reason (added to what it holds); "zero_then_negative",
        the samples F < 0 that follow a sample F == 0 (no crossing: F_prev > 0 fails), and "zero_then_negative_live", those
        of them where a rule with F_prev >= 0 would have returned a hit (both trilinear reads have a value, Ftdt - Ft < 0
        and t* lies in its bracket and in [z_min, z_max]); "max_step", the largest step index a ray used; "exit", the
        reason of every pixel ([h, w] of str).  The result does not depend on it."""
        M = np.asarray(T_vol_cam, np.float32).reshape(4, 4)
        fx, fy, cx, cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
        z_min, z_max = F(cam["z_min"]), F(cam["z_max"])
        n = width * height
        u = np.arange(width, dtype=np.float32)[None, :]
        v = np.arange(height, dtype=np.float32)[:, None]
        dx = np.broadcast_to((u - cx) / fx, (height, width)).reshape(-1).astype(np.float32)
        dy = np.broadcast_to((v - cy) / fy, (height, width)).reshape(-1).astype(np.float32)
        o = M[:3, 3]
        D = [(M[a, 0] * dx + M[a, 1] * dy) + M[a, 2] for a in range(3)]
        tn, tf = np.full(n, z_min, np.float32), np.full(n, z_max, np.float32)
        miss = np.zeros(n, bool)
        with np.errstate(all="ignore"):
            for a in range(3):
                lo = self.origin[a] + self.voxel
                hi = self.origin[a] + F(self.n[a] - 1) * self.voxel
                zero = D[a] == F(0)
                miss |= zero & ~((o[a] >= lo) & (o[a] <= hi))
                ta, tb = (lo - o[a]) / D[a], (hi - o[a]) / D[a]
                tn = np.where(zero, tn, np.maximum(tn, np.minimum(ta, tb)))
                tf = np.where(zero, tf, np.minimum(tf, np.maximum(ta, tb)))
            active = ~miss & (tn <= tf)
        why = np.full(n, "exhausted", dtype="U16") if trace is not None else None      # marched to tf without a crossing
        if trace is not None:
            any_zero = (D[0] == F(0)) | (D[1] == F(0)) | (D[2] == F(0))
            why[miss] = "zero_miss"
            why[~miss & ~active] = "empty"
            gap = np.zeros(n, bool)                       # the ray forgot a sample it had: an unseen gap
            tr = dict(zero_inside=int((any_zero & ~miss).sum()), zero_marched=int((any_zero & active).sum()),
                      tn_is_z_min=int((active & (tn == z_min)).sum()), tf_is_z_max=int((active & (tf == z_max)).sum()),
                      zero_then_negative=0, zero_then_negative_live=0, max_step=-1)
        step = F(0.5) * self.mu
        have = np.zeros(n, bool)
        Fp, tp, ts = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        for k in range(MAX_STEPS):
            idx = np.flatnonzero(active)
            if idx.size == 0:
                break
            t = tn[idx] + F(k) * step
            alive = t <= tf[idx]
            active[idx[~alive]] = False
            idx, t = idx[alive], t[alive]
            if trace is not None and idx.size:
                tr["max_step"] = k
            x, y, zz = (o[a] + D[a][idx] * t for a in range(3))
            Fc, w = self._nearest(x, y, zz)
            seen = w > 0
            if trace is not None:
                gap[idx[~seen & have[idx]]] = True
                zn = seen & have[idx] & (Fp[idx] == F(0)) & (Fc < F(0))
                tr["zero_then_negative"] += int(zn.sum())
                if zn.any():
                    iz = idx[zn]
                    Fa, oka = self._trilinear(*(o[a] + D[a][iz] * tp[iz] for a in range(3)))
                    Fb, okb = self._trilinear(x[zn], y[zn], zz[zn])
                    with np.errstate(all="ignore"):
                        tz = tp[iz] - (step * Fa) / (Fb - Fa)
                        live = oka & okb & (Fb - Fa < F(0)) & (tz >= tp[iz]) & (tz <= t[zn]) & (tz >= z_min) & (tz <= z_max)
                    tr["zero_then_negative_live"] += int(live.sum())
            have[idx[~seen]] = False
            cross = seen & have[idx] & (Fp[idx] > F(0)) & (Fc < F(0))
            back = seen & ~cross & have[idx] & (Fp[idx] < F(0)) & (Fc > F(0))
            rest = seen & ~cross & ~back
            active[idx[cross | back]] = False
            if trace is not None:
                why[idx[back]] = "back_face"
            ic = idx[cross]
            if ic.size:
                tpc, tc = tp[ic], t[cross]
                Ft, ok0 = self._trilinear(*(o[a] + D[a][ic] * tpc for a in range(3)))
                Ftdt, ok1 = self._trilinear(x[cross], y[cross], zz[cross])
                with np.errstate(all="ignore"):
                    den = Ftdt - Ft
                    tstar = tpc - (step * Ft) / den
                    good = ok0 & ok1 & (den < F(0)) & (tstar >= tpc) & (tstar <= tc) & (tstar >= z_min) & (tstar <= z_max)
                ts[ic[good]] = tstar[good]
                if trace is not None:
                    with np.errstate(all="ignore"):
                        for name, m in (("z_cut", ~((tstar >= z_min) & (tstar <= z_max))),
                                        ("off_bracket", ~((tstar >= tpc) & (tstar <= tc))), ("den", ~(den < F(0))),
                                        ("trilinear", ~(ok0 & ok1)), ("hit", good)):       # the first that fails names it
                            why[ic[m]] = name
            ir = idx[rest]
            have[ir] = True
            Fp[ir] = Fc[rest]
            tp[ir] = t[rest]
        hit = ts > F(0)
        ih = np.flatnonzero(hit)
        V, N, has = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
        if ih.size:
            t = ts[ih]
            p = [o[a] + D[a][ih] * t for a in range(3)]
            g, ok = [], np.ones(ih.size, bool)
            for a in range(3):
                hi_p = [p[b] + self.voxel if b == a else p[b] for b in range(3)]
                lo_p = [p[b] - self.voxel if b == a else p[b] for b in range(3)]
                v1, ok1 = self._trilinear(*hi_p)
                v0, ok0 = self._trilinear(*lo_p)
                ok &= ok1 & ok0
                g.append(v1 - v0)
            with np.errstate(all="ignore"):
                ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(np.float32)
                ok &= (ln > F(0)) & (ln <= F(3.0e38))
                nv = [g[a] / ln for a in range(3)]
                nc = [(M[0, a] * nv[0] + M[1, a] * nv[1]) + M[2, a] * nv[2] for a in range(3)]
                vx, vy = dx[ih] * t, dy[ih] * t
                ok &= ((nc[0] * vx + nc[1] * vy) + nc[2] * t) < F(0)
            sel = ih[ok]
            has[sel] = True
            V[sel] = np.stack([vx[ok], vy[ok], t[ok]], axis=1)
            N[sel] = np.stack([nc[0][ok], nc[1][ok], nc[2][ok]], axis=1)
        shape = (height, width)
        if trace is not None:
            why[hit & ~has] = "no_normal"
            tr["gap_then_hit"] = int((gap & hit).sum())
            for name in ("zero_miss", "empty", "exhausted", "back_face", "trilinear", "den", "off_bracket", "z_cut", "no_normal",
                         "hit"):
                tr[name] = int((why == name).sum())
            for key, val in tr.items():
                trace[key] = max(trace.get(key, -1), val) if key == "max_step" else trace.get(key, 0) + val
            trace["exit"] = why.reshape(shape)
        return ts.reshape(shape), (V.reshape(shape + (3,)), N.reshape(shape + (3,)), has.reshape(shape)), \
            dict(hits=int(hit.sum()), normals=int(has.sum()))

    # ------------------------------------------------------------ frame-to-model tracking
    def track(self, frame_maps, cam, T_prev, sums="f64", **kw):
        """oslam_volume_track: -> (T_vol_cam float32 4x4, the egomotion result dict)."""
        h, w = frame_maps[2].shape
        _, model, _ = self.raycast(T_prev, cam, w, h)
        T, r = E.egomotion(frame_maps, model, cam, sums=sums, **kw)
        return compose(T_prev, T), r


def z_image(depth, cam):
    return view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])


# ---------------------------------------------------------------- the room of camera_ref at a size the CPU can afford
SMALL = dict(width=320, height=240, fx=262.5, fy=262.5, cx=159.5, cy=119.5)
SMALL_CAM = dict(E.CAM, fx=262.5, fy=262.5, cx=159.5, cy=119.5)
ROOM_VOXEL = 0.05
ROOM_MU = 0.40                  # 8 voxels: see tests/test_volume_host.py for why the default of 4 is too thin for this room
# the bounds of tests/test_volume_host.py for the end pose of the there-and-back loop (1.5 times its worst seed)
MODEL_ROT_BOUND, MODEL_TRANS_BOUND = 1.5 * 0.0262, 1.5 * 0.0027


def room_volume(seed, voxel=ROOM_VOXEL, cls=Volume, **kw):
    """A volume around what the camera of camera_ref.trajectory sees of camera_ref.make_world(seed), in the frame of the
    first camera: x from the side wall to the far end of the back wall, y from above the image to below the floor, z to
    behind the back wall."""
    lo = np.array([-2.9, -4.3, 0.3])
    hi = np.array([6.3, 1.9, E.WORLD_DEPTH + 0.4 * seed + 0.5])
    n = [int(np.ceil((hi[a] - lo[a]) / voxel / 8.0)) * 8 for a in range(3)]
    kw.setdefault("mu", ROOM_MU)
    return cls(n[0], n[1], n[2], voxel, [float(x) for x in lo], **kw)


def small_stream(synth, seed):
    """The world, the 10 poses and the 320 x 240 frames of seed `seed` with their z images and maps."""
    world = E.make_world(synth, seed)
    traj = E.trajectory(synth, seed)
    imgs = [E.render(synth, world, T, **SMALL) for T in traj]
    return dict(world=world, traj=traj, imgs=imgs, z=[z_image(im, SMALL_CAM) for im in imgs],
                maps=[K.view_maps(im, SMALL_CAM, E.MAX_JUMP) for im in imgs])


THERE_AND_BACK = list(range(10)) + list(range(8, -1, -1))


def between(synth, seed, k=9):
    """A true pose of the stream that is none of its frames: step k of the same motion at half the rate."""
    return E.trajectory(synth, seed, frames=20, deg=1.5, step=0.015)[k]


def there_and_back(vol, s, cam=SMALL_CAM, sums="f64"):
    """The frame-to-model loop of ppf.Volume.step over frames 0..9, 8..0 -> [(frame, T_vol_cam, result or None)]."""
    T = np.eye(4, dtype=np.float32)
    vol.integrate(s["z"][0], cam, T)
    out = [(0, T, None)]
    for f in THERE_AND_BACK[1:]:
        Tn, r = vol.track(s["maps"][f], cam, T, sums=sums)
        if r["ok"]:
            T = Tn
            vol.integrate(s["z"][f], cam, T)
        out.append((f, T, r))
    return out
