"""Numpy restatement of the colour volume (include/oslam.h at oslam_volume_integrate_colour, oslam_volume_colours and
oslam_volume_paint_view): the yardstick of the device path.

A coloured volume is a volume_ref.Volume with one more array, c: uint32 [nz, ny, nx], r | g << 8 | b << 16 | wc << 24.
The geometry of the colour pass is volume_ref.Volume.integrate's, float32 with the header's operation order; the mean is
integer arithmetic; the read at a point shares volume_ref's trilinear coordinates.  The shift is shift_ref.shifted with
the colours moved the same way.  numpy only: it runs wherever the tests do.
"""
import numpy as np

import shift_ref as S
import volume_ref as V

F = np.float32
U = np.uint32
DEFAULT_MAX_WEIGHT = 8


def pack(rgb, valid=None):
    """rgb uint8 [h, w, 3], valid [h, w] or None -> the image's words uint32 [h, w]: a = 255 with colour, the word 0
    without."""
    c = np.asarray(rgb, np.uint8).astype(U)
    words = c[..., 0] | c[..., 1] << U(8) | c[..., 2] << U(16) | U(0xff000000)
    if valid is not None:
        words = np.where(np.asarray(valid) != 0, words, U(0))
    return words.astype(U)


def unpack(words):
    """image or point words -> (rgb uint8 [..., 3], valid bool [...])"""
    w = np.asarray(words, U)
    rgb = np.stack([w & U(255), (w >> U(8)) & U(255), (w >> U(16)) & U(255)], axis=-1).astype(np.uint8)
    return rgb, (w >> U(24)) != 0


class Volume(V.Volume):
    """volume_ref.Volume with colour.  band None or 0: the volume's mu."""

    def __init__(self, *a, colour_max_weight=DEFAULT_MAX_WEIGHT, band=None, **kw):
        self.colour_max_weight = int(colour_max_weight)
        super().__init__(*a, **kw)
        self.band = self.mu if not band else F(band)
        assert 1 <= self.colour_max_weight <= 255 and F(0) < self.band <= self.mu

    def reset(self):
        super().reset()
        nx, ny, nz = self.n
        self.c = np.zeros((nz, ny, nx), U)

    # ------------------------------------------------------------ integration
    def coloured_mask(self, z, rgba, cam, T_vol_cam):
        """(the voxels the colour pass updates bool [nz, ny, nx], the pixel's word at each uint32 [nz, ny, nx])"""
        T = V.invert_pose(T_vol_cam)
        h, w = z.shape
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
            ok &= (sdf >= -self.band) & (sdf <= self.band)
        assert px.dtype == np.float32 and sdf.dtype == np.float32
        pix = np.asarray(rgba, U)[vi, ui]
        ok &= (pix >> U(24)) != 0
        return ok, pix

    def integrate_colour(self, z, rgba, cam, T_vol_cam):
        """oslam_volume_integrate_colour: the TSDF pass from z, then the colour pass from z and the image words rgba
        [h, w].  -> (voxels updated, voxels coloured)"""
        updated = self.integrate(z, cam, T_vol_cam)
        ok, pix = self.coloured_mask(z, rgba, cam, T_vol_cam)
        wc = (self.c >> U(24)).astype(np.uint64)
        out = np.zeros(self.c.shape, np.uint64)
        for sh in (0, 8, 16):
            ch = ((self.c >> U(sh)) & U(255)).astype(np.uint64)
            p = ((pix >> U(sh)) & U(255)).astype(np.uint64)
            out |= ((ch * wc + p + ((wc + 1) >> 1)) // (wc + 1)) << np.uint64(sh)
        out |= np.minimum(wc + 1, self.colour_max_weight) << np.uint64(24)
        self.c[ok] = out[ok].astype(U)
        return updated, int(ok.sum())

    # ------------------------------------------------------------ reads
    def colour_at(self, P):
        """The image word of the colour at each volume-frame point of P float32 [n, 3]: a = 255, or the word 0."""
        P = np.asarray(P, np.float32).reshape(-1, 3)
        out = np.zeros(len(P), U)
        with np.errstate(all="ignore"):
            u = [(P[:, a] - self.origin[a]) * self.inv_voxel for a in range(3)]
            c = [u[a] - F(0.5) for a in range(3)]
            b = [np.floor(v) for v in c]
            tri = np.ones(len(P), bool)
            for a in range(3):
                tri &= (b[a] >= F(0)) & (b[a] <= F(self.n[a] - 2))
            f = [c[a] - b[a] for a in range(3)]
            i, j, k = (np.where(tri, b[a], 0).astype(np.int64) for a in range(3))
            corner = [self.c[k + dk, j + dj, i + di] for dk in (0, 1) for dj in (0, 1) for di in (0, 1)]   # x fastest
            for w in corner:
                tri &= (w >> U(24)) != 0
            one = F(1.0)

            def lerp(p, q, t):
                return p * (one - t) + q * t

            word = np.full(len(P), 0xff000000, U)
            for sh in (0, 8, 16):
                v = [((w >> U(sh)) & U(255)).astype(np.float32) for w in corner]
                c00, c10 = lerp(v[0], v[1], f[0]), lerp(v[2], v[3], f[0])
                c01, c11 = lerp(v[4], v[5], f[0]), lerp(v[6], v[7], f[0])
                val = np.floor(lerp(lerp(c00, c10, f[1]), lerp(c01, c11, f[1]), f[2]) + F(0.5))
                assert val.dtype == np.float32
                word |= np.clip(np.where(tri, val, 0), 0, 255).astype(U) << U(sh)
            out[tri] = word[tri]
            # otherwise the voxel that holds the point
            n = [np.floor(u[a]) for a in range(3)]
            inr = ~tri
            for a in range(3):
                inr &= (n[a] >= F(0)) & (n[a] < F(self.n[a]))
            i, j, k = (np.where(inr, n[a], 0).astype(np.int64) for a in range(3))
            w = self.c[k, j, i]
            inr &= (w >> U(24)) != 0
            out[inr] = w[inr] | U(0xff000000)
        return out

    def colours(self, P):
        """oslam_volume_colours: -> (rgb uint8 [n, 3], valid bool [n])"""
        return unpack(self.colour_at(P))

    def paint(self, z, cam, T_vol_cam):
        """oslam_volume_paint_view over the z image of a view: -> the view's colour image, uint32 [h, w]"""
        M = np.asarray(T_vol_cam, np.float32).reshape(4, 4)
        h, w = z.shape
        fx, fy, cx, cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
        dx = (np.arange(w, dtype=np.float32)[None, :] - cx) / fx
        dy = (np.arange(h, dtype=np.float32)[:, None] - cy) / fy
        z = np.asarray(z, np.float32)
        vx, vy = dx * z, dy * z
        P = np.stack([((M[a, 0] * vx + M[a, 1] * vy) + M[a, 2] * z) + M[a, 3] for a in range(3)], axis=-1)
        assert P.dtype == np.float32
        return np.where(z > F(0), self.colour_at(P.reshape(-1, 3)).reshape(h, w), U(0)).astype(U)


def shifted(vol, s):
    """shift_ref.shifted with the colours moved as the words are: zeros (wc = 0) where no source voxel exists.  This is
    also what a shift through the voxel store leaves: the store keeps no colour."""
    out = S.shifted(vol, s)
    if out is None:
        return None
    out.c = np.zeros_like(vol.c)
    dst, src = [], []
    for a in (2, 1, 0):
        n, sa = vol.n[a], int(s[a])
        lo, hi = max(0, -sa), min(n, n - sa)
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + sa, hi + sa))
    out.c[tuple(dst)] = vol.c[tuple(src)]
    return out
