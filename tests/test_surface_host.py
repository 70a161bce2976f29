"""CPU: the surface extraction's arguments (include/oslam.h at oslam_volume_surface) and its restatement
(tests/surface_ref.py) against analysis, on volumes written directly into the restatement.

The analytic volumes are 24^3 with voxel 0.05 and origin 0, the field F = clamp(sdf / mu) with mu = 6 voxels, stored
as the integration stores it (q = rintf(F * 32767) in float32), unseen where sdf < -mu.

Bounds (derived, not measured).  e = 0.5 / 32767 is the most a stored F is off.
  Point.  Along an edge a plane's sdf is linear, so with t = F0' / (F0' - F1') from the stored F' = F + e_i the point's
    sdf / mu = F0 - t (F0 - F1) = -(1 - t) e_0 - t e_1, at most e in size: the point lies within mu * e of the plane.
    The asserted bound is mu / 32767 = 2 mu e; the second half is room for the float32 operations (coordinates up to
    1.2 m carry 2^-24 * 1.2 = 7e-8 m per rounding, a dozen roundings are 1e-6 m, mu * e is 4.6e-6 m).
  Normal.  The trilinear read of a linear field is exact, and a read of the stored field is a convex combination of
    stored values, so it is off by at most e, plus r = 32 * 2^-24 for its float32 operations (7 lerps of 3 roundings
    each on values below 1, and the fractions' own rounding, 3 operations on coordinates below 24 voxels, times the
    field's slope of at most 1/6 per voxel).  mu = 6 voxels keeps every corner of the reads unclamped and seen: a corner
    is at most 2 voxels from the point on each axis, 2 * sqrt(3) = 3.5 voxels from the plane.  So each g_b = F(P + voxel
    e_b) - F(P - voxel e_b) is off by at most 2 (e + r), the gradient by sqrt(3) * 2 (e + r) in length, against the true
    |g| = 2 voxel |n| / mu = 1/3: the angle is at most asin(sqrt(3) * 2 (e + r) / (1/3)) = 1.8e-4 rad.
  Count.  For a field none of whose voxel centres has |F| < 1 / 32767 the sign of the stored q is the sign of F, so
    the crossings are the sign changes of the analytic field, counted here in float64.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as S  # noqa: E402

N, VOXEL = 24, 0.05
MU = 6 * VOXEL
E_Q = 0.5 / 32767.0
R_F32 = 32.0 * 2.0 ** -24
POINT_BOUND = MU / 32767.0
ANGLE_BOUND = float(np.arcsin(np.sqrt(3.0) * 2.0 * (E_Q + R_F32) / (2.0 * VOXEL / MU)))

PLANES = [("axis-aligned", (1.0, 0.0, 0.0), 12.3 * VOXEL), ("45 degrees", (1.0, 1.0, 0.0), 16.9 * VOXEL),
          ("general", (0.3, -0.5, 0.8), 7.37 * VOXEL)]


def centres64():
    c = (np.arange(N, dtype=np.float64) + 0.5) * VOXEL
    return c[None, None, :], c[None, :, None], c[:, None, None]


def analytic_volume(sdf64):
    """the field sdf (float64, [nz, ny, nx]) stored as the integration stores it"""
    vol = S.blank(N, N, N, voxel=VOXEL, mu=MU)
    sdf = sdf64.astype(np.float32)
    f = np.minimum(np.float32(1.0), sdf / vol.mu)
    seen = sdf >= -vol.mu
    vol.q[seen] = np.rint(f[seen] * np.float32(32767.0)).astype(np.int16)
    vol.w[seen] = 1
    return vol


def sign_changes64(sdf64):
    """sign changes of the analytic field along the legal edges between voxels with sdf >= -mu, in float64"""
    assert np.abs(sdf64 / MU).min() >= 1.0 / 32767.0               # no voxel centre within 1/32767 of the surface
    seen, neg, n = sdf64 >= -MU, sdf64 < 0, 0
    for ax in range(3):
        lo = tuple(slice(None, -1) if d == ax else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == ax else slice(None) for d in range(3))
        n += int((seen[lo] & seen[hi] & (neg[lo] != neg[hi])).sum())
    return n


def test_planes_points_normals_and_counts():
    assert 1.5e-4 < ANGLE_BOUND < 2.0e-4
    x, y, z = centres64()
    for name, nv, d in PLANES:
        nv = np.asarray(nv, np.float64) / np.linalg.norm(nv)
        sdf = nv[0] * x + nv[1] * y + nv[2] * z - d
        vol = analytic_volume(sdf)
        tr = {}
        xyz, nrm, crossings = S.surface(vol, trace=tr)
        assert crossings == sign_changes64(sdf) >= N * N, name
        assert len(xyz) == tr["points"] > crossings // 2, (name, tr)   # only the crossings near the faces lose their normal
        assert tr["drop_unseen_corner"] == 0 and tr["drop_len_zero"] == 0, (name, tr)
        dist = np.abs(xyz.astype(np.float64) @ nv - d)
        n64 = nrm.astype(np.float64)                                    # atan2 of sine and cosine: acos loses small angles
        ang = np.arctan2(np.linalg.norm(np.cross(n64, nv), axis=1), n64 @ nv)
        print("%s: %d crossings, %d points, max distance %.3e m (bound %.3e), max angle %.3e rad (bound %.3e)"
              % (name, crossings, len(xyz), dist.max(), POINT_BOUND, ang.max(), ANGLE_BOUND))
        assert dist.max() <= POINT_BOUND, (name, dist.max())
        assert ang.max() <= ANGLE_BOUND, (name, ang.max())              # outward: towards growing F
        assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_sphere_count():
    x, y, z = centres64()
    c, r = np.array([0.61, 0.58, 0.63]), 0.33
    sdf = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
    vol = analytic_volume(sdf)
    xyz, nrm, crossings = S.surface(vol)
    assert crossings == sign_changes64(sdf) > 500
    dist = np.abs(np.linalg.norm(xyz.astype(np.float64) - c, axis=1) - r)
    out = (nrm.astype(np.float64) * (xyz.astype(np.float64) - c)).sum(axis=1)
    print("sphere: %d crossings, %d points, max distance %.3e m (a measurement: the field is not linear along an edge)"
          % (crossings, len(xyz), dist.max()))
    assert len(xyz) == crossings and np.all(out > 0)                  # far from the faces: every crossing has its normal


def test_order_and_determinism_of_the_restatement():
    vol = S.sparse_random(40, 72, 24, seed=5)
    a, b = S.surface(vol), S.surface(vol)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] > 100
    # min_weight drops edges and never adds one
    assert S.surface(vol, 3)[2] < a[2]


def test_edge_inputs_reach_their_branches():
    for dims in ((16, 16, 16), (40, 72, 24)):
        for mw in (1, 3):
            tr = {}
            xyz, nrm, crossings = S.surface(S.edge_inputs(*dims, min_weight=mw), mw, trace=tr)
            print(dims, mw, tr)
            assert crossings == tr["crossings"] and len(xyz) == tr["points"] > 0
            for key in ("zero_negative", "zero_positive", "q_max", "q_min", "w_below_min_0", "w_below_min_1", "w_at_min_0",
                        "w_at_min_1", "w_65535_0", "w_65535_1", "last_edge_x", "last_edge_y", "last_edge_z", "wrap_x",
                        "drop_unseen_corner", "drop_low_x", "drop_low_y", "drop_low_z", "drop_high_x", "drop_high_y",
                        "drop_high_z"):
                assert tr[key] > 0, (dims, mw, key)
            # the voxel with w = min_weight - 1 has six edges with a sign change and none of them is a crossing
            assert tr["sign_change_unseen"] >= 6
    # q0 == 0 with a positive neighbour is no crossing: a zero among positive voxels leaves the volume without any
    vol = S.blank(16, 16, 16)
    vol.q[:], vol.w[:] = 700, 1
    S.put(vol, 8, 8, 8, 0, 1)
    tr = {}
    assert S.surface(vol, trace=tr)[2] == 0 and tr["zero_positive"] == 6
    S.put(vol, 9, 8, 8, -700, 1)                                        # ... and with a negative one it is found once
    tr = {}
    xyz, _, crossings = S.surface(vol, trace=tr)
    assert crossings == 6 and tr["zero_negative"] == 1 and tr["zero_positive"] == 5
    assert np.any(np.all(xyz == np.float32([np.float32(8.5) * vol.voxel, np.float32(8.5) * vol.voxel, np.float32(8.5) * vol.voxel]), axis=1))


def test_wrap_bait_checkerboard_and_single_crossings():
    tr = {}
    xyz, nrm, crossings = S.surface(S.wrap_bait(), trace=tr)
    assert crossings == 0 and len(xyz) == 0 and tr["wrap_x"] == tr["wrap_y"] == tr["wrap_z"] == 1
    tr = {}
    xyz, nrm, crossings = S.surface(S.checkerboard(), trace=tr)
    assert crossings == 11520 and tr["drop_len_zero"] > 1000 and tr["points"] == len(xyz) < crossings
    assert all(tr["drop_%s_%s" % (side, ax)] > 0 for side in ("low", "high") for ax in "xyz")
    for a, vol in enumerate(S.single_crossings()):
        tr = {}
        xyz, nrm, crossings = S.surface(vol, trace=tr)
        assert crossings == 1 and len(xyz) == 0 and tr["last_edge_" + "xyz"[a]] == 1


# ---------------------------------------------------------------- ABI
def test_surface_defaults(built_lib, ppf):
    p = ppf.default_surface_params()
    assert p.min_weight == 1 and list(p.reserved) == [0] * 7 and C.sizeof(ppf.SurfaceParams) == 32
    assert C.sizeof(ppf.SurfaceResult) == 16
    assert ppf.default_surface_params(min_weight=7).min_weight == 7
    with pytest.raises(TypeError):
        ppf.default_surface_params(no_such_field=1)


def test_surface_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    """Every OSLAM_E_INVALID case of the three entry points with a stand-in handle (zeroed host memory: device 0), on a
    machine with or without a GPU."""
    L = ppf.lib()
    fa = C.create_string_buffer(4096)
    vol = C.cast(fa, C.c_void_p)
    INV = ppf.OSLAM_E_INVALID
    n, h = C.c_size_t(0), C.c_void_p(0)
    buf = np.zeros(64, np.float32)
    q, w = np.zeros(8, np.int16), np.zeros(8, np.uint16)
    ok = ppf.default_surface_params()

    def surface(vo=vol, sp=ok, xyz=buf, nrm=buf, cap=4, n_out=C.byref(n)):
        return L.oslam_volume_surface(vo, C.byref(sp) if sp is not None else None, ppf._p(xyz) if xyz is not None else None,
                                      ppf._p(nrm) if nrm is not None else None, cap, n_out, None)

    def from_volume(vo=vol, sp=ok, leaf=0.0, d_dist=0.1, df=1, out=C.byref(h)):
        return L.oslam_scene_from_volume(vo, C.byref(sp) if sp is not None else None, leaf, d_dist, df, None, out, C.byref(n))

    assert L.oslam_surface_params_default(None) == INV
    assert surface(vo=None) == surface(n_out=None) == INV
    assert surface(xyz=None) == surface(nrm=None) == INV                 # one output without the other
    assert surface(xyz=None, nrm=None, cap=4) == INV                     # no outputs: cap must be 0
    for mw in (0, 65536):
        bad = ppf.default_surface_params(min_weight=mw)
        assert surface(sp=bad) == surface(sp=bad, xyz=None, nrm=None, cap=0) == from_volume(sp=bad) == INV, mw
    assert "min_weight" in L.oslam_last_error().decode()
    assert from_volume(vo=None) == from_volume(out=None) == INV
    assert from_volume(leaf=-1.0) == from_volume(leaf=float("nan")) == from_volume(d_dist=-0.5) == from_volume(df=0) == INV
    assert not h.value
    assert L.oslam_volume_set_voxels(None, ppf._p(q), ppf._p(w)) == L.oslam_volume_set_voxels(vol, None, ppf._p(w)) == INV
    assert L.oslam_volume_set_voxels(vol, ppf._p(q), None) == INV
