"""CPU: the shifting window's restatement (tests/shift_ref.py) against the rule of include/oslam.h at oslam_volume_shift,
the library's argument checks, and oslam_volume_follow, which is host arithmetic and runs without a device.

The calls that read a volume's parameters get a stand-in handle: host memory laid out as the library's oslam_volume
(csrc/oslam_internal.h), filled here.  No call in this file reaches a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as M  # noqa: E402
import shift_ref as H  # noqa: E402
import surface_ref as S  # noqa: E402

F = np.float32
RAGGED = (40, 72, 24)
EXACT = dict(voxel=0.0625, origin=(-1.25, 2.0, 0.5))              # voxel centres and crossings' grid are exact in float32


def exact_frame(vol, voxel=EXACT["voxel"], origin=EXACT["origin"]):
    vol.voxel = F(voxel)
    vol.inv_voxel = F(1.0) / vol.voxel
    vol.origin = np.asarray(origin, np.float32)
    return vol


def full_range(n, seed):
    """every bit of the 32-bit words in use: q over all of int16, w over all of uint16"""
    rng = np.random.default_rng(seed)
    vol = S.blank(*n)
    shape = (n[2], n[1], n[0])
    words = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    vol.q[:] = (words & 0xffff).astype(np.uint16).view(np.int16)
    vol.w[:] = (words >> 16).astype(np.uint16)
    return vol


# ---------------------------------------------------------------- the restatement
def test_words_move_and_the_rest_is_unseen():
    vol = full_range(RAGGED, 1)
    nx, ny, nz = vol.n
    for s in [(1, 0, 0), (-1, 0, 0), (4, 0, 0), (3, -5, 2), (0, 8, 0), (0, 0, -(nz - 1)), (nx - 1, 0, 0)]:
        out = H.shifted(vol, s)
        assert out.off == s and out.q.shape == vol.q.shape
        rng = np.random.default_rng(7)
        for i, j, k in zip(rng.integers(0, nx, 200), rng.integers(0, ny, 200), rng.integers(0, nz, 200)):
            si, sj, sk = i + s[0], j + s[1], k + s[2]
            if 0 <= si < nx and 0 <= sj < ny and 0 <= sk < nz:
                assert (out.q[k, j, i], out.w[k, j, i]) == (vol.q[sk, sj, si], vol.w[sk, sj, si]), (s, i, j, k)
            else:
                assert (out.q[k, j, i], out.w[k, j, i]) == (0, 0), (s, i, j, k)
        overlap = np.prod([vol.n[a] - abs(s[a]) for a in range(3)])
        assert H.kept(out) <= overlap and (out.w != 0).sum() + (out.q != 0).sum() > 0
    for s in [(nx, 0, 0), (nx + 5, -3, 0), (0, -ny, 0), (0, 0, 1 << 20)]:
        out = H.shifted(vol, s)
        assert not out.q.any() and not out.w.any() and out.off == s
    same = H.shifted(vol, (0, 0, 0))
    assert same.q.tobytes() == vol.q.tobytes() and same.w.tobytes() == vol.w.tobytes() and same.off == (0, 0, 0)
    assert H.shifted(vol, ((1 << 20) + 1, 0, 0)) is None
    assert H.shifted(H.shifted(vol, (1 << 20, 0, 0)), (1, 0, 0)) is None              # the offset's limit


def test_origin_is_derived_and_comes_back_bit_for_bit():
    vol = full_range((16, 16, 16), 2)
    vol.voxel, vol.origin = F(0.02), np.array([-0.0, 0.1, -1.28], np.float32)
    s = (3, -5, 2)
    out = H.shifted(vol, s)
    want = [vol.origin[a] + F(F(s[a]) * vol.voxel) for a in range(3)]
    assert out.origin.tobytes() == np.array(want, np.float32).tobytes()
    two = H.shifted(out, (5, 5, 0))                                # derived from the offset, not added to the last origin
    assert two.off == (8, 0, 2) and two.origin[1].tobytes() == vol.origin[1].tobytes()
    assert two.origin[0] == vol.origin[0] + F(F(8) * vol.voxel)
    back = H.shifted(out, (-3, 5, -2))
    assert back.off == (0, 0, 0) and back.origin.tobytes() == vol.origin.tobytes() and np.signbit(back.origin[0])
    inner = (slice(2, 16), slice(0, 11), slice(3, 16))             # [k, j, i] of the overlap: what stayed both times
    assert back.q[inner].tobytes() == vol.q[inner].tobytes() and back.w[inner].tobytes() == vol.w[inner].tobytes()
    mask = np.ones(vol.q.shape, bool)
    mask[inner] = False
    assert not back.q[mask].any() and not back.w[mask].any()
    a, b = H.shifted(H.shifted(vol, (1, 2, 3)), (2, -1, 1)), H.shifted(vol, (3, 1, 4))
    assert a.off == b.off and a.origin.tobytes() == b.origin.tobytes()
    assert (a.w != 0).sum() <= (b.w != 0).sum()                    # two steps lose at least what one step loses


def test_nothing_is_lost_and_nothing_twice():
    """surface's crossings before a shift = the leaving ones + the crossings after it; with voxel centres that are exact
    in float32 the positions that stay are the same bytes in the same order.  The figures are the header's example."""
    s = (3, -5, 2)
    vol = exact_frame(M.random_signs(*RAGGED, 5, 0.02))
    key, xyz, _ = M.vertices(vol, 1, normals=False)
    gone = H.leaving_keys(vol, key, s)
    after = H.shifted(vol, s)
    _, xyz_after, _ = M.vertices(after, 1, normals=False)
    _, _, n_leave = H.leaving(vol, s)
    assert (len(key), n_leave, len(xyz_after)) == (96489, 20601, 75888)
    assert n_leave == int(gone.sum()) and xyz[~gone].tobytes() == xyz_after.tobytes()
    for mw, shifts in ((1, [(1, 0, 0), (0, 0, -23), (40, 0, 0), (0, 0, 0)]), (3, [(-8, 8, 0)])):
        for t in shifts:
            lx, ln, lc = H.leaving(vol, t, mw)
            sx, sn, sc = S.surface(vol, mw)
            assert lc + S.surface(H.shifted(vol, t), mw)[2] == sc, (mw, t)
            if t == (40, 0, 0):                                    # the whole volume leaves: the surface itself
                assert lx.tobytes() == sx.tobytes() and ln.tobytes() == sn.tobytes() and lc == sc
            if t == (0, 0, 0):
                assert (len(lx), lc) == (0, 0)
    # voxel 0.05: the counts still partition, the positions differ in the last bit
    vol = M.random_signs(*RAGGED, 5, 0.02)
    key, xyz, _ = M.vertices(vol, 1, normals=False)
    gone = H.leaving_keys(vol, key, s)
    _, xyz_after, _ = M.vertices(H.shifted(vol, s), 1, normals=False)
    assert len(xyz_after) == len(key) - int(gone.sum()) and np.abs(xyz[~gone] - xyz_after).max() < 1e-6


def test_a_staying_voxels_edge_into_a_leaving_one_leaves():
    vol = S.blank(16, 16, 16)
    S.put(vol, 7, 5, 5, 3000, 2)
    S.put(vol, 8, 5, 5, -1000, 2)
    key = np.array([3 * (7 + 16 * (5 + 16 * 5))])
    assert not H.leaving_keys(vol, key, (7, 0, 0))[0]              # voxels 7 and 8 become 0 and 1
    assert H.leaving_keys(vol, key, (8, 0, 0))[0]                  # 7 leaves, 8 stays: the edge's start is gone
    assert H.leaving_keys(vol, key, (-8, 0, 0))[0]                 # 7 stays as 15, 8 leaves: 15 has no +x edge
    assert not H.leaving_keys(vol, key, (-7, 0, 0))[0]
    assert H.leaving(vol, (-8, 0, 0))[2] == 1 and S.surface(H.shifted(vol, (-8, 0, 0)))[2] == 0


# ---------------------------------------------------------------- ABI
class KVolume(C.Structure):
    _fields_ = [("words", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("voxel", C.c_float),
                ("inv_voxel", C.c_float), ("origin", C.c_float * 3), ("mu", C.c_float), ("max_weight", C.c_uint32)]


def stand_in(ppf, ref, off=(0, 0, 0)):
    """host memory laid out as csrc/oslam_internal.h's struct oslam_volume, with the restated volume's parameters"""
    class Handle(C.Structure):
        _fields_ = [("dev", C.c_int), ("k", KVolume), ("p", ppf.VolumeParams), ("off", C.c_int * 3), ("spare", C.c_void_p)]

    h = Handle()
    origin0, _ = H.state(ref)
    h.p.nx, h.p.ny, h.p.nz = ref.n
    h.p.voxel, h.p.mu, h.p.max_weight = float(ref.voxel), float(ref.mu), ref.max_weight
    h.p.origin[:] = [float(x) for x in origin0]
    h.k.nx, h.k.ny, h.k.nz = ref.n
    h.k.voxel, h.k.inv_voxel, h.k.mu, h.k.max_weight = h.p.voxel, float(ref.inv_voxel), h.p.mu, ref.max_weight
    h.k.origin[:] = [float(x) for x in H.window_origin(origin0, off, ref.voxel)]
    h.off[:] = list(off)
    return h


def default_volume():
    return S.blank(256, 256, 256, voxel=0.02, origin=(F(-128.0) * F(0.02), F(-128.0) * F(0.02), 0.0))


def lib_follow(ppf, h, T, fp=None):
    s = np.full(3, 99, np.int32)
    rc = ppf.lib().oslam_volume_follow(C.byref(h), ppf._p(ppf._pose16(T)), C.byref(fp) if fp is not None else None, ppf._p(s))
    return rc, tuple(int(x) for x in s)


def test_structures(built_lib, ppf):
    assert C.sizeof(ppf.ShiftResult) == 24 and C.sizeof(ppf.FollowParams) == 32
    h = stand_in(ppf, default_volume())
    fp = ppf.FollowParams()
    assert ppf.lib().oslam_follow_params_default(C.byref(h), C.byref(fp)) == 0
    d = H.follow_defaults(default_volume())
    assert (fp.lookahead, fp.threshold, fp.granule) == (d["lookahead"], d["threshold"], d["granule"]) == (F(2.56), 64.0, 8)
    assert list(fp.reserved) == [0] * 5


def test_shift_rejects_bad_arguments_before_touching_a_device(built_lib, ppf):
    L = ppf.lib()
    INV = ppf.OSLAM_E_INVALID
    ref = S.blank(16, 16, 16)
    h = stand_in(ppf, ref)
    vol = C.byref(h)
    n, res, sres = C.c_size_t(0), ppf.ShiftResult(), ppf.SurfaceResult()
    buf, off, org = np.zeros(64, np.float32), np.zeros(3, np.int32), np.zeros(3, np.float32)
    ok = ppf.default_surface_params()

    def s3(*s):
        return ppf._p(np.array(s, np.int32))

    big = (1 << 20) + 1
    assert L.oslam_volume_shift(None, s3(1, 0, 0), None) == L.oslam_volume_shift(vol, None, None) == INV
    for s in [(big, 0, 0), (0, -big, 0), (0, 0, big)]:
        assert L.oslam_volume_shift(vol, s3(*s), C.byref(res)) == INV, s
    assert "2^20" in L.oslam_last_error().decode()
    # a zero shift returns at once: no launch, the offset as it is
    assert L.oslam_volume_shift(vol, s3(0, 0, 0), C.byref(res)) == 0
    assert (tuple(res.offset), res.kept, res.launches) == ((0, 0, 0), 0, 0)
    # the offset's limit, from both sides of it, with the window at 2^20 - 8 on x and -2^20 on z
    h2 = stand_in(ppf, ref, off=((1 << 20) - 8, 0, -(1 << 20)))
    res.offset[:] = [7, 7, 7]
    assert L.oslam_volume_shift(C.byref(h2), s3(9, 0, 0), C.byref(res)) == INV
    assert L.oslam_volume_shift(C.byref(h2), s3(0, 0, -1), C.byref(res)) == INV
    assert tuple(res.offset) == (7, 7, 7) and tuple(h2.off) == ((1 << 20) - 8, 0, -(1 << 20))      # nothing changed
    assert L.oslam_volume_shift(C.byref(h2), s3(0, 0, 0), C.byref(res)) == 0 and tuple(res.offset) == tuple(h2.off)
    # the tap
    assert L.oslam_volume_window(None, ppf._p(off), ppf._p(org)) == L.oslam_volume_window(vol, None, ppf._p(org)) == INV
    assert L.oslam_volume_window(vol, ppf._p(off), None) == INV
    assert L.oslam_volume_window(C.byref(h2), ppf._p(off), ppf._p(org)) == 0
    assert tuple(off) == tuple(h2.off) and org.tobytes() == H.window_origin(ref.origin, tuple(h2.off), ref.voxel).tobytes()

    def leaving(vo=vol, s=s3(1, 0, 0), sp=ok, xyz=buf, nrm=buf, cap=4, n_out=C.byref(n)):
        return L.oslam_volume_leaving(vo, s, C.byref(sp) if sp is not None else None, ppf._p(xyz) if xyz is not None else None,
                                      ppf._p(nrm) if nrm is not None else None, cap, n_out, C.byref(sres))

    assert leaving(vo=None) == leaving(s=None) == leaving(n_out=None) == INV
    assert leaving(xyz=None) == leaving(nrm=None) == leaving(xyz=None, nrm=None, cap=4) == INV
    assert leaving(s=s3(0, big, 0)) == leaving(s=s3(-big, 0, 0)) == INV
    for mw in (0, 65536):
        assert leaving(sp=ppf.default_surface_params(min_weight=mw)) == INV


def test_follow_rejects_bad_arguments(built_lib, ppf):
    L = ppf.lib()
    INV = ppf.OSLAM_E_INVALID
    h = stand_in(ppf, default_volume())
    eye = np.eye(4, dtype=np.float32)
    s = np.zeros(3, np.int32)
    fp = ppf.FollowParams()
    assert L.oslam_follow_params_default(None, C.byref(fp)) == L.oslam_follow_params_default(C.byref(h), None) == INV
    assert L.oslam_follow_params_default(C.byref(h), C.byref(fp)) == 0
    assert L.oslam_volume_follow(None, ppf._p(eye), None, ppf._p(s)) == L.oslam_volume_follow(C.byref(h), None, None, ppf._p(s)) == INV
    assert L.oslam_volume_follow(C.byref(h), ppf._p(eye), None, None) == INV
    for field, bad in [("lookahead", -0.1), ("lookahead", float("nan")), ("lookahead", float("inf")), ("threshold", -1.0),
                       ("threshold", float("nan")), ("threshold", float("inf")), ("granule", 0), ("granule", 65), ("granule", -8)]:
        q = ppf.FollowParams.from_buffer_copy(fp)
        setattr(q, field, bad)
        assert lib_follow(ppf, h, eye, q) == (INV, (99, 99, 99)), (field, bad)
    for field, good in [("lookahead", 0.0), ("threshold", 0.0), ("granule", 1), ("granule", 64)]:
        q = ppf.FollowParams.from_buffer_copy(fp)
        setattr(q, field, good)
        assert lib_follow(ppf, h, eye, q)[0] == 0, (field, good)
    for T in (2.0 * eye, np.diag([1, 1, -1, 1]).astype(np.float32), np.full((4, 4), np.nan, np.float32)):
        assert lib_follow(ppf, h, T)[0] == INV


def test_follow_rule(built_lib, ppf):
    ref = default_volume()
    h = stand_in(ppf, ref)
    eye = np.eye(4, dtype=np.float32)
    assert lib_follow(ppf, h, eye) == (0, (0, 0, 0)) == (0, H.follow(ref, eye))      # the defaults: d = 0 at the identity
    # the threshold from both sides: 64 voxels of 0.02f along x.  d is formed in double from the float inputs
    voxel = float(F(0.02))
    at = eye.copy()
    at[0, 3] = F(64.0) * F(0.02)                                   # exact in float32: d_x = 64 exactly
    assert (float(at[0, 3]) - 0.0) / voxel == 64.0
    assert lib_follow(ppf, h, at) == (0, (0, 0, 0)) == (0, H.follow(ref, at))
    over = at.copy()
    over[0, 3] = np.nextafter(at[0, 3], F(2.0))
    assert lib_follow(ppf, h, over) == (0, (64, 0, 0)) == (0, H.follow(ref, over))
    under = at.copy()
    under[0, 3] = -np.nextafter(at[0, 3], F(0.0))
    under[1, 3] = F(0.11)
    assert lib_follow(ppf, h, under) == (0, (0, 0, 0)) == (0, H.follow(ref, under))
    over[1, 3] = F(0.11)                                           # one axis over: every axis moves, y by rint(5.5 / 8) * 8
    assert lib_follow(ppf, h, over) == (0, (64, 8, 0)) == (0, H.follow(ref, over))
    # rint is to nearest even.  A voxel of 1/16 keeps d exact: d_y = 4 of granule 8 is 0.5 -> 0, 12 is 1.5 -> 2
    exact = S.blank(64, 64, 64, voxel=0.0625, origin=(-2.0, -2.0, 0.0))
    he = stand_in(ppf, exact)
    assert lib_follow(ppf, he, eye) == (0, (0, 0, 0))
    for dy, want in ((4.0, 0), (12.0, 16), (-12.0, -16), (20.0, 16), (28.0, 32), (16.0, 16)):
        T = eye.copy()
        T[0, 3], T[1, 3] = F(-17.0) * F(0.0625), F(dy) * F(0.0625)
        assert lib_follow(ppf, he, T) == (0, (-16, want, 0)) == (0, H.follow(exact, T)), dy
    far = eye.copy()
    far[:3, 3] = [1.0e6, -1.0e6, 40.0]                             # clamped to +-n_a
    assert lib_follow(ppf, h, far) == (0, (256, -256, 256)) == (0, H.follow(ref, far))
    # the optical axis moves the look-ahead point: a quarter turn about y looks along +x
    turn = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], np.float32)
    assert lib_follow(ppf, h, turn) == (0, (128, 0, -128)) == (0, H.follow(ref, turn))
    # a shifted window follows from its own origin, and other parameters
    ref2 = H.shifted(S.blank(40, 72, 24, voxel=0.05, origin=(-1.0, -1.8, 0.0)), (8, -16, 0))
    h2 = stand_in(ppf, ref2, off=ref2.off)
    rng = np.random.default_rng(3)
    for _ in range(20):
        T = eye.copy()
        T[:3, 3] = rng.uniform(-1.5, 1.5, 3).astype(np.float32)
        fp = ppf.FollowParams(lookahead=0.6, threshold=float(rng.integers(0, 12)), granule=int(rng.integers(1, 9)))
        rc, s = lib_follow(ppf, h2, T, fp)
        assert rc == 0 and s == H.follow(ref2, T, fp.lookahead, fp.threshold, fp.granule), (T[:3, 3], s)


def test_python_surface(built_lib, ppf):
    with pytest.raises(ValueError):
        ppf._shift3((1, 2))
    assert ppf._shift3((1, -2, 3)).dtype == np.int32
    assert "oslam_volume_shift" in ppf._SIGNATURES and "oslam_volume_leaving" in ppf._SIGNATURES
