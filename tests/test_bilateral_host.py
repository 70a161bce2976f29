"""CPU: the bilateral depth filter (include/oslam.h at oslam_view_bilateral) -- its weight table (tools/gen_gauss_table.py
against the committed header and the library's compiled-in copy), its defaults and argument checks through the C-ABI,
the properties of the restatement (tests/bilateral_ref.py) and the calibration of DESIGN.md 7s
(tests/bilateral_calib.py)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilateral_calib as BC  # noqa: E402
import bilateral_ref as B  # noqa: E402

F = np.float32
GT = B.GT
Z_MIN, Z_MAX = 0.5, 6.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------- the table
def test_library_table_equals_the_generator_and_the_header(built_lib, ppf):
    want = np.array(GT.table(), np.float32)
    assert len(want) == GT.N == ppf.GAUSS_TABLE_N == 288
    got = ppf.gauss_table()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(want), np.array(GT.bits(), np.uint32))
    header = open(os.path.join(os.path.dirname(ppf.LIB_PATH), "csrc", "oslam_gauss_table.h")).read()
    assert header == GT.header()                                     # the committed header is the generator's output
    L, w = ppf.lib(), C.c_float(0)
    assert L.oslam_gauss_table(288, C.byref(w)) == ppf.OSLAM_E_INVALID
    assert L.oslam_gauss_table(0, None) == ppf.OSLAM_E_INVALID


def test_table_is_a_decreasing_gaussian():
    g = np.array(GT.table(), np.float32)
    assert np.all(g[1:] < g[:-1]) and g[0] < 1 and g[-1] > 0
    for i, x in enumerate(g):
        exact = math.exp(-0.5 * (i + 0.5) / 32)
        assert abs(float(x) - exact) <= float(np.spacing(F(exact))), i
    # t < 9 is the cut and t * 32 the index: the largest float below 9 still lands in the last bin
    t = np.nextafter(F(9.0), F(0))
    assert int(t * F(32.0)) == 287


# ---------------------------------------------------------------- defaults and argument checks
def test_bilateral_params_default(built_lib, ppf):
    p, want = ppf.default_bilateral_params(), B.default_params()
    assert p.radius == want["radius"] == 6 and p.sigma_space == F(want["sigma_space"]) == F(4.5)
    assert p.sigma_depth == F(want["sigma_depth"]) == F(0.03) and list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_bilateral_params(radius=3).radius == 3 and ppf.BILATERAL_MAX_RADIUS == B.MAX_RADIUS == 8
    with pytest.raises(TypeError):
        ppf.default_bilateral_params(no_such_field=1)
    assert ppf.lib().oslam_bilateral_params_default(None) == ppf.OSLAM_E_INVALID
    for name in ("oslam_bilateral_params_default", "oslam_view_bilateral", "oslam_gauss_table"):
        assert name in ppf._SIGNATURES


def test_bilateral_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: the stand-in handle (zeroed host memory)
    is never looked at, on a machine with or without a GPU."""
    L = ppf.lib()
    buf = C.create_string_buffer(16384)
    v = C.cast(buf, C.c_void_p)
    res = ppf.BilateralResult()
    out = C.c_void_p(1)
    assert L.oslam_view_bilateral(None, None, C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    assert not out.value
    assert L.oslam_view_bilateral(v, None, None, C.byref(res)) == ppf.OSLAM_E_INVALID
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=0), dict(radius=9), dict(radius=1 << 31), dict(sigma_space=0.0), dict(sigma_space=-1.0),
                dict(sigma_space=nan), dict(sigma_space=inf), dict(sigma_space=-inf), dict(sigma_depth=0.0),
                dict(sigma_depth=-0.03), dict(sigma_depth=nan), dict(sigma_depth=inf), dict(sigma_depth=1e-30)):
        out = C.c_void_p(1)
        p = ppf.default_bilateral_params(**bad)
        assert L.oslam_view_bilateral(v, C.byref(p), C.byref(out), C.byref(res)) == ppf.OSLAM_E_INVALID, bad
        assert not out.value, bad
        assert L.oslam_view_bilateral(v, C.byref(p), C.byref(out), None) == ppf.OSLAM_E_INVALID, bad
    with pytest.raises(ppf.OslamError) as e:
        ppf._check(L.oslam_view_bilateral(v, C.byref(ppf.default_bilateral_params(radius=12)), C.byref(out), None))
    assert e.value.code == ppf.OSLAM_E_INVALID and "radius" in str(e.value)


# ---------------------------------------------------------------- the restatement's properties
def test_constant_and_two_level_images_are_fixed_points():
    for R in (1, 6, 8):
        z = np.full((13, 21), 2.5, np.float32)
        out, valid, taps = B.bilateral(z, Z_MIN, Z_MAX, radius=R)
        assert np.array_equal(bits(out), bits(z)) and valid == z.size
        # every pixel of the clipped window takes part
        n = sum(min(x + R, 20) - max(x - R, 0) + 1 for x in range(21)) * sum(min(y + R, 12) - max(y - R, 0) + 1 for y in range(13))
        assert taps == n
        # a step above 3 sigma_depth: the two sides do not see each other
        z2 = z.copy()
        z2[:, :10], z2[:, 10:] = 2.0, 2.1
        out2, valid2, taps2 = B.bilateral(z2, Z_MIN, Z_MAX, radius=R)
        assert np.array_equal(bits(out2), bits(z2)) and valid2 == z.size and taps2 < taps


def test_holes_stay_holes_and_nothing_else_becomes_one():
    rng = np.random.default_rng(5)
    z = (2.0 + 0.02 * rng.standard_normal((40, 50))).astype(np.float32)
    z[rng.uniform(size=z.shape) < 0.3] = 0
    out, valid, taps = B.bilateral(z, Z_MIN, Z_MAX)
    assert np.array_equal(out == 0, z == 0) and valid == int((z > 0).sum())
    assert np.all(out[z > 0] >= F(Z_MIN)) and np.all(out[z > 0] <= F(Z_MAX))
    assert taps >= valid                                             # the centre always takes part
    # the noise shrinks
    assert out[z > 0].std() < 0.5 * z[z > 0].std()
    # all invalid: nothing at all
    out0, valid0, taps0 = B.bilateral(np.zeros((7, 9), np.float32), Z_MIN, Z_MAX)
    assert not out0.any() and valid0 == 0 and taps0 == 0


def test_a_lone_pixel_and_the_clamp():
    z = np.zeros((9, 9), np.float32)
    z[4, 4] = F(3.3)
    out, valid, taps = B.bilateral(z, Z_MIN, Z_MAX)
    assert np.array_equal(bits(out), bits(z)) and (valid, taps) == (1, 1)
    # a pixel at z_min among higher neighbours is pulled up, one at z_max among lower ones down: both stay in range; a
    # mean that leaves the range is clamped (a view never holds such z, the restatement is handed it directly)
    lo = np.full((5, 5), 0.51, np.float32)
    lo[2, 2] = F(Z_MIN)
    hi = np.full((5, 5), 5.99, np.float32)
    hi[2, 2] = F(Z_MAX)
    a, b = B.bilateral(lo, Z_MIN, Z_MAX, radius=2)[0], B.bilateral(hi, Z_MIN, Z_MAX, radius=2)[0]
    assert F(Z_MIN) < a[2, 2] < F(0.51) and F(5.99) < b[2, 2] < F(Z_MAX)
    below = np.full((5, 5), 0.49, np.float32)
    below[2, 2] = F(0.5)
    above = np.full((5, 5), 6.01, np.float32)
    above[2, 2] = F(6.0)
    assert B.bilateral(below, Z_MIN, Z_MAX, radius=2)[0][2, 2] == F(Z_MIN)
    assert B.bilateral(above, Z_MIN, Z_MAX, radius=2)[0][2, 2] == F(Z_MAX)


def exact_gate_image():
    """9 x 9 of 2.0 with 2.25 at (dx, dy) = (2, 2) and (1, 0) from the centre; with sigma_space 1 and sigma_depth 0.25 the
    first has t == 9.0f exactly (excluded), the second t == 2.0f (included)."""
    z = np.full((9, 9), 2.0, np.float32)
    z[4 + 2, 4 + 2] = 2.25
    z[4 + 0, 4 + 1] = 2.25
    return z, dict(radius=3, sigma_space=1.0, sigma_depth=0.25)


def test_the_exact_gate():
    z, kw = exact_gate_image()
    inv_s, inv_r = B.constants(kw["sigma_space"], kw["sigma_depth"])
    assert inv_s == F(1.0) and inv_r == F(16.0)
    d = F(2.25) - F(2.0)
    assert F(8) * inv_s + (d * d) * inv_r == F(9.0) and F(1) * inv_s + (d * d) * inv_r == F(2.0)
    # the centre by hand: the 7 x 7 window in row-major order; every 2.0 within dx^2 + dy^2 < 9 takes part with d = 0
    g = [F(x) for x in GT.table()]
    sd, sw, taps = F(0), F(0), 0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            zz = F(z[4 + dy, 4 + dx])
            dd = zz - F(2.0)
            t = F(dx * dx + dy * dy) * inv_s + (dd * dd) * inv_r
            if zz > 0 and t < F(9.0):
                w = g[int(t * F(32.0))]
                sd = F(sd + F(w * dd))
                sw = F(sw + w)
                taps += 1
    assert taps == 24                    # 25 lattice points with dx^2 + dy^2 < 9, less (2, 2), whose depth term lifts it to 9
    centre = F(F(2.0) + F(sd / sw))
    assert word(centre) == 0x4000FEE1, hex(word(centre))
    out, valid, _ = B.bilateral(z, Z_MIN, Z_MAX, **kw)
    assert word(out[4, 4]) == 0x4000FEE1 and valid == 81
    # with (2, 2) a hair closer in depth it takes part
    z2 = z.copy()
    z2[6, 6] = np.nextafter(F(2.25), F(0))
    assert B.bilateral(z2, Z_MIN, Z_MAX, **kw)[0][4, 4] > out[4, 4]


# ---------------------------------------------------------------- the calibration
def test_filter_halves_the_normal_error_and_keeps_clean_depth(pkg):
    rows = BC.normals_table()
    print(BC.fmt_normals(rows))
    clean, half = rows[0], rows[1]
    assert clean["noise"] == 0.0 and half["noise"] == 0.5
    assert half["filtered"][0] < 0.5 * half["raw"][0], half
    assert clean["rms"] < 0.25 * B.default_params()["sigma_depth"], clean


def test_filter_keeps_the_camera_tracker_on_a_noisy_stream(pkg):
    rows = BC.motion_table()
    print(BC.fmt_motion(rows))
    six = [r for r in rows if r["sigma_mm"] == 6.0][0]
    for p in six["raw"]:
        assert not p["ok"], six
    for p in six["filtered"]:
        assert p["ok"] and p["trans"] < 0.005, six
