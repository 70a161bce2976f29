"""The named inputs of the segments stage's tests (tests/test_segments_host.py, tests/test_gpu_segments.py): depth
images at the smallest sizes at which each kernel can still go wrong (one tile, exactly two, ragged tiles in both
directions, components that cross every seam, merges against index order, ties, the cap, the limit, gates that hold or
miss by one ulp), a view with its planes, and three frames of the calibration room.

A case is dict(name, depth, cam, max_jump, params, planes): depth uint16 (millimetres) or float32 (metres), cam a dict
with fx fy cx cy depth_scale z_min z_max, params the fields of oslam_segments_params that differ from the defaults,
planes None or the fields of oslam_planes_params under which the view's planes are found first and handed over.
"""
import functools

import numpy as np

import camera_ref as E
import planes_inputs as PI
import segments_ref as SR

F = np.float32
MAX_JUMP = 0.08                 # the stream camera's: the default gate
Z0 = 2.0


def _case(name, z, cam=None, max_jump=MAX_JUMP, planes=None, **params):
    z = np.ascontiguousarray(z)
    h, w = z.shape
    if cam is None:
        cam = PI.camera(w, h, depth_scale=1.0 if z.dtype == np.float32 else 0.001)
    return dict(name=name, depth=z, cam=cam, max_jump=max_jump, params=params, planes=planes)


def of_mask(mask, z=Z0):
    return np.where(mask, F(z), F(0)).astype(np.float32)


def patchwork(w, h, seed, kind="f32"):
    """Cells of 3 x 3 pixels at one of three depths half a metre apart, a tenth of the pixels missing: many components of
    many sizes, at any image size."""
    rng = np.random.default_rng(seed)
    lev = rng.integers(0, 3, size=((h + 2) // 3, (w + 2) // 3))
    z = 1.0 + 0.5 * np.kron(lev, np.ones((3, 3)))[:h, :w]
    z[rng.uniform(size=z.shape) < 0.1] = 0.0
    return PI.as_image(z, kind)


def serpentine(w=130, h=67):
    """One pixel wide: the even rows whole, joined alternately at the right and the left end.  Its root is pixel 0, its far
    end lies in the last tile, and it crosses every seam many times."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for y in range(1, h, 2):
        m[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    return of_mask(m)


def comb(w=97, h=70):
    """Teeth in every other column that join only through a spine in the last row: the local roots of the upper tiles
    merge through the bottom tiles, against index order."""
    m = np.zeros((h, w), bool)
    m[:, 0::2] = True
    m[h - 1] = True
    return of_mask(m)


def _spiral(w, h, off, pitch=4):
    m = np.zeros((h, w), bool)
    l, t, r, b = off, off, w - 1 - off, h - 1 - off
    x0 = l
    while r > l and b > t:
        m[t, x0:r + 1] = True
        m[t:b + 1, r] = True
        m[b, l:r + 1] = True
        m[t + pitch:b + 1, l] = True
        x0 = l
        l, t, r, b = l + pitch, t + pitch, r - pitch, b - pitch
    return m


def spirals(w=65, h=33):
    """Two interleaved rectangular spirals at the same depth, a pixel apart everywhere."""
    a, b = _spiral(w, h, 0), _spiral(w, h, 2)
    assert not (a & b).any()
    return of_mask(a | b)


def ring_and_island(w=40, h=36):
    """A ring along the image border, touching all four sides, around an island that touches none."""
    m = np.zeros((h, w), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    m[10:20, 12:30] = True
    return of_mask(m)


def diagonal_blobs(w=65, h=40):
    """Squares that meet only at a corner: at the corner of four tiles (31, 31 | 32, 32) and inside a tile."""
    m = np.zeros((h, w), bool)
    m[28:32, 28:32] = True
    m[32:36, 32:36] = True
    m[7:11, 7:11] = True
    m[11:15, 11:15] = True
    m[11:15, 3:7] = True                            # the other diagonal
    return of_mask(m)


def checkerboard(w, h):
    v, u = np.mgrid[0:h, 0:w]
    return of_mask((u + v) % 2 == 0)


STEP = 0.0625                   # 2^-4: exact, and so is every difference below


def steps(transposed=False):
    """Four pairs of runs along x, each from 2.0 to 2.0 + STEP (exactly the gate: joined) or to the next float32 above
    (one ulp of z more: cut), the boundary inside a tile (9|10, 19|20) or on a seam (31|32, 63|64); zeros between the
    pairs.  za - zb is exact in float32 for every pair.  With rel_step 2^-6 and max_step 2^-5 the gate at min(za, zb) =
    2.0 is the same 2^-4."""
    up = F(Z0 + STEP)
    up1 = np.nextafter(up, F(np.inf))
    assert F(up - F(Z0)) == F(STEP) and F(up1 - F(Z0)) > F(STEP) and float(up1) - Z0 == float(F(up1 - F(Z0)))
    row = np.zeros(70, np.float32)
    row[0:10], row[10:15] = Z0, up                  # inside a tile, joined
    row[16:20], row[20:25] = Z0, up1                # inside a tile, cut
    row[26:32], row[32:37] = Z0, up                 # on the seam, joined
    row[38:64], row[64:70] = Z0, up1                # on the seam, cut
    z = np.repeat(row[None, :], 5, axis=0)
    return np.ascontiguousarray(z.T) if transposed else z


@functools.lru_cache(maxsize=None)
def fma_pair(max_step=0.05, rel_step=0.01):
    """(za, zb) for which the gate's two roundings and a fused multiply-add decide differently: found by a seeded search,
    checked in exact arithmetic."""
    ms, rs = F(max_step), F(rel_step)
    rng = np.random.default_rng(3)
    for _ in range(200000):
        za = F(rng.uniform(1.0, 4.0))
        two = F(ms + F(rs * za))
        one = F(float(ms) + float(rs) * float(za))  # the product is exact in double; the sum of two floats 2^-5 apart too
        if two == one:
            continue
        zb = F(za + max(two, one))
        d = F(zb - za)
        if min(two, one) < d <= max(two, one) and zb > za:
            return float(za), float(zb)
    raise AssertionError("no pair found")


def fma_image():
    za, zb = fma_pair()
    z = np.zeros((5, 40), np.float32)
    z[:, 4:12], z[:, 12:20] = za, zb                # inside a tile
    z[:, 26:32], z[:, 32:38] = za, zb               # on the seam
    return z


def split_by_holes(w=37, h=21):
    z = np.full((h, w), Z0, np.float32)
    z[:, 17] = 0                                    # a column of holes cuts the blob in two
    z[5, 3] = 0
    return z


def two_equal(w=33, h=9):
    m = np.zeros((h, w), bool)
    m[1:4, 20:23] = True                            # the lower root, further right
    m[5:8, 2:5] = True
    return of_mask(m)


def exact_and_short(w=33, h=9):
    m = np.zeros((h, w), bool)
    m[1:4, 2:5] = True                              # 9 pixels
    m[5:8, 10:13] = True
    m[5, 10] = False                                # 8 pixels
    return of_mask(m)


def far_off_axis():
    """Points at 9 m under a camera with a focal length of a thousandth of a pixel: p_x * 8192 passes 2^30 from 15
    pixels off the axis on (|p_x| > 131072 m), so those pixels stay out of the centroid."""
    w, h = 40, 5
    cam = dict(fx=0.001, fy=0.001, cx=0.0, cy=2.0, depth_scale=1.0, z_min=0.1, z_max=20.0)
    return np.full((h, w), 9.0, np.float32), cam


def small_cases():
    out = []
    for k, (w, h) in enumerate(((1, 1), (3, 3), (7, 5), (40, 1), (1, 40), (33, 9), (64, 32), (65, 33), (97, 70), (130, 67))):
        for kind in ("f32", "u16"):
            out.append(_case("patchwork_%dx%d_%s" % (w, h, kind), patchwork(w, h, 10 + k, kind), min_pixels=2))
    out.append(_case("patchwork_cap_65x33", patchwork(65, 33, 17), min_pixels=1, max_segments=2))
    out.append(_case("patchwork_max64_97x70", patchwork(97, 70, 18), min_pixels=1, max_segments=64))
    out.append(_case("full_97x70", np.full((70, 97), Z0, np.float32)))
    out.append(_case("serpentine_130x67", serpentine()))
    out.append(_case("comb_97x70", comb()))
    out.append(_case("spirals_65x33", spirals()))
    out.append(_case("ring_and_island_40x36", ring_and_island()))
    out.append(_case("diagonal_blobs_65x40", diagonal_blobs(), min_pixels=1))
    out.append(_case("checkerboard_64x32", checkerboard(64, 32), min_pixels=1, max_segments=64))
    out.append(_case("checkerboard_limit_130x67", checkerboard(130, 67), min_pixels=1))
    for t in (False, True):
        sfx = "_y" if t else "_x"
        out.append(_case("steps_exact" + sfx, steps(t), min_pixels=1, max_step=STEP))
        out.append(_case("steps_rel" + sfx, steps(t), min_pixels=1, max_step=STEP / 2, rel_step=1.0 / 64))
    out.append(_case("fma_pair_40x5", fma_image(), min_pixels=1, max_step=0.05, rel_step=0.01))
    out.append(_case("split_by_holes_37x21", split_by_holes()))
    out.append(_case("two_equal_33x9", two_equal(), min_pixels=1))
    out.append(_case("exact_and_short_33x9", exact_and_short(), min_pixels=9))
    z, cam = far_off_axis()
    out.append(_case("far_off_axis_40x5", z, cam=cam, max_jump=0.5))
    img, cam = PI.room_corner(37, 21, "f32")
    out.append(_case("room_corner_planes_37x21", img, cam=cam, max_jump=PI.MAX_JUMP, planes=dict(min_pixels=12), min_pixels=2))
    img, cam = PI.room_corner(64, 16, "u16")
    out.append(_case("room_corner_planes_64x16", img, cam=cam, max_jump=PI.MAX_JUMP, planes=dict(min_pixels=12), min_pixels=2))
    return out


ROOM_NAMES = ["room_f0_320x240", "room_f5_320x240", "room_f0_640x480"]


def room_cases(synth):
    """planes_inputs' three room frames, each with its planes (defaults)."""
    return [dict(c, planes={}) for c in PI.room_cases(synth)]


def view_of(ppf, case):
    return PI.view_of(ppf, case)


def restate(case, trace=None):
    """The restatement on a case: the planes first where the case has them -> (result, z, plane labels or None)."""
    import planes_ref as PR
    lab = None
    if case["planes"] is not None:
        lab = PR.find_in_depth(case["depth"], case["cam"], case["max_jump"], **case["planes"])[0]["labels"]
    res, z = SR.find_in_depth(case["depth"], case["cam"], case["max_jump"], plane_labels=lab, trace=trace, **case["params"])
    return res, z, lab


def edges_of(case):
    """(n pixels, a, b): the joined pairs of a case, for tests/native/seg_union_check.c."""
    res, z, lab = restate(case)
    inn = z > 0
    if lab is not None:
        inn &= lab < 0
    step = case["params"].get("max_step", 0.0) or case["max_jump"]
    a, b = SR.edge_list(z, inn, step, case["params"].get("rel_step", 0.0))
    return z.size, a, b, res["roots"]


E_MAX_JUMP = E.MAX_JUMP
