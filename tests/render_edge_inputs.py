"""Deterministic inputs at the edges of the render kernels (k_render_splat, k_render_resolve, k_view_mask): a ragged
image, splats clipped by every border and corner, centres one pixel outside, p'z on and one ulp outside the z range,
half-widths 0 and capped, bit-equal depths of two hypotheses in both orders, a skipped hypothesis, models around the
workgroup size, 1024 hypotheses, and for the mask the tolerance to the ulp, occluders, invalid pixels and windows clipped
by the border.

Every builder returns its inputs in one shape (`case`): the distinct clouds, the hypotheses as indices into them with
their poses, the camera, the size and the render parameters.  tests/test_render_edge_inputs.py asserts on the
restatement (tests/render_ref.py), on a machine without a GPU, that the inputs reach the branches they are meant for;
tests/test_gpu_render.py compares the device with the same answer.  numpy only; seeded (synth.SplitMix64)."""
import numpy as np

import render_ref as R

F = np.float32
W, H_IMG = 37, 29                       # neither a multiple of 32 nor of 8
CAM = dict(fx=40.0, fy=41.0, cx=17.25, cy=13.5, depth_scale=1.0, z_min=0.5, z_max=8.0)
PLANE_Z = 2.0
D_EDGE = 0.125                          # tol = 0.125 exactly at depth_tol 1; rho = 0.09375: k = 2 at z = 2 under CAM
TOWARDS = (0.0, 0.0, -1.0)              # a normal that faces the camera


def at_pixel(a, b, z, cam=CAM):
    """the camera-frame point whose centre pixel is (a, b) at depth z"""
    return [(a - cam["cx"]) * z / cam["fx"], (b - cam["cy"]) * z / cam["fy"], z]


def cloud(pts, nrm=None):
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = np.tile(F(TOWARDS), (len(p), 1)) if nrm is None else np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
    return p, n


def eye(t=(0.0, 0.0, 0.0)):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = t
    return T


def case(name, clouds, member, T, cam=CAM, w=W, h=H_IMG, **params):
    p = R.default_params()
    p.update(params)
    T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(len(member), 4, 4))
    return dict(name=name, clouds=clouds, member=list(member), T=T, cam=cam, w=w, h=h, params=p)


def hypotheses(c):
    """the case's hypotheses as render_ref takes them"""
    return [c["clouds"][m] for m in c["member"]]


def reference(c):
    p = c["params"]
    return R.render(hypotheses(c), c["T"], c["cam"], c["w"], c["h"], p["footprint"], p["max_splat"], p["depth_tol"],
                    p["keep_back"])


# ---------------------------------------------------------------- one hypothesis at the borders and the z limits
BORDER_PIXELS = [(0, 14), (W - 1, 14), (18, 0), (18, H_IMG - 1), (0, 0), (W - 1, 0), (0, H_IMG - 1), (W - 1, H_IMG - 1)]
OUTSIDE_PIXELS = [(-1, 7), (W, 7), (9, -1), (9, H_IMG), (-1, -1), (W, H_IMG)]
Z_MIN, Z_MAX = F(CAM["z_min"]), F(CAM["z_max"])
BELOW, ABOVE = np.nextafter(Z_MIN, F(0)), np.nextafter(Z_MAX, F(np.inf))


def border_cloud():
    """-> (cloud, index dict): points on the four borders and in the four corners, points whose centre is one pixel
    outside, p'z on and one ulp outside both limits, two points of one pixel, a point that faces away"""
    pts, nrm, idx = [], [], {}

    def add(key, p, n=TOWARDS):
        idx.setdefault(key, []).append(len(pts))
        pts.append(p)
        nrm.append(n)
    for a, b in BORDER_PIXELS:
        add("border", at_pixel(a, b, PLANE_Z))
    for a, b in OUTSIDE_PIXELS:
        add("outside", at_pixel(a, b, PLANE_Z))
    add("z_min", at_pixel(10, 20, float(Z_MIN)))        # k = 7.5 + 0.5 -> 8: the cap, reached from below
    add("z_max", at_pixel(30, 8, float(Z_MAX)))         # k = 0: one pixel
    add("below", at_pixel(30, 20, float(BELOW)))
    add("above", at_pixel(5, 5, float(ABOVE)))
    add("pair", at_pixel(24, 14, 3.0))
    add("pair", at_pixel(24, 14, 2.5))
    add("back", at_pixel(12, 6, 4.0), (0.0, 0.0, 1.0))
    p, n = cloud(pts, nrm)
    # the limits exactly: the float32 rounding of at_pixel's z is the limit itself
    for key, z in (("z_min", Z_MIN), ("z_max", Z_MAX), ("below", BELOW), ("above", ABOVE)):
        p[idx[key][0], 2] = z
    return (p, n, D_EDGE), idx


def border_cases():
    c, idx = border_cloud()
    near = cloud([at_pixel(20, 12, 0.6), at_pixel(3, 25, 0.6)]) + (0.4,)       # kf = 20: capped
    out = []
    for name, kw in (("default", {}), ("max_splat 0", dict(max_splat=0)), ("max_splat 3", dict(max_splat=3)),
                     ("keep_back", dict(keep_back=1)), ("footprint 3", dict(footprint=3.0))):
        out.append(case("border " + name, [c], [0], [eye()], **kw))
    out.append(case("near capped", [near], [0], [eye()]))
    return out, idx


# ---------------------------------------------------------------- ties, order, a skipped hypothesis
def tie_clouds():
    """X: a 3 x 3 patch of points at PLANE_Z; Y: the patch's first point again (bit-equal p'z on its pixels) and a
    point in front of the patch's last one, its splat clear of the first's"""
    X = cloud([at_pixel(a, b, PLANE_Z) for b in (10, 13, 16) for a in (10, 13, 16)])
    Y = cloud([at_pixel(10, 10, PLANE_Z), at_pixel(16, 16, 1.9)])
    return X + (D_EDGE,), Y + (D_EDGE,)


def tie_cases():
    X, Y = tie_clouds()
    z = np.zeros((4, 4), np.float32)
    return [case("tie X Y", [X, Y], [0, 1], [eye(), eye()]), case("tie Y X", [X, Y], [1, 0], [eye(), eye()]),
            case("skipped between", [X, Y], [0, 1, 1], [eye(), z, eye()]),
            case("all skipped", [X, Y], [0, 1], [z, z])]


# ---------------------------------------------------------------- the workgroup edge and many hypotheses
SIZE_W, SIZE_H = 83, 61
SIZE_CAM = dict(fx=75.0, fy=77.0, cx=40.3, cy=31.7, depth_scale=1.0, z_min=0.5, z_max=8.0)


def size_case(synth):
    """models of 255, 256 and 257 points in one call: one and two workgroups per hypothesis in one grid"""
    mp, mn = synth.make_model(0, 257)
    mp = np.ascontiguousarray(mp * F(0.12))
    d = synth.d_dist_for(mp, 0.05)
    rng = synth.SplitMix64(99)
    clouds, T = [], []
    for k, n in enumerate((255, 256, 257)):
        clouds.append((mp[:n].copy(), mn[:n].copy(), d))
        Tk = np.eye(4)
        Tk[:3, :3] = synth.random_rotation(rng)
        Tk[:3, 3] = [(-0.45, 0.0, 0.4)[k], (0.1, -0.1, 0.05)[k], (1.6, 1.9, 1.7)[k]]
        T.append(Tk.astype(np.float32))
    return case("sizes 255 256 257", clouds, [0, 1, 2], T, cam=SIZE_CAM, w=SIZE_W, h=SIZE_H)


def many_case(n_hyp=1024):
    """n_hyp hypotheses of three two-point models on a lattice of translations that overlap: every seventeenth one is
    skipped, and neighbours at the same depth tie"""
    clouds = [cloud([[0.0, 0.0, 0.0], [0.02 * (k + 1), 0.01, 0.03 * k]]) + (0.05 + 0.02 * k,) for k in range(3)]
    member, T = [], []
    for i in range(n_hyp):
        member.append(i % 3)
        if i % 17 == 5:
            T.append(np.zeros((4, 4), np.float32))
            continue
        a, b = (i * 7) % SIZE_W, (i * 3) % SIZE_H
        z = 1.5 + 0.25 * (i % 4)                       # four depths: many bit-equal keys apart from the index
        T.append(eye(at_pixel(a, b, z, SIZE_CAM)))
    return case("hypotheses %d" % n_hyp, clouds, member, T, cam=SIZE_CAM, w=SIZE_W, h=SIZE_H)


def render_cases(synth):
    b, _ = border_cases()
    return b + tie_cases() + [size_case(synth), many_case()]


# ---------------------------------------------------------------- observed images for the mask
def observed(c, ref):
    """A float32 depth image (metres, depth_scale 1) for the case's camera: the render itself where something is drawn
    and a far plane elsewhere, the object one pixel wider to the right than the render, then by flat index an invalid pixel, an occluder nearer than z_r - tol, a pixel exactly
    tol behind z_r and one an ulp beyond that, and NaN."""
    z_r, lab = ref["z"], ref["labels"]
    far = F(0.9) * F(c["cam"]["z_max"])
    img = np.where(lab >= 0, z_r, far).astype(np.float32)
    tol = np.where(lab >= 0, ref["tol"][np.clip(lab, 0, None)], F(0)).astype(np.float32)
    idx = np.arange(img.size).reshape(img.shape)
    on = lab >= 0
    ring = ~on & np.roll(on, 1, axis=1)                 # right of a labelled pixel: the object seen one pixel wider
    ring[:, 0] = False
    img[ring] = np.roll(z_r, 1, axis=1)[ring]
    img[idx % 7 == 3] = 0.0
    occ = on & (idx % 5 == 1)
    img[occ] = np.maximum(z_r[occ] - F(3) * tol[occ], F(c["cam"]["z_min"]))
    edge = on & (idx % 11 == 2)
    img[edge] = z_r[edge] + tol[edge]
    beyond = on & (idx % 13 == 4)
    img[beyond] = np.nextafter(z_r[beyond] + tol[beyond], F(np.inf))
    img.reshape(-1)[idx.reshape(-1) % 29 == 6] = np.nan
    return img


MASK_SETTINGS = [dict(mode=m, dilate=d, only=-1) for m in (R.REMOVE, R.KEEP) for d in (0, 2, 8)]


def mask_case():
    """By hand: a patch of the rendered object in the image's corner (labels touch two borders), a second hypothesis
    hidden behind it that owns no pixel, and an observed image whose pixels are named."""
    front = cloud([at_pixel(a, b, PLANE_Z) for b in range(0, 9, 2) for a in range(0, 11, 2)]) + (D_EDGE,)
    hidden = cloud([at_pixel(a, b, 3.0) for b in (2, 4) for a in (2, 4, 6)]) + (D_EDGE,)
    c = case("mask corner", [front, hidden], [0, 1], [eye(), eye()], max_splat=1)
    ref = reference(c)
    tol = F(D_EDGE)
    img = np.full((H_IMG, W), F(5.0), np.float32)
    img[:14, :16] = F(PLANE_Z)                         # the observed object is larger than the render: dilate matters
    names = dict(exact=(3, 4), beyond=(3, 6), occluder=(5, 4), invalid=(5, 6))      # (row, column), all labelled
    img[names["exact"]] = F(PLANE_Z) + tol
    img[names["beyond"]] = np.nextafter(F(PLANE_Z) + tol, F(np.inf))
    img[names["occluder"]] = F(1.0)
    img[names["invalid"]] = F(0.0)
    return c, ref, img, names
