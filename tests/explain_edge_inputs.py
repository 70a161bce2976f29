"""Deterministic inputs at the edges of the explain kernels (k_explain_splat, k_explain_score, k_explain_claims): the
ragged images and clouds of tests/render_edge_inputs.py (splats clipped by every border and corner, models around the
workgroup size, up to 1024 hypotheses over three models) with observed images made for the classes: observed z exactly
Z_h +- tol_h and one ulp beyond on both sides, invalid pixels under the silhouette, an occluder; a hypothesis wholly
off-image, skipped hypotheses, a hypothesis the camera sees through everywhere (agree 0), one it agrees with everywhere
(through 0), equal conflict rates, and tiles 4, 7, 128 and automatic with a partial last tile.

Every builder returns a `case`: render_edge_inputs' (clouds, member, T, cam, w, h) with the explain parameters and the
observed image `img` (float32 metres, depth_scale 1).  tests/test_explain_edge_inputs.py asserts on the restatement
(tests/explain_ref.py), without a GPU, that the inputs reach the branches they are meant for; tests/test_gpu_explain.py
compares the device with the same answer.  numpy only; seeded."""
import numpy as np

import explain_ref as X
import render_edge_inputs as E

F = np.float32
FAR_SHARE = F(0.9)


def case(name, base, img=None, **params):
    """an explain case from a render case: the render's own parameters give way to explain's defaults, then `params`"""
    p = X.default_params()
    p.update({k: base["params"][k] for k in ("footprint", "max_splat", "keep_back")})
    p.update(params)
    c = dict(base, name=name, params=p)
    c["img"] = observed(c) if img is None else img
    return c


def solo(c):
    """[Z_h] of the case's hypotheses on the full image (zeros for a skipped one)"""
    p = c["params"]
    out = []
    for cloud, T in zip(E.hypotheses(c), c["T"]):
        if not T.any():
            out.append(np.zeros((c["h"], c["w"]), np.float32))
        else:
            out.append(X.solo_z(cloud, T, c["cam"], c["w"], c["h"], p["footprint"], p["max_splat"], p["keep_back"])[0])
    return out


def front(c):
    """(z, tol) of the nearest drawn surface over all hypotheses, 0 where nobody draws"""
    z = np.zeros((c["h"], c["w"]), np.float32)
    tol = np.zeros((c["h"], c["w"]), np.float32)
    for cloud, T, z_h in zip(E.hypotheses(c), c["T"], solo(c)):
        if not T.any():
            continue
        nearer = (z_h > 0) & ((z == 0) | (z_h < z))
        z = np.where(nearer, z_h, z)
        tol = np.where(nearer, X.view_ref.tolerance(c["params"]["depth_tol"], cloud[2]), tol).astype(np.float32)
    return z, tol


PATTERN = dict(invalid=(7, 3), occluder=(5, 1), behind_eq=(11, 2), behind_ulp=(13, 4), front_eq=(17, 6), front_ulp=(19, 8),
               nan=(29, 6))


def pattern(shape, key):
    m, r = PATTERN[key]
    return np.arange(shape[0] * shape[1]).reshape(shape) % m == r


def observed(c):
    """The nearest drawn surface where something is drawn and a far plane elsewhere; then by flat index (PATTERN) an
    occluder three tolerances in front, the surface exactly tol behind and one ulp beyond that, exactly tol in front and
    one ulp beyond that, and last an invalid pixel and NaN."""
    z, tol = front(c)
    on = z > 0
    img = np.where(on, z, FAR_SHARE * F(c["cam"]["z_max"])).astype(np.float32)
    sel = lambda k: on & pattern(img.shape, k)  # noqa: E731
    s = sel("occluder")
    img[s] = np.maximum(z[s] - F(3) * tol[s], F(c["cam"]["z_min"]))
    s = sel("behind_eq")
    img[s] = z[s] + tol[s]
    s = sel("behind_ulp")
    img[s] = np.nextafter(z[s] + tol[s], F(np.inf))
    s = sel("front_eq")
    img[s] = z[s] - tol[s]
    s = sel("front_ulp")
    img[s] = np.nextafter(z[s] - tol[s], F(0))
    img[pattern(img.shape, "invalid")] = 0.0
    img[pattern(img.shape, "nan")] = np.nan
    return img


def reference(c, taps=None):
    return X.explain(E.hypotheses(c), c["T"], c["img"], c["cam"], taps=taps, **c["params"])


def border_cases():
    b, idx = E.border_cases()
    return [case(x["name"], x, tile=t, min_tiles=1) for x, t in zip(b, (4, 7, 128, 0, 4, 7))], idx


def off_image_case():
    """X in the image, the same patch 50 units to the right (every point OUT, its sphere projects beyond the image: an
    empty rectangle), a skipped hypothesis between them, and the patch behind the far limit"""
    Xc, _ = E.tie_clouds()
    z = np.zeros((4, 4), np.float32)
    base = E.case("off image", [Xc], [0, 0, 0, 0], [E.eye(), z, E.eye((50.0, 0.0, 0.0)), E.eye((0.0, 0.0, 20.0))])
    return case(base["name"], base, tile=4, min_tiles=1)


def skipped_cases():
    t = {c["name"]: c for c in E.tie_cases()}
    Xc, _ = E.tie_clouds()
    return [case("skipped between", t["skipped between"], tile=4, min_tiles=1), case("all skipped", t["all skipped"]),
            case("one hypothesis", E.case("one", [Xc], [0], [E.eye()]), tile=4, min_tiles=1)]


def conflict_cases():
    """A 9 x 9 patch of points every second pixel (a closed silhouette at k = 2).  `see through`: the camera sees the
    far plane everywhere (agree 0, through > 0: no claims, explained 0).  `all agree`: the image is the patch's own z
    (through 0: conflict_q 0).  `equal rates`: two patches side by side, each with the same share of its pixels seen
    through: equal conflict_q, two hypotheses that never meet; and the first one again: its duplicate loses the tie."""
    patch = E.cloud([E.at_pixel(a, b, E.PLANE_Z) for b in range(6, 23, 2) for a in range(4, 13, 2)]) + (E.D_EDGE,)
    one = E.case("patch", [patch], [0], [E.eye()])
    far = np.full((E.H_IMG, E.W), FAR_SHARE * F(E.CAM["z_max"]), np.float32)
    out = [case("see through", one, img=far.copy(), tile=4, min_tiles=1)]
    c = case("all agree", one, tile=4, min_tiles=1)
    z, _ = front(c)
    c["img"] = np.where(z > 0, z, far).astype(np.float32)
    out.append(c)
    shift = 16.0 * E.PLANE_Z / E.CAM["fx"]              # 16 pixels to the right at the patch's depth
    two = E.case("equal rates", [patch], [0, 0, 0], [E.eye(), E.eye((shift, 0.0, 0.0)), E.eye()])
    c = case("equal rates", two, tile=4, min_tiles=1)
    zs = solo(c)
    img = np.where(zs[0] > 0, zs[0], np.where(zs[1] > 0, zs[1], far)).astype(np.float32)
    for z_h in zs[:2]:
        ys, xs = np.nonzero(z_h > 0)
        first = ys == ys.min()                          # the silhouette's first row is seen through, in both
        img[ys[first], xs[first]] = far[0, 0]
    c["img"] = img
    out.append(c)
    return out


def size_case(synth):
    return case("sizes 255 256 257", E.size_case(synth), tile=7, min_tiles=1)


def many_case(n_hyp, synth=None):
    """render_edge_inputs.many_case under one 128-pixel tile (83 x 61: a partial tile), so that the restatement's
    elimination stays quick at 1024 hypotheses"""
    return case("hypotheses %d" % n_hyp, E.many_case(n_hyp), tile=128, min_tiles=1, min_owned_share=0.0)


def identical_case(n_hyp):
    """n_hyp copies of one hypothesis: equal conflict rates, every tie to the lower index"""
    base = E.many_case(3)
    T = np.repeat(base["T"][:1], n_hyp, axis=0)
    c = case("identical %d" % n_hyp, dict(base, member=[0] * n_hyp, T=T), tile=128, min_tiles=1)
    return c


def identical_answer(n_hyp):
    """(kept, suppressed_by) known without running anything"""
    return [True] + [False] * (n_hyp - 1), [-1] + [0] * (n_hyp - 1)


def edge_cases(synth):
    b, _ = border_cases()
    return (b + [off_image_case()] + skipped_cases() + conflict_cases() + [size_case(synth)] +
            [many_case(n) for n in (255, 256, 257, 1024)])
