"""GPU: the colour volume (oslam_volume_integrate_colour, oslam_volume_colours, oslam_volume_paint_view, the shift of the
colours and the Python surface over them) against the numpy restatement of tests/colour_ref.py, bit for bit: colour words
are integers, and the float arithmetic of the reads is pinned.

Shapes: the 40 x 72 x 24 volume of tests/test_gpu_volume.py (its x tile is partial) under the ragged 333 x 251 camera, and
one 128^3 under 640 x 480.  The colour images are pseudo-random bytes (synth.SplitMix64) with holes on strides of 17, 19,
29 and 2, coprime to the strides 7, 5, 11, 3, 13 and 4 of the depth holes of test_gpu_volume.holed, so a word taken from a
wrong pixel or a wrong voxel changes bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as E  # noqa: E402
import colour_ref as CR  # noqa: E402
import edge_inputs  # noqa: E402
import test_gpu_volume as TV  # noqa: E402
import volume_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint32
BIG, RAGGED_VOL = TV.BIG, TV.RAGGED_VOL
COLOUR = {"128^3": dict(max_weight=2), "ragged": dict(max_weight=2, band=0.15)}        # band < mu = 0.25 on the ragged one


def colour_image(synth, h, w, seed):
    """(rgb uint8 [h, w, 3], valid bool [h, w])"""
    rgb = (synth.SplitMix64(seed).u64(3 * h * w) >> np.uint64(17)).astype(np.uint8).reshape(h, w, 3)
    valid = np.ones((h, w), bool)
    valid[2::17, 1::19] = False
    valid[::29, ::2] = False
    return rgb, valid


def random_words(synth, n, seed, unseen_share=0.2):
    """colour words over all 32 bits, [nz, ny, nx], a fifth of them with wc = 0 (and colour bits that must not show)"""
    nx, ny, nz = n
    rng = synth.SplitMix64(seed)
    words = (rng.u64(nx * ny * nz) >> np.uint64(13)).astype(U)
    words[rng.uniform(nx * ny * nz) < unseen_share] &= U(0xffffff)
    return words.reshape(nz, ny, nx)


def ref_volume(spec, colour):
    return CR.Volume(spec["nx"], spec["ny"], spec["nz"], spec["voxel"], spec["origin"], mu=spec["mu"], max_weight=spec["max_weight"],
                     colour_max_weight=colour.get("max_weight", CR.DEFAULT_MAX_WEIGHT), band=colour.get("band"))


def dev_volume(ppf, spec, colour, ref=None):
    """a coloured device volume, in the state of ref when one is given"""
    dev = ppf.Volume(**spec)
    dev.enable_colour(**colour)
    if ref is not None:
        dev.set_voxels(ref.q, ref.w)
        dev.set_colour_words(ref.c)
    return dev


def same_tsdf(dev, ref):
    q, w = dev.voxels()
    return q.tobytes() == ref.q.tobytes() and w.tobytes() == ref.w.tobytes()


def colour_diff(dev, ref):
    return np.flatnonzero((dev.colour_words() != ref.c).ravel())


@pytest.fixture(scope="module")
def stream(ppf, synth):
    """Seed 0 of tests/test_camera_host.py: three frames at 640x480 and at the ragged 333x251, each with a colour image"""
    world = E.make_world(synth, 0)
    traj = [T.astype(np.float32) for T in E.trajectory(synth, 0)[:3]]
    fcam = dict(E.CAM, depth_scale=1.0)
    rcam = edge_inputs.ragged_cam()
    imgs = [E.render(synth, world, T) for T in traj]
    rimgs = [E.render(synth, world, T, **edge_inputs.RAGGED) for T in traj]
    # (depth for z, camera of z, depth of the view that carries the colour or None when it is the same view, its camera)
    big = [(imgs[0], E.CAM, None, None), (TV.holed(imgs[1]), fcam, imgs[1], E.CAM), (imgs[2], E.CAM, None, None)]
    rag = [(rimgs[0], rcam, None, None), (TV.holed(rimgs[1]), dict(rcam, depth_scale=1.0), rimgs[1], rcam), (rimgs[2], rcam, None, None)]
    cols = {"128^3": [colour_image(synth, 480, 640, 900 + f) for f in range(3)],
            "ragged": [colour_image(synth, 251, 333, 910 + f) for f in range(3)]}
    return dict(traj=traj, frames={"128^3": big, "ragged": rag}, colours=cols, spec={"128^3": BIG, "ragged": RAGGED_VOL})


@pytest.fixture(scope="module")
def before(built_lib, ppf, stream):
    """what an uncoloured volume gives before any volume of the process has colour"""
    return uncoloured_results(ppf, stream)


def uncoloured_results(ppf, stream):
    vol = ppf.Volume(**RAGGED_VOL)
    out = []
    views = [TV.view_of(ppf, fr[0], fr[1]) for fr in stream["frames"]["ragged"][:2]]
    for f, v in enumerate(views):
        out.append(TV.plain(vol.integrate(v, stream["traj"][f])))
    out += [a.tobytes() for a in vol.voxels()]
    cam = edge_inputs.ragged_cam()
    rv, res = TV.raycast(vol, stream["traj"][1], cam, 333, 251)
    maps, z = ppf.view_maps(rv)
    out += [TV.plain(res), maps.tobytes(), z.tobytes(), rv.has_colour()]
    po, no, res = vol.surface()
    out += [po.tobytes(), no.tobytes(), TV.plain(res)]
    res = vol.shift((3, -8, 5))
    out += [TV.plain(res), res["launches"]] + [a.tobytes() for a in vol.voxels()]
    rv.close()
    for v in views:
        v.close()
    vol.close()
    return out


def make_views(ppf, stream, name, f):
    """-> (the view z comes from, the view colour comes from, the views to close)"""
    img, cam, cimg, ccam = stream["frames"][name][f]
    rgb, valid = stream["colours"][name][f]
    v = TV.view_of(ppf, img, cam)
    c = v if cimg is None else TV.view_of(ppf, cimg, ccam)
    assert not c.has_colour()
    c.set_colour(rgb, valid)
    assert c.has_colour() and c.colour().tobytes() == CR.pack(rgb, valid).tobytes()
    return v, c, [v] if c is v else [v, c]


@pytest.fixture(scope="module")
def fused(before, built_lib, ppf, stream):
    """the three frames of both cases fused with colour on the restatement, once: {name: (ref, [(updated, coloured)])}"""
    out = {}
    for name in ("128^3", "ragged"):
        ref = ref_volume(stream["spec"][name], COLOUR[name])
        counts = []
        for f in range(3):
            img, cam, _, _ = stream["frames"][name][f]
            counts.append(ref.integrate_colour(V.z_image(img, cam), CR.pack(*stream["colours"][name][f]), cam, stream["traj"][f]))
        out[name] = (ref, counts)
    return out


@pytest.mark.parametrize("name", ["128^3", "ragged"])
def test_colour_integration_equals_restatement(fused, built_lib, ppf, stream, name):
    ref, counts = fused[name]
    spec = stream["spec"][name]
    dev, plain_vol = dev_volume(ppf, spec, COLOUR[name]), ppf.Volume(**spec)
    assert not dev.colour_words().any()
    for run in range(2):
        for f in range(3):
            v, c, views = make_views(ppf, stream, name, f)
            res = dev.integrate(v, stream["traj"][f], colour=c)
            assert (res["updated"], res["coloured"]) == counts[f] and res["launches"] == 2, (f, res, counts[f])
            if run == 0:
                assert plain_vol.integrate(v, stream["traj"][f])["launches"] == 1
            for x in views:
                x.close()
        bad = colour_diff(dev, ref)
        wc = dev.colour_words() >> U(24)
        print("%s: %d of %d voxels coloured (restatement %s), %d colour words differ" % (name, int((wc > 0).sum()), wc.size, counts, bad.size))
        assert bad.size == 0, (name, bad[:8], dev.colour_words().ravel()[bad[:8]], ref.c.ravel()[bad[:8]])
        assert same_tsdf(dev, ref) and int(wc.max()) == 2 and (wc > 0).sum() > wc.size // 100      # saturated at max_weight
        # the TSDF words are the plain call's
        assert [a.tobytes() for a in dev.voxels()] == [a.tobytes() for a in plain_vol.voxels()]
        if run == 0:
            dev.reset()                                           # two runs from a reset volume give equal bits
            assert not dev.colour_words().any() and not dev.voxels()[1].any()
    plain_vol.close()
    dev.close()


def test_preset_weights_254_and_255(fused, built_lib, ppf, synth, stream):
    spec, name = RAGGED_VOL, "ragged"
    ref = ref_volume(spec, dict(max_weight=255))
    words = random_words(synth, ref.n, 31)
    pick = synth.SplitMix64(32).uniform(words.size).reshape(words.shape)
    words = np.where(pick < 0.4, (words & U(0xffffff)) | U(254) << U(24), np.where(pick < 0.8, words | U(255) << U(24), words)).astype(U)
    ref.c[:] = words
    dev = dev_volume(ppf, spec, dict(max_weight=255), ref)
    v, c, views = make_views(ppf, stream, name, 0)
    res = dev.integrate(v, stream["traj"][0], colour=c)
    want = ref.integrate_colour(V.z_image(*stream["frames"][name][0][:2]), CR.pack(*stream["colours"][name][0]), edge_inputs.ragged_cam(),
                                stream["traj"][0])
    bad = colour_diff(dev, ref)
    moved = int((ref.c != words).sum())
    print("preset weights: %d voxels coloured, %d words changed, %d differ" % (res["coloured"], moved, bad.size))
    assert (res["updated"], res["coloured"]) == want and bad.size == 0 and same_tsdf(dev, ref)
    touched = ref.c != words
    assert 0 < moved < res["coloured"]                            # at wc = 255 a pixel within 127 levels on all channels changes nothing
    assert set(np.unique(ref.c[touched & (words >> U(24) >= 254)] >> U(24))) == {255}
    # set_voxels does not touch the colours, reset zeroes them
    dev.set_voxels(np.zeros_like(ref.q), np.zeros_like(ref.w))
    assert colour_diff(dev, ref).size == 0
    for x in views:
        x.close()
    dev.close()


def test_refusals_change_nothing(fused, built_lib, ppf, stream):
    name, spec = "ragged", RAGGED_VOL
    ref, _ = fused[name]
    dev = dev_volume(ppf, spec, COLOUR[name], ref)
    v, c, views = make_views(ppf, stream, name, 0)
    img, cam = stream["frames"][name][0][:2]
    T = stream["traj"][0]
    other = TV.view_of(ppf, img, dict(cam, fx=np.float32(cam["fx"]) + np.float32(2.0 ** -15)))       # one ulp of fx away
    other.set_colour(*stream["colours"][name][0])
    bare = TV.view_of(ppf, img, cam)
    small = TV.view_of(ppf, np.ascontiguousarray(img[:-1]), cam)
    small.set_colour(stream["colours"][name][0][0][:-1], stream["colours"][name][0][1][:-1])
    plain_vol = ppf.Volume(**spec)
    for what, call in (("other intrinsics", lambda: dev.integrate(v, T, colour=other)), ("no colour", lambda: dev.integrate(v, T, colour=bare)),
                       ("another size", lambda: dev.integrate(v, T, colour=small)), ("enabled twice", lambda: dev.enable_colour()),
                       ("volume without colour", lambda: plain_vol.integrate(v, T, colour=c)),
                       ("colours without colour", lambda: plain_vol.colours(np.zeros((2, 3), np.float32))),
                       ("paint without colour", lambda: plain_vol.paint(v, T)), ("words without colour", lambda: plain_vol.colour_words()),
                       ("bad max_weight", lambda: plain_vol.enable_colour(max_weight=256)),
                       ("band above mu", lambda: plain_vol.enable_colour(band=0.26))):
        with pytest.raises(ppf.OslamError) as e:
            call()
        assert e.value.code == ppf.OSLAM_E_INVALID, what
        assert colour_diff(dev, ref).size == 0 and same_tsdf(dev, ref), what
        assert not plain_vol.voxels()[1].any(), what
    # after the refusals both still work
    plain_vol.enable_colour(band=0.25)
    assert plain_vol.integrate(v, T, colour=c)["coloured"] > 0
    rgb, valid = dev.colours(np.zeros((0, 3), np.float32))
    assert rgb.shape == (0, 3) and valid.shape == (0,)
    for x in views + [other, bare, small]:
        x.close()
    plain_vol.close()
    dev.close()


def point_list(synth, ref, surface):
    """every surface point; points on both sides of b_a = 0 and b_a = n_a - 2 of the trilinear read; points outside the
    volume on every face; NaN and infinite points; random points in and around the volume"""
    n = np.array(ref.n, np.float32)
    rng = synth.SplitMix64(55)
    lo, hi = ref.origin, ref.origin + n * ref.voxel
    inside = (lo + (rng.uniform(3 * 4000).reshape(-1, 3) * (n + 4.0) - 2.0) * float(ref.voxel)).astype(np.float32)
    edge = []
    for a in range(3):
        for at in (0.5, float(ref.n[a]) - 0.5, 0.0, float(ref.n[a]), 1.0, float(ref.n[a]) - 1.0):   # b_a = 0 | n_a - 2, the faces, a voxel in
            for eps in (-0.01, 0.0, 0.01):
                p = (lo + rng.uniform(3 * 40).reshape(-1, 3) * n * float(ref.voxel)).astype(np.float32)
                p[:, a] = lo[a] + np.float32(at + eps) * ref.voxel
                edge.append(p)
    odd = np.array([[np.nan, 0, 5], [0, np.inf, 5], [0, 0, -np.inf], [np.nan] * 3, [3e38, 3e38, 3e38], [-3e38, 0, 5],
                    list(lo), list(hi), [1e-45, 0, 5]], np.float32)            # the first six have no colour whatever the volume
    return np.concatenate([surface, inside] + edge + [odd]).astype(np.float32)


@pytest.mark.parametrize("name", ["128^3", "ragged"])
def test_colours_of_points(fused, built_lib, ppf, synth, stream, name):
    ref, _ = fused[name]
    spec = stream["spec"][name]
    dev = dev_volume(ppf, spec, COLOUR[name], ref)
    po, no, sres, srgb, svalid = dev.surface(colour=True)
    assert len(po) == sres["points"] > 0
    for state in ("fused", "random"):
        if state == "random":                                     # every bit pattern, corners partly uncoloured everywhere
            ref = ref_volume(spec, COLOUR[name])
            ref.c[:] = random_words(synth, ref.n, 77)
            dev.set_colour_words(ref.c)
        P = point_list(synth, ref, po)
        rgb, valid = dev.colours(P)
        want_rgb, want_valid = ref.colours(P)
        bad = np.flatnonzero((rgb != want_rgb).any(axis=1) | (valid != want_valid))
        print("%s, %s colours: %d points, %d with a colour (%d of the %d surface points), %d differ" % (
            name, state, len(P), int(valid.sum()), int(valid[:len(po)].sum()), len(po), bad.size))
        assert bad.size == 0, (name, state, bad[:8], P[bad[:8]], rgb[bad[:8]], want_rgb[bad[:8]])
        assert not rgb[~valid].any() and not valid[-9:-3].any() and 0 < valid.sum() < len(P)
        if state == "fused":
            # surface(colour=True) is colours() of its own points
            assert srgb.tobytes() == rgb[:len(po)].tobytes() and np.array_equal(svalid, valid[:len(po)])
            assert svalid.mean() > 0.5
    dev.close()


def test_mesh_colour_and_ply(fused, built_lib, ppf, stream, tmp_path):
    name = "128^3"
    ref, _ = fused[name]
    dev = dev_volume(ppf, stream["spec"][name], COLOUR[name], ref)
    xyz, nrm, tri, res, rgb, valid = dev.mesh(colour=True)
    xyz0, nrm0, tri0, res0 = dev.mesh()
    assert xyz.tobytes() == xyz0.tobytes() and tri.tobytes() == tri0.tobytes() and len(xyz) == res["vertices"] > 0
    want_rgb, want_valid = ref.colours(xyz)
    assert rgb.tobytes() == want_rgb.tobytes() and np.array_equal(valid, want_valid) and valid.mean() > 0.5
    r2, v2 = dev.colours(xyz)
    assert r2.tobytes() == rgb.tobytes() and np.array_equal(v2, valid)
    f = str(tmp_path / "coloured_mesh.ply")
    ppf.ply_write_mesh(f, xyz, nrm, tri, rgb=rgb)
    p2, n2, t2 = ppf.ply_read_mesh(f)
    assert p2.tobytes() == xyz.tobytes() and n2.tobytes() == nrm.tobytes() and t2.tobytes() == tri.tobytes()
    head = open(f, "rb").read(600).split(b"end_header")[0]
    assert b"property uchar red" in head and os.path.getsize(f) == len(head) + len(b"end_header\n") + 27 * len(xyz) + 13 * len(tri)
    dev.close()


@pytest.mark.parametrize("name", ["128^3", "ragged"])
def test_paint_equals_restatement(fused, built_lib, ppf, stream, name):
    ref, _ = fused[name]
    dev = dev_volume(ppf, stream["spec"][name], COLOUR[name], ref)
    img, cam, _, _ = stream["frames"][name][1]                    # the holed float frame
    h, w = img.shape
    T = stream["traj"][1]
    # a ray-cast view: the map's picture from that pose
    rv, rres = TV.raycast(dev, T, cam, w, h)
    assert not rv.has_colour()
    with pytest.raises(ppf.OslamError):
        rv.colour()
    _, z = ppf.view_maps(rv)
    painted = dev.paint(rv, T)
    got, want = rv.colour(), ref.paint(z, cam, T)
    print("%s: ray cast with %d hits, %d pixels painted" % (name, rres["hits"], painted))
    assert rv.has_colour() and got.tobytes() == want.tobytes(), np.flatnonzero((got != want).ravel())[:8]
    assert painted == int((want != 0).sum()) and set(np.unique(got >> U(24))) <= {0, 255} and not got[z <= 0].any()
    if name == "128^3":
        assert painted > rres["hits"] // 2
    # a holed depth view, from a pose that is not the frame's; a second paint replaces the image
    dv = TV.view_of(ppf, img, cam)
    zd = V.z_image(img, cam)
    for Tp in (stream["traj"][2], T):
        painted = dev.paint(dv, Tp)
        got, want = dv.colour(), ref.paint(zd, cam, Tp)
        assert got.tobytes() == want.tobytes() and painted == int((want != 0).sum()) > 0 and not got[zd <= 0].any()
    # set_colour replaces a painted image
    rgb, valid = stream["colours"][name][1]
    dv.set_colour(rgb, valid)
    assert dv.colour().tobytes() == CR.pack(rgb, valid).tobytes()
    rv.close()
    dv.close()
    dev.close()


def test_shift_moves_the_colours(fused, built_lib, ppf, stream):
    name, spec = "ragged", RAGGED_VOL
    ref, _ = fused[name]
    dev = dev_volume(ppf, spec, COLOUR[name], ref)
    cur = ref
    for s in ((3, -8, 5), (4, 0, 0), (0, 0, 0), (-7, 8, -5)):     # one word at a time, then whole quads: both load paths
        res = dev.shift(s)
        cur = CR.shifted(cur, s)
        bad = colour_diff(dev, cur)
        print("shift %s: kept %d, %d launches, %d colour words differ" % (s, res["kept"], res["launches"], bad.size))
        assert bad.size == 0 and same_tsdf(dev, cur), (s, bad[:8])
        assert res["launches"] == (2 if any(s) else 0) and res["offset"] == cur.off
        assert res["kept"] == (int((cur.w > 0).sum()) if any(s) else 0)
    assert (cur.c >> U(24) > 0).any()
    # integration goes on in the shifted window
    v, c, views = make_views(ppf, stream, name, 2)
    got = dev.integrate(v, stream["traj"][2], colour=c)
    want = cur.integrate_colour(V.z_image(*stream["frames"][name][2][:2]), CR.pack(*stream["colours"][name][2]),
                                stream["frames"][name][2][1], stream["traj"][2])
    assert (got["updated"], got["coloured"]) == want and colour_diff(dev, cur).size == 0 and same_tsdf(dev, cur)
    for x in views:
        x.close()
    dev.close()


def test_shift_through_the_store_returns_without_colour(fused, built_lib, ppf, stream):
    name, spec = "ragged", RAGGED_VOL
    ref, _ = fused[name]
    dev = dev_volume(ppf, spec, COLOUR[name], ref)
    world = ppf.World(dev)
    s = (8, -8, 8)
    out = dev.shift(s, world)
    there = CR.shifted(ref, s)
    assert colour_diff(dev, there).size == 0 and out["stored"] > 0
    back = dev.shift(tuple(-x for x in s), world)
    home = CR.shifted(there, tuple(-x for x in s))
    print("out: %s; back: %s" % (TV.plain(out), TV.plain(back)))
    assert back["reloaded"] == out["stored"] and same_tsdf(dev, ref)               # the TSDF came back whole
    got = dev.colour_words()
    assert got.tobytes() == home.c.tobytes()                      # the colours of what stayed; wc = 0 on what returned
    returned = (ref.w > 0) & (home.w == 0)
    assert returned.sum() == back["reloaded"] and not got[returned].any() and (ref.c[returned] >> U(24) > 0).any()
    # out: count and scan, emit, the two shifts; back: count and scan (nothing seen leaves), the two shifts, unpack
    assert out["launches"] == 5 and back["launches"] == 5
    world.close()
    dev.close()


def test_step_fuses_colour(fused, built_lib, ppf, stream):
    name = "128^3"
    dev = dev_volume(ppf, stream["spec"][name], COLOUR[name])
    steps = []
    ego = ppf.default_egomotion_params(min_overlap=0.0)           # every tracked frame counts as ok: the test is about what follows
    for f, kw in ((0, {}), (1, dict(smooth=ppf.default_bilateral_params())), (2, dict(follow=ppf.default_follow_params(dev)))):
        v, c, views = make_views(ppf, stream, name, f)
        dev.last_integrate = None
        T, res = dev.step(v, params=ego, colour=c, **kw)
        assert (res is None) == (f == 0) and (f == 0 or res["ok"] == 1), (f, res)
        steps.append(dev.last_integrate)
        assert dev.last_integrate["launches"] == 2 and dev.last_integrate["coloured"] > 0, (f, dev.last_integrate)
        for x in views:
            x.close()
    wc = dev.colour_words() >> U(24)
    print("three steps: %s, %d voxels coloured" % ([TV.plain(s) for s in steps], int((wc > 0).sum())))
    assert int(wc.max()) == 2
    # without colour= the step is what it was
    dev.reset()
    v = TV.view_of(ppf, *stream["frames"][name][0][:2])
    dev.step(v)
    assert dev.last_integrate["launches"] == 1 and "coloured" not in dev.last_integrate and not dev.colour_words().any()
    v.close()
    dev.close()


def test_an_uncoloured_volume_is_unchanged(before, fused, built_lib, ppf, stream):
    """after all of the above an uncoloured volume's integrate, raycast, surface and shift give what they gave before any
    volume of the process had colour"""
    dev = dev_volume(ppf, RAGGED_VOL, {})                         # a coloured volume lives while the plain one works
    after = uncoloured_results(ppf, stream)
    assert len(after) == len(before)
    for k, (a, b) in enumerate(zip(after, before)):
        assert a == b, k
    assert after[-3] == 1                                         # launches of the plain shift
    dev.close()
