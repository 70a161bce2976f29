"""CPU: the conditions on the inputs of tests/fusion_edge_inputs.py, asserted on the numpy restatements alone
(camera_ref, volume_ref and its trace), so that the device comparisons of tests/test_gpu_fusion_edges.py cannot pass on
inputs that miss the paths they are named for: every lattice has the blocks, chunk and slots it is meant to have, every
skip reason of the integration and every exit of the ray cast occurs in its case, the weights saturate and cross
255/256.

Reasons no honest input reaches, with the argument:
  * a crossing whose t* passes t_prev <= t* <= t_k and fails z_min <= t* <= z_max ("z_cut"): every sample lies in
    [tn, tf], which starts as [z_min, z_max] and only shrinks, so t_prev and t_k lie inside it and so does t*.  The
    z_min / z_max cut is therefore shown through the interval: the same pose hits with the wide range and not with
    the cut one.
  * a voxel with p'z == 0 that is updated: (p'x * fx) / 0 is an infinity or a NaN, and both fail the float range check
    of the pixel.  The voxel centres in the camera plane and at the camera centre are present all the same."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as C  # noqa: E402
import fusion_edge_inputs as X  # noqa: E402
import track_ref as K  # noqa: E402
import volume_ref as V  # noqa: E402


# ---------------------------------------------------------------- lattices
def test_lattices_are_the_intended_ones():
    for name, (w, h, stride, schedule, want) in X.EGO_CASES.items():
        assert X.lattice_of(w, h, stride) == want, (name, X.lattice_of(w, h, stride))
        assert 1 <= len(schedule) <= 3 and all(1 <= s <= 16 for s, _ in schedule)
        for s, _ in schedule:
            assert X.lattice_of(w, h, s)[4] <= X.MAX_SLOTS
    lattices = {k: v[4] for k, v in X.EGO_CASES.items()}                   # name -> (lw, n, n_blocks, chunk, n_slots)
    slots = {k: n_slots for k, (_, _, _, _, n_slots) in lattices.items()}
    assert slots["16x16"] == 1 and slots["1x1"] == 1                       # one workgroup: its own last arriver
    assert [slots[k] for k in ("48x37", "48x42", "48x43")] == [7, 8, 9] and X.STRANDS == 8
    assert slots["256x256"] == X.MAX_SLOTS == 256 and lattices["256x256"][3] == 1
    lw, n, nb, chunk, G = lattices["257x256"]
    assert chunk == 2 and G * chunk - nb == 1                              # the last workgroup walks one block of two
    lw, n, nb, chunk, G = lattices["17x16"]
    assert nb == 2 and n - X.THREADS == 16                                 # a block with 16 live indices
    lw, n, nb, chunk, G = lattices["83x61/4"]
    assert 83 % 4 and 61 % 4 and lw == 21 and n == 21 * 16
    assert X.EGO_CASES["333x251/16"][2] == 16
    sched = X.EGO_CASES["333x251 skip"][3]
    assert [it for _, it in sched] == [2, 0, 2]
    # the 640x480 lattices the suite ran before: none of the above
    assert [X.lattice_of(640, 480, s)[2:] for s in (4, 2, 1)] == [(75, 1, 75), (300, 2, 150), (1200, 5, 240)]


def test_small_sources_stop_or_step(synth):
    world, traj = X.ego_world(synth)
    c = X.ego_case(synth, world, traj, "1x1")
    T, r = C.egomotion(c["maps"][0], c["maps"][1], c["cam"], sums="f32", levels=c["schedule"])
    assert r["correspondences"] < 6 and r["iterations"] == [0, 0] and r["ok"] == 0 and np.array_equal(T, np.eye(4))
    for name in ("16x16", "17x16", "83x61/4"):
        c = X.ego_case(synth, world, traj, name)
        for levels in ([(c["stride"], 1)], c["schedule"]):
            T, r = C.egomotion(c["maps"][0], c["maps"][1], c["cam"], sums="f32", levels=levels)
            assert r["iterations"] == [it for _, it in levels] and r["correspondences"] >= 6, (name, r)
            assert r["cond"] > X.COND_STREAM_640                           # small and ill-conditioned: bits are not promised
    for name in X.BITS_HELD:                                               # well conditioned: the bit assertion is live
        c = X.ego_case(synth, world, traj, name)
        for levels in ([(c["stride"], 1)], c["schedule"]):
            T, r = C.egomotion(c["maps"][0], c["maps"][1], c["cam"], sums="f32", levels=levels)
            assert r["iterations"] == [it for _, it in levels] and 0 < r["cond"] < 0.1 * X.COND_STREAM_640, (name, r)
    # different views: the source's pixels land inside the larger destination
    a, b = X.ego_case(synth, world, traj, X.DIFFERENT_VIEWS[0]), X.ego_case(synth, world, traj, X.DIFFERENT_VIEWS[1])
    assert a["cam"] != b["cam"] and a["maps"][0][2].shape != b["maps"][1][2].shape
    p = C.default_params()
    pix, _, has = C.correspondences(a["maps"][0], b["maps"][1], np.eye(4, dtype=np.float32), b["cam"], p["max_corr_dist"],
                                    p["min_normal_dot"])
    assert (pix >= 0).sum() > has.sum() // 2 and pix.max() > a["w"] * a["h"]    # indices of the destination's size


def test_the_cond_of_the_640x480_stream(synth):
    world = C.make_world(synth, 0)
    traj = C.trajectory(synth, 0)
    maps = [K.view_maps(C.render(synth, world, T), C.CAM, C.MAX_JUMP) for T in traj]
    # cond is that of the first step, which the default schedule takes at stride 4
    conds = [C.egomotion(maps[f - 1], maps[f], C.CAM, sums="f32", levels=[(4, 1)])[1]["cond"] for f in range(1, 10)]
    print("cond of the first step, frames 1..9:", ["%.1f" % x for x in conds])
    assert 0.999 * X.COND_STREAM_640 < max(conds) <= X.COND_STREAM_640, conds


# ---------------------------------------------------------------- integration
def test_integration_inputs_reach_every_skip_reason():
    total = {}
    for name, n, T, img, cam in X.integration_cases():
        vol, tr = V.Volume(**X.volume_spec(n)), {}
        plain = V.Volume(**X.volume_spec(n))
        z = V.z_image(img, cam)
        assert vol.integrate(z, cam, T, trace=tr) == plain.integrate(z, cam, T) == tr["updated"] > 0, name
        assert np.array_equal(vol.q, plain.q) and np.array_equal(vol.w, plain.w)          # the trace changes nothing
        size = n[0] * n[1] * n[2]
        assert tr["behind"] + tr["outside"] + tr["hole"] + tr["far"] + tr["updated"] == size, (name, tr)
        assert tr["updated"] < size // 8 and tr["outside"] > 0 and tr["far"] > 0 and tr["band"] > 0, (name, tr)
        if " centre " in name:
            assert 0.4 * size < tr["behind"] < 0.6 * size, (name, tr)      # half the volume behind the camera
            assert tr["at_minus_mu"] > 0 and tr["q_min"] > 0, (name, tr)   # sdf == -mu exactly: the last voxel that is kept
            assert np.array_equal(T[:3, 3].astype(np.float64), X.centre_of(X.volume_spec(n), n[0] // 2, n[1] // 2, n[2] // 2))
        if " near plane " in name:
            k = n[2] // 2                                                  # that layer is in front now, and projects far outside
            assert tr["behind"] == n[0] * n[1] * k and 0 < np.float32(X.centre_of(X.volume_spec(n), 0, 0, k)[2]) - T[2, 3] < 1e-6
        if "holes" in name:
            assert tr["hole"] > 0, (name, tr)
        else:
            assert tr["hole"] == 0
        if name.endswith("7x31") or name.endswith("9x33"):
            assert tr["clamped"] > 0 and tr["q_max"] > 0, (name, tr)
        if name == "136x16x16 end 9x33":
            assert vol.w[:, :, 128:].any() and vol.w[:, :, 64:128].any()   # the tile with 8 live lanes is written
        key = name.split(" ")[-1] if "holes" not in name else "holes"
        for k, v in tr.items():
            total[(key, k)] = total.get((key, k), 0) + v
    for shape in ("1x1", "7x31", "9x33"):
        for side in ("off_left", "off_right", "off_top", "off_bottom"):    # the ring one pixel outside, all four sides
            assert total[(shape, side)] > 0, (shape, side)


def test_weight_inputs_saturate_and_cross_256():
    n, T, imgs, cam = X.weight_case()
    z = [V.z_image(im, cam) for im in imgs]
    assert not np.array_equal(z[0], z[1])
    for mw in X.MAX_WEIGHTS:
        vol, tr, moved = V.Volume(**X.volume_spec(n, mw)), {}, 0
        for s in range(X.WEIGHT_STEPS):
            q0 = vol.q.copy()
            vol.integrate(z[s % 2], cam, T, trace=tr)
            moved += int(s >= 290 and (vol.q != q0).any())
            assert vol.w.max() == min(s + 1, mw)
        assert tr["w_max"] > 0 and tr["q_max"] > 0 and tr["q_neg"] > 0 and tr["q_min"] > 0, (mw, tr)
        assert (tr["w_256"] > 0) == (mw == 300), (mw, tr)                  # a weight crosses 255 -> 256
        if mw <= 2:
            assert moved == 11                                             # F keeps moving to the end
        assert (vol.q == 32767).any() and (vol.q == -32767).any() and ((vol.q < 0) & (vol.q > -32767)).any()


# ---------------------------------------------------------------- ray cast
@pytest.fixture(scope="module")
def ray_volume():
    return X.fused(X.RAY_N)


def cast(vol, T, cam, w, h):
    tr = {}
    z, maps, cnt = vol.raycast(T, X.full_cam(cam), w, h, trace=tr)
    z2, maps2, cnt2 = vol.raycast(T, X.full_cam(cam), w, h)
    assert z.tobytes() == z2.tobytes() and cnt == cnt2 and all(np.array_equal(a, b) for a, b in zip(maps, maps2))
    assert tr["hit"] == cnt["normals"] and tr["hit"] + tr["no_normal"] == cnt["hits"]
    assert sum(tr[k] for k in ("zero_miss", "empty", "exhausted", "back_face", "trilinear", "den", "off_bracket", "z_cut",
                               "no_normal", "hit")) == w * h
    return z, cnt, tr


def test_ray_inputs_reach_every_exit(ray_volume):
    vol = ray_volume
    assert 0 < (vol.w > 0).sum() < vol.w.size // 4 and vol.w.max() == 2
    got, worst = {}, -1
    for name, T, cam, w, h in X.ray_cases():
        z, cnt, tr = cast(vol, T, cam, w, h)
        why = tr.pop("exit")
        got[name] = (z, cnt, tr, why)
        worst = max(worst, tr["max_step"])
        assert tr["z_cut"] == 0, name                                      # see the module's docstring
    print({k: v[2] for k, v in got.items()})
    assert 0 <= worst < V.MAX_STEPS // 8                                   # far below the step limit
    cx, cy = int(X.RAY_CAM["cx"]), int(X.RAY_CAM["cy"])
    z, cnt, tr, why = got["zero inside"]
    assert tr["zero_miss"] == 0 and tr["zero_marched"] == X.RAY_W + X.RAY_H - 1     # column cx and row cy, all marched
    assert (z[:, cx] > 0).any() and (z[cy, :] > 0).any()                   # and they hit
    assert tr["hit"] > 1000 and tr["no_normal"] > 0 and tr["trilinear"] > 0 and tr["den"] > 0 and tr["off_bracket"] > 0
    z, cnt, tr, why = got["zero outside x"]
    assert (why[:, cx] == "zero_miss").all() and tr["zero_miss"] == X.RAY_H and tr["empty"] > 0 and tr["exhausted"] > 0
    z, cnt, tr, why = got["zero outside y"]
    assert (why[cy, :] == "zero_miss").all() and tr["zero_miss"] == X.RAY_W and tr["hit"] > 0
    z, cnt, tr, why = got["turned inside"]
    assert tr["zero_miss"] == 0 and tr["zero_marched"] == X.RAY_W + X.RAY_H - 1 and tr["hit"] > 0 and tr["back_face"] > 0
    z, cnt, tr, why = got["turned outside z"]
    assert (why[:, cx] == "zero_miss").all() and tr["zero_miss"] == X.RAY_H
    assert got["inside"][2]["hit"] > 1000 and got["outside"][2]["hit"] > 100 and got["outside"][2]["tn_is_z_min"] == 0
    z, cnt, tr, why = got["behind the wall"]
    assert tr["back_face"] == X.RAY_W * X.RAY_H and cnt["hits"] == 0
    for name, key in (("z_max before the surface", "tf_is_z_max"), ("z_min behind the surface", "tn_is_z_min")):
        z, cnt, tr, why = got[name]
        assert cnt["hits"] == 0 and tr[key] == X.RAY_W * X.RAY_H and tr["exhausted"] == X.RAY_W * X.RAY_H, (name, tr)
        T, cam = [(c[1], c[2]) for c in X.ray_cases() if c[0] == name][0]
        assert cast(vol, T, X.RAY_CAM, X.RAY_W, X.RAY_H)[1]["hits"] > 2000  # the same pose without the cut
    z, cnt, tr, why = got["across the gap"]
    assert tr["gap_then_hit"] > 100 and tr["hit"] > 100
    for h, w in ((1, 1), (33, 9), (9, 33), (31, 7)):
        z, cnt, tr, why = got["shape %dx%d" % (h, w)]
        assert z.shape == (h, w) and (h * w == 1 or tr["hit"] > h * w // 4)


def test_small_volumes_are_hit():
    for n in X.VOLUME_SIZES[:2]:
        vol = X.fused(n)
        for name, T, cam, w, h in X.small_ray_cases(n):
            z, cnt, tr = cast(vol, T, cam, w, h)
            assert tr["hit"] > 50 and tr["no_normal"] > 0, (n, name, tr)


def test_special_ray_cases_reach_their_branches():
    got = {}
    for name, n, frames, T, cam, w, h in X.special_ray_cases():
        vol = V.Volume(**X.volume_spec(n))
        for img, fcam, Tf in frames:
            assert vol.integrate(V.z_image(img, fcam), fcam, Tf) > 0
        z, cnt, tr = cast(vol, T, cam, w, h)
        got[name] = (z, cnt, tr, vol)
    print({k: {a: b for a, b in v[2].items() if a != "exit"} for k, v in got.items()})
    z, cnt, tr, vol = got["zero then negative"]
    # Fp == 0 exactly, then F < 0: no crossing, where everything a crossing needs is there (the result depends on Fp > 0)
    assert tr["zero_then_negative_live"] > 100 and (vol.q[vol.w > 0] == 0).any(), tr
    assert cnt["hits"] < tr["zero_then_negative_live"]
    z, cnt, tr, vol = got["low sliver"]
    lo = vol.origin[1]
    assert lo + 0.5 * vol.voxel < -0.9 < lo + vol.voxel                    # trilinear reads succeed there, the slab says no
    assert (tr["exit"][4, :] == "zero_miss").all() and tr["zero_miss"] == 33 and not z[4].any()
    assert (z[5] > 0).sum() > 20 and (z[6] > 0).sum() > 20 and vol.w[:, 0, :].any() and vol.w[:, 1, :].any()
    z, cnt, tr, vol = got["inside the band"]
    assert tr["back_face"] > 500                                           # by the rule these rays end there
