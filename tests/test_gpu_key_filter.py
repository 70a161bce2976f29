"""GPU: the scene-key stage drops (reference point, group of 64 scene points) blocks by a box test and keys the rest.

Phase 1 of k_scene_count and k_scene_hits walks the scene in Morton order and drops a block whose bounding box cannot
hold a pair within reach (pc_box_bin_range against the reach bitset); what is left goes through the unchanged per-pair
test and the unchanged keying.  Nothing may be lost and nothing added: for a 600-point model and each of the scenes
below, the sorted hit list of a few reference points (the hit tap) is, as a multiset of (key number, scene index), what
the row-key tap and the model's key set give on the host, and the demand keep_count is the host's count by the same
predicate -- the pair's distance bin (float32, the kernels' operation order) is within reach, where reach is worked out
here from the model's keys by hashing all 17^3 angle combinations of the bin.  theta_v of the hits is checked through the
accumulator they vote, against the oracle's.

The scenes: 3000 points; 3001 (a ragged last group and tile); 63 (less than one group); a lattice whose every pair is
farther apart than the model's diameter (only bins that collide by hash are within reach: nearly every block is
dropped); 1024 copies of one point next to a reference point (every pair of a tile is kept: a full list); one NaN and one
infinite coordinate (their groups are never dropped, their pairs never hit); and the clouds of
test_more_distance_bins_than_the_key_map_covers with 3000 and 40000 bins (beyond the key map; beyond the bitset)."""
import numpy as np
import pytest

from conftest import make_case

pytestmark = pytest.mark.gpu

REACH_BINS = 16384
FNV_BASIS, FNV_PRIME = 2166136261, 16777619
NAN_BITS = 0xFFC00000


def _fnv_word(h, w):
    """pm_fnv1a_word on uint64 arrays: four bytes, low first, each read through a signed char"""
    h = np.asarray(h, np.uint64)
    w = np.asarray(w, np.uint64)
    for _ in range(4):
        b = w & np.uint64(0xFF)
        b = np.where(b >= 0x80, b | np.uint64(0xFFFFFF00), b)
        h = ((h ^ b) * np.uint64(FNV_PRIME)) & np.uint64(0xFFFFFFFF)
        w = w >> np.uint64(8)
    return h


def _angle_bits():
    d_angle = np.float32(2.0) * np.float32(np.pi) / np.float32(30.0)
    bits = (np.arange(16, dtype=np.float32) * d_angle).view(np.uint32).astype(np.uint64)
    return np.concatenate([bits, np.array([NAN_BITS], np.uint64)])


def _bins_in_reach(bins, d, model_keys):
    """pc_key_of_bins over the 17^3 angle combinations of every bin: does the model hold one of the keys?"""
    if len(bins) == 0:
        return np.zeros(0, bool)
    ab = _angle_bits()
    q = (bins.astype(np.float32) * np.float32(d)).view(np.uint32)
    h = _fnv_word(np.uint64(FNV_BASIS), q)
    for _ in range(3):
        h = _fnv_word(h[..., None], ab)
    return np.isin(h.astype(np.uint32), model_keys).reshape(len(bins), -1).any(axis=1)


def _dist_bins(sp, r, d):
    """pc_pair_dist_bin of (r, every point): float32 in the kernels' order; -1 where the quotient is no bin"""
    with np.errstate(all="ignore"):
        dx, dy, dz = (sp[:, a] - sp[r, a] for a in range(3))
        nd = np.sqrt(dx * dx + dy * dy + dz * dz)
        q = nd.astype(np.float64) / np.float64(np.float32(d))
        ok = np.isfinite(q) & (nd * (np.float32(1.0) / np.float32(d)) < np.float32(2097152.0))
        return np.where(ok, np.floor(np.where(ok, q, 0.0)), -1).astype(np.int64)


def _check_scene(ppf, model, keys, nums, sp, sn, d, refs):
    scene = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=1)
    n_hits = n_keep = 0
    for r in refs:
        num, th, idx, keep = model.vote_hits(scene, r)
        # the demand: pairs whose distance bin is within reach, bins beyond the bitset and non-bins included
        k = _dist_bins(sp, r, d)
        inside = (k >= 0) & (k < REACH_BINS)
        ub = np.unique(k[inside])
        reach = dict(zip(ub.tolist(), _bins_in_reach(ub, d, keys).tolist()))
        kept = np.array([reach[int(b)] if i else True for b, i in zip(k, inside)], bool)
        kept[r] = False
        assert keep == int(kept.sum()), (r, keep, int(kept.sum()))
        # the hits: the pairs whose key the model holds, under the key's number
        row = scene.getHashKeys(r)
        at = np.searchsorted(keys, row)
        at[at == len(keys)] = 0
        hit = (row != 0) & (keys[at] == row)
        hit[r] = False
        want = np.stack([nums[at[hit]].astype(np.int64), np.nonzero(hit)[0].astype(np.int64)], 1)
        got = np.stack([num.astype(np.int64), idx.astype(np.int64)], 1)
        want = want[np.lexsort((want[:, 1], want[:, 0]))]
        # the list is sorted by key number: the whole list up to one segment of the sort (every list here but those of
        # test_gpu_wide_keys), segment by segment beyond (tests/sort_ref.py: 16384 hits, 8192 from 2^18 key numbers on)
        seg = 16384 if len(keys) <= 1 << 18 else 8192
        assert all(np.all(num[s + 1:s + seg] >= num[s:s + seg][:-1]) for s in range(0, len(num), seg))
        got = got[np.lexsort((got[:, 1], got[:, 0]))]
        assert np.array_equal(got, want), (r, len(got), len(want))
        assert np.all(kept[idx]) and len(got) <= keep                       # every hit was a kept pair
        n_hits += len(got)
        n_keep += keep
    return scene, n_hits, n_keep


@pytest.fixture(scope="module")
def model600(ppf, synth):
    c = make_case(synth, 600, 3000, 2031)
    model = ppf.Model(c["mp"], c["mn"], d_dist=c["d"])
    keys, nums, _ = model.key_numbers()
    return c, model, keys, nums


@pytest.mark.parametrize("S", [3000, 3001, 63])
def test_hit_lists_of_a_scene(ppf, synth, oracle, model600, S):
    c, model, keys, nums = model600
    sc = c if S == 3000 else make_case(synth, 600, S, 2031 + S)
    sp, sn = sc["sp"], sc["sn"]
    refs = sorted({0, 1, 62, S // 2, S - 1})
    scene, n_hits, _ = _check_scene(ppf, model, keys, nums, sp, sn, c["d"], refs)
    assert n_hits > 0
    if S == 3000:
        for r in (0, S - 1):                                                # theta_v of the hits, through their votes
            assert np.array_equal(model.vote_accumulator(scene, r), oracle.accumulator_for_ref(c["mp"], c["mn"], sp, sn, r, c["d"]))


def test_scene_beyond_the_models_diameter(ppf, model600):
    """Every pair is farther apart than the model is wide: what is kept lies in bins that reach a key by hash collision
    alone, a few in a thousand bins, so nearly every block is dropped -- and the count and the hits still hold."""
    c, model, keys, nums = model600
    rng = np.random.default_rng(5)
    diam = float(np.linalg.norm(c["mp"].max(0) - c["mp"].min(0)))
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
    sp = (g * (1.6 * diam) + rng.uniform(-0.25, 0.25, g.shape) * diam).astype(np.float32)
    sn = rng.normal(size=sp.shape).astype(np.float32)
    k0 = _dist_bins(sp, 0, c["d"])
    top_real = int(np.ceil(diam / c["d"]))
    assert np.all(np.delete(k0, 0) > top_real)
    _, _, n_keep = _check_scene(ppf, model, keys, nums, sp, sn, c["d"], [0, 100, 227, len(sp) - 1])
    assert n_keep < 4 * len(sp) // 10                                       # far fewer than the pairs


def test_a_tile_whose_every_pair_is_kept(ppf, model600):
    """1024 copies of one point two bins from reference point 0: one tile, every pair of it kept, its list full."""
    c, model, keys, nums = model600
    sp = np.repeat(c["sp"][:1], 1025, 0).copy()
    sn = np.repeat(c["sn"][:1], 1025, 0).copy()
    sp[1:, 0] += np.float32(2.5 * c["d"])
    sn[1:] = c["sn"][1]
    _, _, n_keep = _check_scene(ppf, model, keys, nums, sp, sn, c["d"], [0, 1, 1024])
    assert n_keep >= 1024


def test_coordinates_that_are_not_finite(ppf, model600):
    c, model, keys, nums = model600
    sp, sn = c["sp"].copy(), c["sn"].copy()
    sp[17, 1] = np.nan
    sp[40, 0] = np.inf
    _check_scene(ppf, model, keys, nums, sp, sn, c["d"], [0, 16, 17, 40, 41, len(sp) - 1])


@pytest.mark.parametrize("bins", [3000, 40000])
def test_more_bins_than_the_key_map_or_the_bitset(ppf, bins):
    rng = np.random.default_rng(77)
    M, S = 90, 260
    mp = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    mn = rng.normal(size=(M, 3)).astype(np.float32)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    sp = rng.uniform(-2, 2, (S, 3)).astype(np.float32)
    sn = rng.normal(size=(S, 3)).astype(np.float32)
    sp[:M] = (mp @ R.T + np.float32([0.3, -0.2, 0.1])).astype(np.float32)
    sn[:M] = (mn @ R.T).astype(np.float32)
    d = float(np.float32(7.0 / bins))
    model = ppf.Model(mp, mn, d_dist=d)
    keys, nums, _ = model.key_numbers()
    _, n_hits, _ = _check_scene(ppf, model, keys, nums, sp, sn, d, [0, 5, M - 1, S - 1])
    assert n_hits > 0
