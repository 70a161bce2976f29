"""GPU: key numbers at or above 2^18 through whole registrations.

A model of 800 random points at d_dist = 3.5 / 1500 has some 460 000 distinct keys: its numbers take 19 bits, its hit
lists go through the 64-bit instantiation of k_sort_hits (segments of 8192), and kmap, the uinfo rows, the near-edge
search of k_vote and the slot_r packing all see numbers at or above 2^18, which no other model of the suite has.  The
scenes are exact copies of model points: identical coordinates give bit-identical keys, so every copy hits, a reference
point has more than one segment of hits and a key more than one run.

Checked: the hit list against the row-key tap and the key set (_check_scene of test_gpu_key_filter, unchanged), the
accumulator against the oracle's, and one registration's cells, counters and pose against the oracle's -- at 1500 bins
(numbers from the key map) and at 3000 (beyond OSLAMK_KMAP_MAX_BINS: hashed and probed); a database group of two
500-point models whose union of keys, not either alone, passes 2^18; and one run that mixes a hit with the "always
re-evaluate" marker and a hit without.  tests/test_sort_host.py checks the constructions on the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDE = 1 << 18
EXTRA_POINTS = (5, 300, 650)            # the three model points with extra copies in the scene
EXTRA_COPIES = 120
WIDE_REFS = (0, 4321, 8005)             # a first copy, a later copy, an extra copy of point 5
WIDE_DF = 401
MIXED_ON_AXIS, MIXED_OFF_AXIS = 1, 60   # scene indices of the mixed run's two hits


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nr = rng.normal(size=(n, 3))
    return p, (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)


def wide_model(bins):
    mp, mn = random_cloud(800, 1801)
    return mp, mn, float(np.float32(3.5 / bins))


def wide_scene(mp, mn):
    """ten copies of every model point, then EXTRA_COPIES more of three of them: a reference point has 7990 hits from the
    ten copies and at least 240 from the extra ones, and its key with an extra point has 130"""
    pick = np.concatenate([np.tile(np.arange(len(mp)), 10), np.repeat(EXTRA_POINTS, EXTRA_COPIES)])
    return mp[pick].copy(), mn[pick].copy()


def group_models():
    return random_cloud(500, 1802), random_cloud(500, 1803), float(np.float32(3.5 / 1500))


def group_scene(ca, cb):
    return np.concatenate([ca[0], cb[0]]), np.concatenate([ca[1], cb[1]])


def mixed_run_case():
    """model and scene share 60 points: point 0 at the origin with the normal (1, 0, 0) exactly, point 1 on that axis;
    the scene adds point 60, point 1 moved 1e-5 off the axis: the same key, but a theta of its own"""
    rng = np.random.default_rng(1804)
    mp = rng.uniform(-1, 1, (60, 3)).astype(np.float32)
    mn = rng.normal(size=(60, 3))
    mn = (mn / np.linalg.norm(mn, axis=1, keepdims=True)).astype(np.float32)
    mp[0], mn[0] = (0, 0, 0), (1, 0, 0)
    mp[1], mn[1] = (0.53, 0, 0), np.float32([0.6, 0.64, 0.48])
    sp, sn = np.concatenate([mp, mp[1:2]]), np.concatenate([mn, mn[1:2]])
    sp[60, 1] = np.float32(1e-5)
    return mp, mn, sp, sn, 0.05


def oracle_key_set(oracle, mp, mn, d):
    keys = np.unique(oracle.ppf_all_pairs(mp, mn, 1, d, want_ppf=False)[1])
    return keys[keys != 0]


def _check_registration(ppf, oracle, model, scene, mp, mn, sp, sn, df, d):
    T = model.ppf_lookup(scene)
    cells, _ = model.last_cells()
    ocells, ost = oracle.votes_fused(mp, mn, sp, sn, df, d, 0.4)
    assert len(ocells) > 0
    assert np.array_equal(cells["code"], ocells["code"]) and np.array_equal(cells["count"], ocells["count"])
    for k in ("num_scene_ppfs", "num_hits", "num_votes", "num_unique_votes", "num_model_keys", "max_count", "num_top"):
        assert model.stats[k] == ost[k], (k, model.stats[k], ost[k])
    assert ost["num_model_keys"] > WIDE
    rc, To = oracle.pose_from_cells(ocells, mp, mn, sp, sn, d)
    assert rc == 0 and np.array_equal(T, To)


@pytest.mark.parametrize("bins", [1500, 3000])
def test_one_model_with_more_than_2_18_keys(ppf, oracle, bins):
    from test_gpu_key_filter import _check_scene
    mp, mn, d = wide_model(bins)
    model = ppf.Model(mp, mn, d_dist=d)
    keys, nums, _ = model.key_numbers()
    assert len(keys) > WIDE and int(nums.max()) == len(keys) - 1
    sp, sn = wide_scene(mp, mn)
    scene, _, _ = _check_scene(ppf, model, keys, nums, sp, sn, d, WIDE_REFS)
    for r in WIDE_REFS:
        num, th, idx, _ = model.vote_hits(scene, r)
        assert len(num) > 8192                                              # more than one segment of 64-bit elements
        assert np.unique(num, return_counts=True)[1].max() > 64             # a key with more than one run
        assert int(num.max()) >= WIDE                                       # numbers the 32-bit element cannot hold
        assert np.array_equal(model.vote_accumulator(scene, r), oracle.accumulator_for_ref(mp, mn, sp, sn, r, d))
    scene.close()
    coarse = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=WIDE_DF)
    _check_registration(ppf, oracle, model, coarse, mp, mn, sp, sn, WIDE_DF, d)
    coarse.close()
    model.close()


def test_database_group_whose_union_passes_2_18_keys(ppf, oracle):
    ca, cb, d = group_models()
    sp, sn = group_scene(ca, cb)
    scene = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=1)
    alone = []
    for mp, mn in (ca, cb):
        one = ppf.Model(mp, mn, d_dist=d)
        assert len(one.key_numbers()[0]) < WIDE
        T = one.ppf_lookup(scene).copy()
        alone.append((T, one.last_cells()[0].copy(), dict(one.stats)))
        one.close()
    models = [ppf.Model(mp, mn, d_dist=d) for mp, mn in (ca, cb)]
    db = ppf.Database(models)
    assert db.n_groups == 1
    keys, nums, _ = models[0].key_numbers()                                  # inside a database: the group's numbering
    assert len(keys) > WIDE and int(nums.max()) == len(keys) - 1
    assert all(np.array_equal(a, b) for a, b in zip(models[1].key_numbers()[:2], (keys, nums)))
    T, stats = db.align(scene)
    for j, (mp, mn) in enumerate((ca, cb)):
        cells = models[j].last_cells()[0]
        ocells, ost = oracle.votes_fused(mp, mn, sp, sn, 1, d, 0.4)
        assert len(ocells) > 0
        for want in (alone[j][1], ocells):
            assert np.array_equal(cells["code"], want["code"]) and np.array_equal(cells["count"], want["count"]), j
        for k in ("num_scene_ppfs", "num_votes", "num_unique_votes", "max_count"):
            assert stats[j][k] == ost[k] == alone[j][2][k], (j, k, stats[j][k], ost[k], alone[j][2][k])
        rc, To = oracle.pose_from_cells(ocells, mp, mn, sp, sn, d)
        assert rc == 0 and np.array_equal(T[j], To) and np.array_equal(T[j], alone[j][0]), j
    db.close()
    for m in models:
        m.close()
    scene.close()


def test_a_run_that_mixes_a_marked_hit_and_a_clean_one(ppf, oracle):
    mp, mn, sp, sn, d = mixed_run_case()
    model = ppf.Model(mp, mn, d_dist=d)
    scene = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=1)
    num, th, idx, _ = model.vote_hits(scene, 0)
    at = {int(i): k for k, i in enumerate(idx)}
    a, b = at[MIXED_ON_AXIS], at[MIXED_OFF_AXIS]
    assert num[a] == num[b] and len(num) <= 64                              # one number inside one group of 64: one run
    assert th[a] == 0xFFFFFFFF and th[b] != 0xFFFFFFFF
    assert np.array_equal(model.vote_accumulator(scene, 0), oracle.accumulator_for_ref(mp, mn, sp, sn, 0, d))
    scene.close()
    model.close()
