"""GPU: the order in which the vote kernel's work is handed out (oslam_params.vote_order) changes no result.

Largest first at both levels is the default: a model's keys are numbered by descending bucket weight (the hit sort
orders a reference point's runs by key number, so a workgroup's waves end on short buckets), and the reference points
of a batch go out by descending demand (so the last rounds of the grid are light).  vote_order 1 is the order before
that: keys numbered in union-slot order, reference points in index order; 2 and 3 switch one level each.

The numbering itself is read through the key-number tap and checked against the buckets; the registrations are checked
word for word between the orders, and against the oracle on the small case."""
import numpy as np
import pytest

from conftest import cells_equal, make_case

pytestmark = pytest.mark.gpu

STAT_KEYS = ("num_votes", "num_hits", "num_unique_votes", "max_count")


def _check_numbering(keys, nums, w):
    n = len(keys)
    assert n > 0 and np.all(keys[1:] > keys[:-1])                 # the tap lists every key once, ascending
    assert np.array_equal(np.sort(nums), np.arange(n, dtype=np.uint32))
    by_num = np.argsort(nums)
    ww, kk = w[by_num].astype(np.int64), keys[by_num].astype(np.int64)
    assert np.all(ww[1:] <= ww[:-1])                               # number 0 is the heaviest key
    tie = ww[1:] == ww[:-1]
    assert np.all(kk[1:][tie] > kk[:-1][tie])                      # equal weights: ascending key


def _sample(keys, nums, rng, n_each=48):
    """the heaviest, the lightest and some keys in between"""
    by_num = np.argsort(nums)
    pick = np.concatenate([by_num[:n_each], by_num[-n_each:], rng.choice(len(keys), min(n_each, len(keys)), replace=False)])
    return np.unique(pick)


def _check_weights(models, keys, nums, w, rng):
    for i in _sample(keys, nums, rng):
        assert int(w[i]) == sum(m.bucket(int(keys[i]), cap=1)[1] for m in models), int(keys[i])


def test_numbering_one_slice(ppf, built_lib, synth, tmp_path):
    mp, mn = synth.make_model(0, 300)
    d = synth.d_dist_for(mp, 0.05)
    mo = ppf.Model(mp, mn, d_dist=d)
    keys, nums, w = mo.key_numbers()
    _check_numbering(keys, nums, w)
    # every weight, against the key kernel: the pairs (r, i != r) of the model under each key (key 0 is never stored)
    rows = np.concatenate([mo.getHashKeys(r) for r in range(len(mp))])
    uk, cnt = np.unique(rows[rows != 0], return_counts=True)
    assert np.array_equal(uk, keys) and np.array_equal(cnt.astype(np.uint64), w)
    _check_weights([mo], keys, nums, w, np.random.default_rng(1))
    # a second build and a saved and reloaded model give the same numbers
    again = ppf.Model(mp, mn, d_dist=d)
    for a, b in zip(again.key_numbers(), (keys, nums, w)):
        assert np.array_equal(a, b)
    f = str(tmp_path / "m.oslam")
    mo.save(f)
    loaded = ppf.Model.load(f)
    for a, b in zip(loaded.key_numbers(), (keys, nums, w)):
        assert np.array_equal(a, b)
    # the order before: union-slot order, the same keys and weights
    old = ppf.Model(mp, mn, d_dist=d, params=ppf.default_params(vote_order=1))
    k1, n1, w1 = old.key_numbers()
    assert np.array_equal(k1, keys) and np.array_equal(w1, w)
    assert np.array_equal(np.sort(n1), np.arange(len(keys), dtype=np.uint32)) and not np.array_equal(n1, nums)
    for m in (mo, again, loaded, old):
        m.close()


def test_numbering_two_slices(ppf, built_lib, case_two_slices, tmp_path):
    c = case_two_slices
    mo = ppf.Model(c["mp"], c["mn"], d_dist=c["d"])
    keys, nums, w = mo.key_numbers()
    _check_numbering(keys, nums, w)
    assert int(w.sum()) <= len(c["mp"]) * (len(c["mp"]) - 1)
    _check_weights([mo], keys, nums, w, np.random.default_rng(2))     # bucket() sums the key's buckets of both slices
    again = ppf.Model(c["mp"], c["mn"], d_dist=c["d"])
    f = str(tmp_path / "m2.oslam")
    mo.save(f)
    loaded = ppf.Model.load(f)
    for other in (again, loaded):
        for a, b in zip(other.key_numbers(), (keys, nums, w)):
            assert np.array_equal(a, b)
    for m in (mo, again, loaded):
        m.close()


def test_numbering_group_of_unequal_models(ppf, built_lib, synth):
    clouds = [synth.make_model(0, 300), synth.make_model(1, 170)]
    d = synth.d_dist_for(clouds[0][0], 0.05)
    alone = []

    def build():
        return [ppf.Model(p, n, d_dist=d) for p, n in clouds]

    models = build()
    alone = [m.key_numbers() for m in models]
    db = ppf.Database(models)
    assert db.n_groups == 1
    keys, nums, w = models[0].key_numbers()
    for a, b in zip(models[1].key_numbers(), (keys, nums, w)):       # one numbering for the group
        assert np.array_equal(a, b)
    _check_numbering(keys, nums, w)
    assert np.array_equal(keys, np.union1d(alone[0][0], alone[1][0]))
    # the weight of a key: its entries in every member
    want = np.zeros(len(keys), np.uint64)
    for k, _, wk in alone:
        want[np.searchsorted(keys, k)] += wk
    assert np.array_equal(w, want)
    _check_weights(models, keys, nums, w, np.random.default_rng(3))
    # a second build of the group gives the same numbers
    models2 = build()
    db2 = ppf.Database(models2)
    for a, b in zip(models2[1].key_numbers(), (keys, nums, w)):
        assert np.array_equal(a, b)
    db2.close()
    # a member that leaves its group has its own numbering again
    db.close()
    for m, want_alone in zip(models, alone):
        for a, b in zip(m.key_numbers(), want_alone):
            assert np.array_equal(a, b)
    for m in models + models2:
        m.close()


def _register(ppf, c, df, order, mode=0, acc_refs=()):
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], ref_point_downsample_factor=df)
    mo = ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=ppf.default_params(vote_order=order, vote_mode=mode))
    T = mo.ppf_lookup(sc).copy()
    cells = mo.last_cells()[0]
    st = {k: mo.stats[k] for k in STAT_KEYS}
    accs = [mo.vote_accumulator(sc, r) for r in acc_refs]
    mo.close()
    sc.close()
    return T, cells, st, accs


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert cells_equal(a[1], b[1])
    assert a[2] == b[2]
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(x, y)


@pytest.fixture(scope="module")
def case_600(synth):
    return make_case(synth, 600, 3000, 2071)


@pytest.mark.parametrize("df, n_ref", [(3000, 1), (231, 13), (40, 75)])
def test_both_orders_give_the_same_registration(ppf, built_lib, case_600, df, n_ref):
    """600 model points against 3 000 scene points: one reference point, 13 (not a multiple of the 8 of a dispatch
    group) and 75 (more than 64)."""
    c = case_600
    assert (len(c["sp"]) + df - 1) // df == n_ref
    refs = sorted({0, (n_ref // 2) * df, (n_ref - 1) * df})
    new = _register(ppf, c, df, 0, acc_refs=refs)
    old = _register(ppf, c, df, 1, acc_refs=refs)
    _same(new, old)
    assert new[2]["num_votes"] > 0


def test_both_orders_two_slices(ppf, built_lib, case_two_slices):
    refs = (0, 700, 1490)
    new = _register(ppf, case_two_slices, 10, 0, acc_refs=refs)
    _same(new, _register(ppf, case_two_slices, 10, 1, acc_refs=refs))


def test_both_orders_fast_mode(ppf, built_lib, case_600):
    new = _register(ppf, case_600, 40, 0, mode=ppf.VOTE_FAST, acc_refs=(0, 1480))
    _same(new, _register(ppf, case_600, 40, 1, mode=ppf.VOTE_FAST, acc_refs=(0, 1480)))


def test_both_orders_group_in_one_grid(ppf, built_lib, synth):
    """two members of unequal size voted in one grid (k_vote_group): every member gives the same in both orders, and
    what it gives alone"""
    c = make_case(synth, 300, 900, 2031)
    c2 = make_case(synth, 170, 900, 2031, model_id=1)
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=0.0, ref_point_downsample_factor=3)
    got = {}
    for order in (0, 1):
        par = [ppf.default_params(vote_order=order) for _ in range(2)]
        models = [ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=par[0]),
                  ppf.Model(c2["mp"], c2["mn"], d_dist=c["d"], params=par[1])]
        alone = []
        for m in models:
            T = m.ppf_lookup(sc, allow_no_votes=True).copy()
            alone.append((T, m.last_cells()[0], {k: m.stats[k] for k in STAT_KEYS if k != "num_hits"}))
        db = ppf.Database(models)
        assert db.n_groups == 1
        Ts, stats = db.align(sc)
        got[order] = [(Ts[j].copy(), models[j].last_cells()[0], {k: stats[j][k] for k in STAT_KEYS if k != "num_hits"})
                      for j in range(2)]
        for j in range(2):
            assert np.array_equal(got[order][j][0], alone[j][0]) and cells_equal(got[order][j][1], alone[j][1])
            assert got[order][j][2] == alone[j][2]
        db.close()
        for m in models:
            m.close()
    for j in range(2):
        assert np.array_equal(got[0][j][0], got[1][j][0]) and cells_equal(got[0][j][1], got[1][j][1])
        assert got[0][j][2] == got[1][j][2]
    sc.close()


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_every_order_equals_the_oracle(ppf, oracle, built_lib, case_small, order):
    c = case_small
    T, cells, st, _ = _register(ppf, c, 1, order)
    ocells, ost = oracle.votes_fused(c["mp"], c["mn"], c["sp"], c["sn"], 1, c["d"], 0.4)
    assert cells_equal(cells, ocells)
    for k in STAT_KEYS:
        assert st[k] == ost[k], k
    _, To = oracle.pose_from_cells(ocells, c["mp"], c["mn"], c["sp"], c["sn"], c["d"])
    assert np.array_equal(T, To)


def _scene_case(synth, isolated):
    """A scene made of the model's own points (every scene pair is a model pair, so every pair is within reach: all
    reference points have the same demand, S - 1), with `isolated` far points put at the first `isolated` reference
    indices: those have next to no pair within reach, and the last reference point is the one heavy one."""
    mp, mn = synth.make_model(0, 300)
    d = synth.d_dist_for(mp, 0.05)
    if not isolated:
        return dict(mp=mp, mn=mn, sp=mp.copy(), sn=mn.copy(), d=d), 30
    df = 38
    sp, sn = list(mp), list(mn)
    far = 10.0 * float(np.linalg.norm(mp.max(0) - mp.min(0)))
    for j in range(isolated):
        sp.insert(j * df, np.array([far * (j + 1), 0.0, 0.0], np.float32))
        sn.insert(j * df, np.array([0.0, 0.0, 1.0], np.float32))
    return dict(mp=mp, mn=mn, sp=np.array(sp, np.float32), sn=np.array(sn, np.float32), d=d), df


@pytest.mark.parametrize("isolated", [0, 8])
def test_equal_demands_and_one_heavy_reference_point_last(ppf, oracle, built_lib, synth, isolated):
    c, df = _scene_case(synth, isolated)
    n_ref = (len(c["sp"]) + df - 1) // df
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], ref_point_downsample_factor=df)
    mo = ppf.Model(c["mp"], c["mn"], d_dist=c["d"])
    mo.ppf_lookup(sc)
    if isolated:
        assert n_ref == isolated + 1 and (n_ref - 1) * df < len(c["sp"])
        # the last reference point has its 299 pairs; a far pair counts only where its distance bin shares a hash
        # with a model key (1 % of the bins: 17^3 keys of a bin x 9 300 model keys / 2^32), so the eight others
        # together stay far below it
        extra = mo.stats["num_pairs_probed"] - (len(c["mp"]) - 1)
        assert 0 <= extra < (len(c["mp"]) - 1) // 4
    else:
        assert mo.stats["num_pairs_probed"] == n_ref * (len(c["sp"]) - 1)   # every reference point the same
    mo.close()
    sc.close()
    refs = (0, (n_ref - 1) * df)
    new = _register(ppf, c, df, 0, acc_refs=refs)
    _same(new, _register(ppf, c, df, 1, acc_refs=refs))
    ocells, ost = oracle.votes_fused(c["mp"], c["mn"], c["sp"], c["sn"], df, c["d"], 0.4)
    assert cells_equal(new[1], ocells)
    for k in STAT_KEYS:
        assert new[2][k] == ost[k], k
