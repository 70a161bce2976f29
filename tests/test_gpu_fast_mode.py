"""GPU: OSLAM_VOTE_FAST against the oracle's statement of it (oracle_ppf.c: fast_alpha_idx) and against the float64
alpha bins of tests/alpha_ref.py.

Every case is bit-exact against the oracle -- dense accumulators, peak cells, the counters in stats and the pose --
and every accumulator passes the float64 interval check within the bound include/oslam.h states for fast mode.  The
paths: the plain vote kernel, two table slices, the wide re-vote with 32-bit counters, database groups (one grid and
mixed modes), shards, degenerate vectors, save / load.  Exact mode is checked beside it on the same votes."""
import os
import sys

import numpy as np
import pytest

from conftest import cells_equal, make_case

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_ref as A  # noqa: E402
from test_refine_host import make_trial  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_BOUND = 2e-5
FAST_BOUND = 3.1e-5        # include/oslam.h (OSLAM_VOTE_FAST), ppf_core.h: PC_FAST_BOUND
STAT_KEYS = ("num_scene_ppfs", "num_hits", "num_votes", "num_unique_votes", "num_model_keys", "max_count", "num_top")


def fast_params(ppf, **kw):
    return ppf.default_params(vote_mode=ppf.VOTE_FAST, **kw)


def check_accumulators(mo, sc, fm, sp, sn, refs, vote_mode):
    """GPU accumulators of `refs` equal the oracle's and pass the float64 interval check; -> votes checked"""
    eps = FAST_BOUND if vote_mode else EXACT_BOUND
    n = 0
    for r in refs:
        got = mo.vote_accumulator(sc, r)
        assert np.array_equal(got, fm.accumulator(sp, sn, r, vote_mode=vote_mode)), r
        dv = fm.vote_dump(sp, sn, r, vote_mode=0)
        fails = A.interval_check(got, dv["m_r"], dv["uy"], dv["uz"], dv["vy"], dv["vz"], eps, vote_mode=vote_mode,
                                 exact_bins=dv["bin"])
        assert fails == [], (r, fails[:5])
        n += len(dv["m_r"])
    return n


def check_registration(ppf, oracle, mo, sc, mp, mn, sp, sn, d, df, vote_mode=1, T=None):
    """cells, counters and pose of the model's last registration against the oracle's fast (or exact) statement"""
    ocells, ost = oracle.votes_fused(mp, mn, sp, sn, df, d, mo.params.vote_count_threshold, vote_mode=vote_mode)
    cells = mo.last_cells()[0]
    assert cells_equal(cells, ocells)
    for k in STAT_KEYS:
        assert mo.stats[k] == ost[k], k
    if T is not None:
        _, To = oracle.pose_from_cells(ocells, mp, mn, sp, sn, d)
        assert np.array_equal(T, To)
    return ocells


def test_accumulators_of_many_reference_points(ppf, oracle, built_lib, synth):
    """100 reference points of a 600 x 3000 registration (2e6 votes, some 300 of them within 1.3e-4 bin below an
    edge): fast mode's accumulators are the oracle's fast statement cell for cell -- a base still shifted by the
    re-evaluation margin puts about 1e-4 of the votes into the next bin -- and exact mode's the reference's; then the
    whole registration in both modes."""
    mp, mn, d, sp, sn, _ = make_trial(synth, 600, 3000, 12, 0.1, 0.0)
    fm = oracle.FusedModel(mp, mn, d)
    refs = range(0, 3000, 30)
    try:
        for mode in (1, 0):
            par = fast_params(ppf) if mode else ppf.default_params()
            sc = ppf.Scene(sp, sn, d_dist=d, params=par)
            mo = ppf.Model(mp, mn, d_dist=d, params=par)
            n = check_accumulators(mo, sc, fm, sp, sn, refs, mode)
            assert n >= 10 ** 6
            T = mo.ppf_lookup(sc)
            check_registration(ppf, oracle, mo, sc, mp, mn, sp, sn, d, 1, mode, T)
            mo.close()
            sc.close()
    finally:
        fm.close()


def test_two_slices(ppf, oracle, built_lib, case_two_slices):
    c = case_two_slices
    par = fast_params(ppf)
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], ref_point_downsample_factor=10, params=par)
    mo = ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=par)
    fm = oracle.FusedModel(c["mp"], c["mn"], c["d"])
    check_accumulators(mo, sc, fm, c["sp"], c["sn"], (0, 750, 1490), 1)
    fm.close()
    T = mo.ppf_lookup(sc)
    check_registration(ppf, oracle, mo, sc, c["mp"], c["mn"], c["sp"], c["sn"], c["d"], 10, 1, T)


def _arc_cloud(n, rng, spread=0.15):
    a = rng.uniform(-spread, spread, n)
    p = np.zeros((n + 1, 3), np.float32)
    p[1:, 0] = np.cos(a)
    p[1:, 1] = np.sin(a)
    p[1:, 2] = rng.uniform(-1e-3, 1e-3, n)
    return p, np.tile(np.float32([0, 0, 1]), (n + 1, 1))


@pytest.mark.parametrize("filler", [0, 1040])
def test_wide_revote(ppf, oracle, built_lib, filler):
    """the arc clouds of test_gpu_configs.py::test_counters_beyond_16_bits: cells of 2.8e5 votes, re-voted with
    32-bit counters (k_vote_wide) in fast mode"""
    rng = np.random.default_rng(5)
    mp, mn = _arc_cloud(159, rng)
    sp, sn = _arc_cloud(2999, rng)
    if filler:
        fp = rng.uniform(5, 6, (filler, 3)).astype(np.float32)
        fn = rng.normal(size=(filler, 3)).astype(np.float32)
        fn /= np.linalg.norm(fn, axis=1, keepdims=True)
        mp, mn = np.concatenate([fp, mp]), np.concatenate([fn, mn])
    d = 0.3
    par = fast_params(ppf)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=1500, params=par)
    mo = ppf.Model(mp, mn, d_dist=d, params=par)
    fm = oracle.FusedModel(mp, mn, d)
    check_accumulators(mo, sc, fm, sp, sn, (0,), 1)
    fm.close()
    T = mo.ppf_lookup(sc)
    assert mo.stats["wide_workgroups"] > 0 and mo.stats["max_count"] > 4 * 65535
    check_registration(ppf, oracle, mo, sc, mp, mn, sp, sn, d, 1500, 1, T)


# what a database member reports as it would alone (its hits count the group's shared scene pass)
DB_KEYS = ("num_scene_ppfs", "num_votes", "num_unique_votes", "num_model_keys", "max_count", "num_top", "wide_workgroups")


def _single_and_db(ppf, models, sc, n_groups):
    single = []
    for mo in models:
        T = mo.ppf_lookup(sc, allow_no_votes=True).copy()
        single.append((T, mo.last_cells()[0], {k: mo.stats[k] for k in STAT_KEYS + ("wide_workgroups",)}))
    db = ppf.Database(models)
    assert db.n_groups == n_groups
    Ts, stats = db.align(sc)
    for j, mo in enumerate(models):
        T, cells, st = single[j]
        assert {k: stats[j][k] for k in DB_KEYS} == {k: st[k] for k in DB_KEYS}, j
        assert cells_equal(mo.last_cells()[0], cells), j
        assert np.array_equal(Ts[j], T), j
    db.close()
    return single


def test_database_groups(ppf, oracle, built_lib, synth):
    """A group of fast models votes in one grid (k_vote_group<1>), the arc models re-voted with 32-bit counters
    afterwards: each member gives what it gives alone, and that is the oracle's fast statement.  A database that mixes
    exact and fast members has one group per mode and gives each member's single-call result."""
    rng = np.random.default_rng(5)
    mp, mn = _arc_cloud(159, rng)
    sp, sn = _arc_cloud(2999, rng)
    mp2, mn2 = _arc_cloud(149, rng)
    op = rng.uniform(-1, 1, (140, 3)).astype(np.float32)
    on = rng.normal(size=(140, 3)).astype(np.float32)
    on /= np.linalg.norm(on, axis=1, keepdims=True)
    d = 0.3
    sc = ppf.Scene(sp, sn, d_dist=0.0, ref_point_downsample_factor=1500)
    clouds = ((mp, mn), (op, on), (mp2, mn2))
    models = [ppf.Model(a, b, d_dist=d, params=fast_params(ppf)) for a, b in clouds]
    single = _single_and_db(ppf, models, sc, 1)
    assert single[0][2]["wide_workgroups"] > 0
    for (a, b), (T, cells, st) in zip(clouds, single):
        ocells, ost = oracle.votes_fused(a, b, sp, sn, 1500, d, 0.4, vote_mode=1)
        assert cells_equal(cells, ocells) and all(st[k] == ost[k] for k in STAT_KEYS)
    for m in models:
        m.close()

    c = make_case(synth, 300, 900, 2031)
    c2 = make_case(synth, 250, 900, 2031, model_id=1)
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=0.0, ref_point_downsample_factor=3)
    mixed = [ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=fast_params(ppf)),
             ppf.Model(c["mp"], c["mn"], d_dist=c["d"]),
             ppf.Model(c2["mp"], c2["mn"], d_dist=c["d"], params=fast_params(ppf))]
    single = _single_and_db(ppf, mixed, sc, 2)
    for (mp_, mn_), mode, (T, cells, st) in zip(((c["mp"], c["mn"]), (c["mp"], c["mn"]), (c2["mp"], c2["mn"])),
                                               (1, 0, 1), single):
        ocells, ost = oracle.votes_fused(mp_, mn_, c["sp"], c["sn"], 3, c["d"], 0.4, vote_mode=mode)
        assert cells_equal(cells, ocells) and all(st[k] == ost[k] for k in STAT_KEYS), mode
    for m in mixed:
        m.close()


def test_shards_equal_the_single_call(ppf, oracle, built_lib, case_small):
    c = case_small
    par = fast_params(ppf)
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], ref_point_downsample_factor=2, params=par)
    mo = ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=par)
    T1 = mo.ppf_lookup(sc).copy()
    cells1 = mo.last_cells()[0]
    check_registration(ppf, oracle, mo, sc, c["mp"], c["mn"], c["sp"], c["sn"], c["d"], 2, 1, T1)
    parts, gmax = [], 0
    for rank in range(2):
        ps = fast_params(ppf, shard_rank=rank, shard_world=2)
        scs = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], ref_point_downsample_factor=2, params=ps)
        ms = ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=ps)
        loc, lmax = ms.align_local(scs, cap=1 << 16)
        parts.append(loc)
        gmax = max(gmax, lmax)
    T2 = ms.align_finish(sc, np.concatenate(parts), gmax)
    assert np.array_equal(T2, T1) and cells_equal(ms.last_cells()[0], cells1)


def _degenerate_cloud():
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (96, 3)).astype(np.float32)
    n = rng.normal(size=(96, 3)).astype(np.float32)
    p[10] = p[3]
    n[20:40] = np.float32([0.6, 0.0, 0.8])
    n[40:50] = np.float32([0.3, 0.1, 0.7])
    n[50] = 0
    p[60:70, 2] = 0
    n[60:70] = np.float32([0, 0, 1])
    p[70] = p[71] + np.float32([0, 0, 1e-7])
    return p, n


def test_degenerate_vectors_follow_the_stated_rule(ppf, oracle, built_lib, synth):
    """Coordinates of 2^45 and 2^-45 (every angle of the 2^45 cloud is degenerate) and the degenerate cloud of
    test_keys_with_degenerate_geometry: a degenerate vector counts as theta = 0 on either side, bit-exactly as the
    oracle states it."""
    cases = []
    for scale in (2.0 ** 45, 2.0 ** -45):
        c = make_case(synth, 90, 200, 2040)
        d = float(np.float32(c["d"]) * np.float32(scale))
        cases.append((c["mp"] * np.float32(scale), c["mn"], c["sp"] * np.float32(scale), c["sn"], d, (0, 57, 199)))
    p, n = _degenerate_cloud()
    cases.append((p, n, p, n, 0.07, tuple(range(0, 96, 5))))
    degenerate_votes = 0
    for mp, mn, sp, sn, d, refs in cases:
        par = fast_params(ppf)
        sc = ppf.Scene(sp, sn, d_dist=d, params=par)
        mo = ppf.Model(mp, mn, d_dist=d, params=par)
        fm = oracle.FusedModel(mp, mn, d)
        check_accumulators(mo, sc, fm, sp, sn, refs, 1)
        for r in refs:
            dv = fm.vote_dump(sp, sn, r)
            degenerate_votes += int(A.alpha64(dv["uy"], dv["uz"], dv["vy"], dv["vz"], 1)[1].sum())
        fm.close()
        T = mo.ppf_lookup(sc, allow_no_votes=True)
        check_registration(ppf, oracle, mo, sc, mp, mn, sp, sn, d, 1, 1, T if np.any(T) else None)
    assert degenerate_votes > 500               # 629 votes with a degenerate side in these reference points


def test_save_and_load(ppf, oracle, built_lib, case_small, tmp_path):
    c = case_small
    pf = fast_params(ppf)
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], params=pf)
    built = ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=pf)
    T0 = built.ppf_lookup(sc).copy()
    cells0 = built.last_cells()[0]
    check_registration(ppf, oracle, built, sc, c["mp"], c["mn"], c["sp"], c["sn"], c["d"], 1, 1, T0)
    refs = (0, 3, 250, 499)
    fm = oracle.FusedModel(c["mp"], c["mn"], c["d"])
    check_accumulators(built, sc, fm, c["sp"], c["sn"], refs, 1)
    fm.close()
    acc0 = [built.vote_accumulator(sc, r) for r in refs]
    # a fast model survives save / load
    f = str(tmp_path / "fast.oslam")
    built.save(f)
    loaded = ppf.Model.load(f)                  # the file's vote mode
    assert np.array_equal(loaded.ppf_lookup(sc), T0) and cells_equal(loaded.last_cells()[0], cells0)
    assert all(np.array_equal(loaded.vote_accumulator(sc, r), a) for r, a in zip(refs, acc0))
    # an exact-built file loaded with fast params votes like the fast-built model
    g = str(tmp_path / "exact.oslam")
    ppf.Model(c["mp"], c["mn"], d_dist=c["d"]).save(g)
    as_fast = ppf.Model.load(g, params=fast_params(ppf))
    assert all(np.array_equal(as_fast.vote_accumulator(sc, r), a) for r, a in zip(refs, acc0))
    assert np.array_equal(as_fast.ppf_lookup(sc), T0) and cells_equal(as_fast.last_cells()[0], cells0)
    # a fast file has no exact entries: loading it with exact params is refused
    with pytest.raises(ppf.OslamError) as e:
        ppf.Model.load(f, params=ppf.default_params())
    assert "fast" in str(e.value)
