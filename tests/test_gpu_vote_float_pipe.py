"""The vote kernels compute the LDS address of a vote, row address + 4 * bin, with v_fma_f32 on bit patterns below 2^23
(VoteRegs::vote in oslam_vote_body.inc).  These tests aim at where that arithmetic could go wrong: the largest
addresses, both halves of a counter word, the first and the last bin, the second slice, a database group, and the wide
passes with their increments of 0 and 1.  All against the CPU oracle."""
import numpy as np
import pytest

from conftest import cells_equal, make_case

pytestmark = pytest.mark.gpu

# First and last rows of slice 0 in both halves of a counter word under either row mapping (row = point, half = point
# / 1023; or row = point / 2, half = point % 2), and the first and last point of slice 1 (2046 points per slice).
EDGE_POINTS = (0, 1, 1022, 1023, 2044, 2045, 2046, 2299)
# At scene reference point 0 model point 1 has no vote in bin 0; reference point 12 is the first one with more than a
# handful of votes in bins 0 and 29 of all eight points (found with the oracle on the CPU: 8, 12 and 15 qualify).
EDGE_REF = 12
STAT_KEYS = ("num_votes", "num_unique_votes", "max_count", "num_top")


@pytest.fixture(scope="module")
def edge_oracle(oracle, case_two_slices):
    c = case_two_slices
    fm = oracle.FusedModel(c["mp"], c["mn"], c["d"])
    want = {mode: fm.accumulator(c["sp"], c["sn"], EDGE_REF, vote_mode=mode) for mode in (0, 1)}
    fm.close()
    for a in want.values():
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
def test_edge_rows_and_bins_one_model(ppf, built_lib, case_two_slices, edge_oracle, mode):
    """2300 model points (two slices) at one scene reference point: the dense accumulator equals the oracle's word
    for word, and the oracle's says that the cells at the edges of the address range are in use."""
    c, want = case_two_slices, edge_oracle[mode]
    for p in EDGE_POINTS:
        assert want[p, 0] > 0 and want[p, 29] > 0, p
    assert not want[:, 30:].any()
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=c["d"])
    mo = ppf.Model(c["mp"], c["mn"], d_dist=c["d"], params=ppf.default_params(vote_mode=mode))
    got = mo.vote_accumulator(sc, EDGE_REF)
    mo.close()
    sc.close()
    assert not got[:, 30:].any()
    assert np.array_equal(got, want)


def test_edge_rows_and_bins_database_group(ppf, oracle, built_lib, synth):
    """Two members of unequal size voted in one grid (k_vote_group): each member's peak cells and counters equal what
    it gives alone and what the oracle gives."""
    c = make_case(synth, 300, 900, 2031)
    c2 = make_case(synth, 170, 900, 2031, model_id=1)
    df = 3
    sc = ppf.Scene(c["sp"], c["sn"], d_dist=0.0, ref_point_downsample_factor=df)
    clouds = [(c["mp"], c["mn"]), (c2["mp"], c2["mn"])]
    models = [ppf.Model(p, n, d_dist=c["d"]) for p, n in clouds]
    alone = []
    for m in models:
        m.ppf_lookup(sc, allow_no_votes=True)
        alone.append((m.last_cells()[0], {k: m.stats[k] for k in STAT_KEYS}))
    db = ppf.Database(models)
    assert db.n_groups == 1
    _, stats = db.align(sc)
    for j, (p, n) in enumerate(clouds):
        cells, st = models[j].last_cells()[0], {k: stats[j][k] for k in STAT_KEYS}
        assert cells_equal(cells, alone[j][0]) and st == alone[j][1], j
        ocells, ost = oracle.votes_fused(p, n, c["sp"], c["sn"], df, c["d"], 0.4)
        assert cells_equal(cells, ocells), j
        assert st == {k: ost[k] for k in STAT_KEYS}, j
        assert st["num_votes"] > 0
    db.close()
    for m in models:
        m.close()
    sc.close()


def _arc_cloud(n, rng, spread=0.15):
    """A point at the origin and n points on a short arc of radius 1 around it, all normals +z: every (origin, arc)
    pair has the same key and nearly the same in-plane angle."""
    a = rng.uniform(-spread, spread, n)
    p = np.zeros((n + 1, 3), np.float32)
    p[1:, 0] = np.cos(a)
    p[1:, 1] = np.sin(a)
    p[1:, 2] = rng.uniform(-1e-3, 1e-3, n)
    return p, np.tile(np.float32([0, 0, 1]), (n + 1, 1))


def test_wide_passes_still_add_zero_and_one(ppf, oracle, built_lib):
    """Arc clouds put 2.8e5 votes into single cells, so the workgroup is voted again with 32-bit counters, one half of
    the slice at a time (increments 0 and 1); 1040 filler points in front put the overflowing rows into the upper half
    of a word.  The accumulator still equals the oracle's, and the statistics say that the wide passes ran."""
    rng = np.random.default_rng(5)
    mp, mn = _arc_cloud(159, rng)
    sp, sn = _arc_cloud(2999, rng)
    fp = rng.uniform(5, 6, (1040, 3)).astype(np.float32)
    fn = rng.normal(size=(1040, 3)).astype(np.float32)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    mp, mn = np.concatenate([fp, mp]), np.concatenate([fn, mn])
    d = 0.3
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=3000)
    mo = ppf.Model(mp, mn, d_dist=d)
    acc = mo.vote_accumulator(sc, 0)
    assert acc.max() > 3 * 65535
    assert np.array_equal(acc, oracle.accumulator_for_ref(mp, mn, sp, sn, 0, d))
    mo.ppf_lookup(sc)
    assert mo.stats["wide_workgroups"] > 0 and mo.stats["max_count"] > 3 * 65535
    mo.close()
    sc.close()
