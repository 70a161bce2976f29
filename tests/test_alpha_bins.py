"""CPU: the oracle's alpha bins of real clouds against the float64 statement of tests/alpha_ref.py.

DESIGN.md section 5 bounds the float32 error of the reference's alpha by 2e-5 bin and fast mode's by the bound of
include/oslam.h (OSLAM_VOTE_FAST); math_exhaustive checks both on samples, this file on every vote of 100 reference
points of a registration (2e6 votes)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_ref as A  # noqa: E402
from test_refine_host import make_trial  # noqa: E402

EXACT_BOUND = 2e-5
FAST_BOUND = 3.1e-5        # include/oslam.h, ppf_core.h: PC_FAST_BOUND
MARGIN = 64 * 30 / 2 ** 24  # the re-evaluation margin of exact mode (1.14e-4 bin)


@pytest.fixture(scope="module")
def trial12(synth, oracle):
    mp, mn, d, sp, sn, _ = make_trial(synth, 600, 3000, 12, 0.1, 0.0)
    fm = oracle.FusedModel(mp, mn, d)
    yield dict(mp=mp, mn=mn, d=d, sp=sp, sn=sn, fm=fm, refs=range(0, 3000, 30))
    fm.close()


def test_oracle_bins_of_real_clouds_within_the_float64_bound(trial12):
    c, fm = trial12, trial12["fm"]
    votes = near = 0
    for r in c["refs"]:
        ex = fm.vote_dump(c["sp"], c["sn"], r, vote_mode=0)
        fa = fm.vote_dump(c["sp"], c["sn"], r, vote_mode=1)
        for k in ("m_r", "uy", "uz", "vy", "vz"):
            assert np.array_equal(ex[k], fa[k]), k            # one set of operands, two statements of the bin
        x, deg = A.alpha64(ex["uy"], ex["uz"], ex["vy"], ex["vz"], 0)
        bad, _, _ = A.bin_errors(ex["bin"], x, deg, EXACT_BOUND)
        assert len(bad) == 0, (r, bad[:5], x[bad[:5]], ex["bin"][bad[:5]])
        xf, degf = A.alpha64(fa["uy"], fa["uz"], fa["vy"], fa["vz"], 1)
        bad, _, _ = A.bin_errors(fa["bin"], xf, degf, FAST_BOUND)
        assert len(bad) == 0, (r, bad[:5], xf[bad[:5]], fa["bin"][bad[:5]])
        votes += len(x)
        near += int(A.below_edge(x, 1.3e-4).sum())
    # enough votes, and enough of them just below an edge, that a base shifted by the margin would show
    assert votes >= 10 ** 6 and near >= 20, (votes, near)


def test_interval_check_of_oracle_accumulators_and_its_teeth(trial12):
    c, fm = trial12, trial12["fm"]
    for r in (0, 1470, 2970):
        ex = fm.vote_dump(c["sp"], c["sn"], r, vote_mode=0)
        ops = (ex["m_r"], ex["uy"], ex["uz"], ex["vy"], ex["vz"])
        acc = fm.accumulator(c["sp"], c["sn"], r, vote_mode=0)
        assert A.interval_check(acc, *ops, EXACT_BOUND, vote_mode=0, exact_bins=ex["bin"]) == []
        accf = fm.accumulator(c["sp"], c["sn"], r, vote_mode=1)
        assert A.interval_check(accf, *ops, FAST_BOUND, vote_mode=1) == []
        # the votes a base shifted by the margin moves into the next bin: the check must see them
        x, _ = A.alpha64(ex["uy"], ex["uz"], ex["vy"], ex["vz"], 1)
        b, _, d = A.edges(x)
        mv = A.below_edge(x, MARGIN) & (d > FAST_BOUND)
        assert mv.any(), r
        shifted = accf.astype(np.int64)
        np.add.at(shifted, (ex["m_r"][mv].astype(np.int64), b[mv] % 30), -1)
        np.add.at(shifted, (ex["m_r"][mv].astype(np.int64), (b[mv] + 1) % 30), 1)
        assert A.interval_check(shifted, *ops, FAST_BOUND, vote_mode=1) != []


def test_degenerate_votes_follow_the_stated_rule():
    # a zero vector on either side counts as theta = 0 in fast mode: alpha + pi = theta_v - theta_u + pi
    uy = np.float32([0.0, 1.0, 0.0, 2.0 ** 50])
    uz = np.float32([0.0, 0.0, 0.0, 0.0])
    vy = np.float32([0.0, 0.0, 1.0, 1.0])
    vz = np.float32([1.0, 0.0, 1.0, 0.0])
    x, deg = A.alpha64(uy, uz, vy, vz, 1)
    assert deg.tolist() == [True, True, True, True]
    # theta_v - theta_u with theta = atan2(z, y) + pi, 0 on a degenerate side: u zero and v = (0, 1); v zero and
    # u = (1, 0); u zero and v = (1, 1); u beyond 2^40 and v = (1, 0)
    want = np.mod(np.array([1.5 * np.pi, -np.pi, 1.25 * np.pi, np.pi]) + np.pi, 2 * np.pi) / A.D32
    assert np.allclose(x, want, rtol=0, atol=1e-9)
    xe, _ = A.alpha64(uy, uz, vy, vz, 0)
    assert np.isnan(xe).all()                  # exact mode: the reference's float32 sequence decides
