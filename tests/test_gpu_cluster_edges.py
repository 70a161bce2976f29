"""GPU: the clustering scores the pose tails really compute, pose by pose, at their edges.

The suite saw k_cluster_scores (with k_cell_table_first / k_cell_table_end) and the chain of oslam_posegpu.hip
(k_pose_split, the packed-key sort, k_pose_cells, k_pose_gather, k_pose_best) only through the winning pose's matrix;
Model.last_result's scores are recomputed by the host loop.  Here Model.tail_scores (oslam_tail_scores) returns what a
NAMED tail computed -- 1: the host tail with k_cluster_scores behind the hook, 2: the device tail -- for the made-up
pose sets of cluster_inputs.py, each of which reaches one path of the kernels on purpose and asserts so from
reference-side data.  Kept cells, every score and the winner must equal the plain numpy reference (cluster_ref.py,
tied to the oracle in test_cluster_host.py) bit for bit, and the tail that ran must be the one asked for.

One-line mutations of the kernels that were tried against this module on a scratch copy, and what caught each:
  the pose's own cell searched too (no `lane != 13`)            nearly every case
  one-cell window test loosened by one (`<= incl + 1`)           windows_short_*
  `d_dist * d_dist` in place of dist2_below                      distance_0.100_l2, distance_0.333_l2
  whole_dev[1] ignored                                           order_sensitive, big_weight
  whole_dev[0]'s bound ignored (device tail)                     sum_bound
  whole_sum's bound ignored (the host hook)                      sum_bound
  a hash of 0 entered and searched                               zero_hash_*
  a group compares hashes only, not cells                        collision_*, zero_hash_one, stride
  compatible poses added in descending order                     order_sensitive, big_weight, order_wide_*
  k_cell_table_end one short                                     nearly every case
  `v < f` in the bpermute search                                 nearly every case
  a round of 4 x 64 skips the next window                        list_257_*, list_513_*
  the probe chain does not wrap / stops after two slots          probe_chains (the latter also windows_block_*, stride)
  the wave of four drops the list's last pose                    ragged_*, every n % 4 != 0
  k_pose_best prefers the last of equal scores                   most cases
  k_pose_best's per-thread loop takes `>=` (the grid stride)     stride
  the all-zero code gets the pose of (0, 0, 0)                   rotation_*
  pose_unpack keeps 24 bits of the count                         order_wide_0
`<` for `<=` in the one-cell window test changes nothing: such a window then takes the bpermute search, which places
the same 64 positions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_inputs as CI  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(CI.CASES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Rig:
    """one model per (d_dist, use_l1, two_sorts) -- pools and buffers are reused from case to case -- and one scene per case"""

    def __init__(self, ppf, oracle):
        self.ppf, self.oracle, self.models, self.scenes = ppf, oracle, {}, {}

    def pair(self, c):
        key = (c["d"], c["use_l1"], c["two_sorts"])
        if key not in self.models:
            self.models[key] = self.ppf.Model(c["mp"], c["mn"], d_dist=c["d"], vote_count_threshold=c["thresh"],
                                              use_l1_norm=c["use_l1"],
                                              params=self.ppf.default_params(pose_two_sorts=int(c["two_sorts"])))
        mo = self.models[key]
        mo.SetModelPointVoteWeights(c["weights"])
        if c["name"] not in self.scenes:
            self.scenes[c["name"]] = self.ppf.Scene(c["sp"], c["sn"], d_dist=c["d"], ref_point_downsample_factor=1)
        return mo, self.scenes[c["name"]]

    def check(self, name, path):
        c = CI.get_case(name, self.oracle)
        ref = c["ref"]
        mo, sc = self.pair(c)
        kept, scores, best, T, ran = mo.tail_scores(sc, c["records"], c["gmax"], path)
        assert ran == path, "%s: asked for tail %d, tail %d made the scores" % (name, path, ran)
        assert np.array_equal(kept["code"], ref["kept"]["code"]) and np.array_equal(kept["count"], ref["kept"]["count"]), (name, path)
        bad = np.nonzero(bits(scores) != bits(c["scores"]))[0]
        assert len(bad) == 0, "%s path %d: %d scores differ, first at pose %d: %r != %r" % (
            name, path, len(bad), bad[0], scores[bad[0]], c["scores"][bad[0]])
        assert best == c["best"], (name, path, best, c["best"])
        assert np.array_equal(T.reshape(16), ref["T"][c["best"]]), (name, path)


@pytest.fixture(scope="module")
def rig(ppf, oracle, built_lib):
    return Rig(ppf, oracle)


@pytest.mark.parametrize("name", NAMES)
def test_tail_scores_equal_the_reference(rig, name):
    for path in (1, 2, 0):
        rig.check(name, path)


def test_pools_grow_shrink_and_alternate(rig):
    """a large set, a small one, the large one again on the same model: the pose pool and the cluster buffer grow and
    are reused; then the two device paths right after one another, both ways round"""
    for path in (2, 1):
        for name in ("best_blocks", "ragged_5_one", "best_blocks", "list_513_one", "ragged_2_one"):
            rig.check(name, path)
    for path in (1, 2, 2, 1, 1, 2):
        rig.check("windows_straddle_one", path)
        rig.check("groups_one", 3 - path)


def test_a_tail_that_cannot_run_says_so(rig, ppf):
    """one kept cell: the device tail leaves it to the host and the tap reports that instead of a path it did not run"""
    c = CI.get_case("ragged_2_one", rig.oracle)
    mo, sc = rig.pair(c)
    with pytest.raises(ppf.OslamError):
        mo.tail_scores(sc, c["records"][:1], c["gmax"], 2)
    kept, scores, best, T, ran = mo.tail_scores(sc, c["records"][:1], c["gmax"], 1)
    assert ran == 0 and len(kept) == 1
