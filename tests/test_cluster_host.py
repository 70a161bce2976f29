"""CPU: the plain reference of the pose tail's clustering scores (cluster_ref.py) tied to the oracle pose by pose, and the
host loop (the tap's path 0: filter, order, oslam_pose_stage_ex) tied to that reference, on every made-up pose set of
cluster_inputs.py.  The GPU test (test_gpu_cluster_edges.py) runs the same sets through the two device paths.

Everything is bit-exact by design; no tolerance anywhere.

The distance cases: the issue asked for d_dist values whose threshold (the smallest float whose root reaches d_dist)
lies below, on and ABOVE fl(d_dist^2).  The third kind does not exist (cluster_inputs.pick_distances gives the
argument and checks it on the candidates 0.1, 0.25, 0.3, 1/3, 0.7: kinds -1, 0, 0, -1, -1); the cases use 0.1 and 1/3
(below) and 0.25 (on)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_inputs as CI  # noqa: E402
import cluster_ref as R  # noqa: E402

NAMES = list(CI.CASES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fnv_transcription_and_the_named_cells(oracle):
    cells = np.asarray(CI.ZERO_HASH_CELLS + [c for p in CI.COLLISIONS for c in p] + [(0, 0, 0), (-1, 2, -3)], np.int32)
    h = R.fnv_cells(cells)
    for c, v in zip(cells, h):
        assert oracle.hash_bytes(c.tobytes()) == int(v)
    assert (h[:3] == 0).all() and h[3] == h[4] and h[5] == h[6] and h[3] != h[5]
    assert CI.pick_distances() == [float(np.float32(v)) for v in (0.1, 0.25, 1.0 / 3.0)]


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_oracle_and_host_loop_equals_reference(ppf, oracle, built_lib, name):
    c = CI.get_case(name, oracle)
    ref = c["ref"]
    if (c["weights"] == 1).all():
        best, scores, _ = oracle.cluster_gpu_style(ref["kept"], ref["trans"], ref["quat"], c["d"], use_l1_norm=c["use_l1"])
        assert np.array_equal(bits(scores), bits(c["scores"])) and best == c["best"]
    kept, scores, best, T = CI.host_tail_scores(ppf, c)
    assert np.array_equal(kept["code"], ref["kept"]["code"]) and np.array_equal(kept["count"], ref["kept"]["count"])
    assert np.array_equal(bits(scores), bits(c["scores"]))
    assert best == c["best"]
    assert np.array_equal(T.reshape(16), ref["T"][c["best"]])


def test_both_window_kinds_and_both_modes_occur(oracle):
    """over the window cases: windows that lie in one cell (the readlane path) and windows that straddle (the bpermute
    search); over all cases: whole and sequential mode"""
    kinds = set()
    for name in ("windows_straddle_one", "windows_exact_one", "windows_block_one", "list_513_one"):
        ref = CI.get_case(name, oracle)["ref"]
        for i in range(len(ref["kept"])):
            for w in CI.windows(CI.list_lens(ref, i)):
                kinds.add("one" if w["one_cell"] else "straddle%d" % min(w["spans"], 3))
    assert kinds >= {"one", "straddle2", "straddle3"}
    modes = {CI.whole_mode(CI.get_case(n, oracle)["ref"]) for n in NAMES if n != "stride"}
    assert modes == {True, False}
