"""CPU: the inputs of tests/refine_edge_inputs.py reach the paths they are named for, asserted on the restatement alone
(refine_ref), so that tests/test_gpu_refine_edges.py cannot pass on inputs that miss their path; and the wrong rules a
kernel could follow instead differ from the right one on these inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_edge_inputs as X  # noqa: E402
import refine_ref as R  # noqa: E402

F = np.float32


@pytest.mark.parametrize("name", list(X.GRID_CASES))
def test_grid_cases_have_their_shape(synth, name):
    c = X.grid_case(synth, name)
    s, want = c["shape"], c["want"]
    assert {k: s[k] for k in want} == want, (name, s)
    assert s["nb"] == (s["n_cells"] + 1 + 4095) // 4096 and s["per"] == (s["nb"] + 1023) // 1024
    assert len(c["sp"]) == X.GRID_POINTS and np.allclose(np.linalg.norm(c["sn"], axis=1), 1.0, atol=1e-6)
    assert (s["lo"] == 0.0).all()                                        # the corners alone decide the box
    cells = R.cell_index(c["sp"], s)
    raw = R.cell_of(c["sp"], s)
    assert (raw >= 0).all() and (raw < np.asarray(s["dims"])).all()      # no scene point needs the clamp
    held = set(int(x) for x in cells)
    assert all(any(first <= x <= last for x in held) for first, last in c["blocks"][:3] + c["blocks"][-3:])
    occupied = np.zeros(s["nb"], bool)
    occupied[cells // R.SCAN_ITEMS] = True
    assert occupied[:len(c["blocks"])].all() and len(c["blocks"]) in (s["nb"], s["nb"] - 1)
    for b in set(k for k in X.GRID_BLOCKS if k < len(c["blocks"])) | {len(c["blocks"]) - 1}:
        assert c["blocks"][b][0] in held and c["blocks"][b][1] in held, (name, b)
    if s["n_cells"] > 1:
        assert (np.diff(cells) < 0).sum() > 1000                         # index order is not cell order
    for pname, T in c["poses"].items():
        q, m = R.transform_f32(T, c["sp"], c["sn"])
        want_idx, _ = R.correspondences(q, m, c["sp"], c["sn"], c["radius"], 0.8)
        assert (want_idx >= 0).all(), (name, pname)                      # every model point finds an index
        walked, _ = R.grid_walk(q, m, c["sp"], c["sn"], c["radius"], 0.8, s)
        assert np.array_equal(walked, want_idx), (name, pname)           # the grid's walk is the brute force
    if name == X.CLAMPED:
        kw, radius = X.clamped_call(c)
        again = R.grid_shape(c["sp"], radius)
        # what scene_grid's cache tests: the edge of the clamped grid lies above twice its radius
        assert again["clamped"] and again["per"] == 4 and again["edge"] > 2.0 * radius
        assert kw["inlier_dist"] <= kw["max_corr_dist"]


def test_tie_lattice_ties_span_cells_and_walk_order(synth):
    sp, sn, copy = X.tie_scene(synth)
    q, m, kind = X.tie_queries()
    shape = R.grid_shape(sp, X.H)
    assert shape["dims"] == (8, 8, 8) and len(sp) == X.LATTICE_N ** 3 + X.N_DUPLICATES and (kind == 8).sum() == 512
    cells = R.cell_index(sp, shape)
    d = sp[None, ~copy, :] - q[kind == 8][:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    tied = d2 == d2.min(axis=1)[:, None]
    assert (tied.sum(axis=1) == 8).all() and (d2.min(axis=1) == F(3.0) * F(X.H / 2) * F(X.H / 2)).all()     # 8-way, exact
    spans = np.array([len(set(cells[~copy][row])) for row in tied])
    print("cells spanned by the 8 tied points of the 512 centres: %s" % dict(zip(*np.unique(spans, return_counts=True))))
    assert (spans >= 2).sum() >= 490 and dict(zip(*np.unique(spans, return_counts=True))) == {1: 1, 2: 21, 4: 147, 8: 343}
    for pname, T in X.tie_poses().items():
        qq, mm = R.transform_f32(T, q, m)
        assert np.array_equal(qq, (q.astype(np.float64) + T[:3, 3].astype(np.float64)).astype(np.float32))   # exact
        by_gate = {}
        for gate in X.GATES:
            want, _ = R.correspondences(qq, mm, sp, sn, X.H, gate)
            walked, first = R.grid_walk(qq, mm, sp, sn, X.H, gate, shape)
            assert np.array_equal(walked, want)
            assert ((first != want) & (want >= 0)).sum() >= 100, pname   # the winner is often not the first tied point met
            wrong, _ = R.grid_walk(qq, mm, sp, sn, X.H, gate, shape, rule="first")
            assert not np.array_equal(wrong, want)                       # first-met instead of lowest index
            by_gate[gate] = want
        # the copies decide through the normal gate: a copy with the lowest index wins at -2 and fails 0.8
        differ = by_gate[0.8] != by_gate[-2.0]
        assert differ.any() and copy[by_gate[-2.0][differ]].all() and (sn[by_gate[-2.0][differ], 2] < F(0.8)).all()
        assert copy[by_gate[0.8][by_gate[0.8] >= 0]].any()               # and copies that pass it win elsewhere


def test_face_queries_reach_the_ball_and_every_cell_class(synth):
    sp, sn, _ = X.tie_scene(synth)
    q, m, labels = X.face_queries()
    shape = R.grid_shape(sp, X.H)
    want, d2 = R.correspondences(q, m, sp, sn, X.H, -2.0)
    r2 = F(X.H) * F(X.H)
    for (what, off), idx, dd in zip(labels, want, d2):
        if what.startswith("face"):
            assert (idx >= 0) == (off in ("0.5 r", "r")), (what, off)
            if off == "r":
                assert dd == r2                                          # exactly on the closed ball
        else:
            assert (idx >= 0) == (off == "0.5 r"), (what, off)
    cq = R.cell_of(q, shape)
    for a in range(3):
        dim = shape["dims"][a]
        assert {-2, -1, 0, dim - 1, dim, dim + 1} <= set(int(x) for x in cq[:, a]), (a, sorted(set(cq[:, a])))
    walked, _ = R.grid_walk(q, m, sp, sn, X.H, -2.0, shape)
    assert np.array_equal(walked, want)
    open_ball, _ = R.grid_walk(q, m, sp, sn, X.H, -2.0, shape, rule="open")           # < instead of <=
    on_ball = np.array([w.startswith("face") and off == "r" for w, off in labels])
    assert (open_ball[on_ball] == -1).all() and np.array_equal(open_ball[~on_ball], want[~on_ball]) and on_ball.sum() == 18
    inside, _ = R.grid_walk(q, m, sp, sn, X.H, -2.0, shape, rule="inside")            # no walk from cell -1 or dim
    assert (inside == -1).all() and (want >= 0).sum() == 18 * 2 + 8
    for pname, T in X.face_poses().items():
        if pname == "identity":
            continue
        qq, mm = R.transform_f32(T, q, m)
        with np.errstate(all="ignore"):
            far, _ = R.correspondences(qq, mm, sp, sn, X.H, -2.0)
        cf = R.cell_of(qq, shape)
        assert (far == -1).all() and np.isfinite(qq).all(), pname
        assert all(((cf[:, a] == -2) | (cf[:, a] == shape["dims"][a] + 1)).all() for a in range(3) if T[a, 3] != 0), pname


def test_block_sums_are_sums():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 5000):
        t = rng.integers(-40, 40, (n, 3)).astype(np.float32)
        b = R.block_sums_f32(t)
        assert b.dtype == np.float32 and b.shape == ((n + 255) // 256, 3)
        pad = np.zeros((len(b) * 256, 3))
        pad[:n] = t
        assert np.array_equal(b, pad.reshape(len(b), 256, 3).sum(axis=1))
        assert np.array_equal(R.member_sums(t), t.astype(np.float64).sum(axis=0))
    ones = np.ones((70000, 1), np.float32)
    assert np.array_equal(R.member_sums(ones), [70000.0]) and (R.block_sums_f32(ones)[:-1] == 256).all()


def test_members_stop_step_converge_and_pin_the_sum_order(synth):
    c = X.member_case(synth)
    a64, a32 = X.member_answers(synth, 30, "f64"), X.member_answers(synth, 30, "f32")
    kinds = [k for _, k in X.MEMBERS]
    zero = [j for j, k in enumerate(kinds) if k == "zero"]
    live = [j for j, k in enumerate(kinds) if k != "zero"]
    assert len(zero) == 2 and all(min(live) < j < max(live) for j in zero) and not c["T_in"][zero].any()
    assert all(a64[j] is None for j in zero)
    stopped = [j for j in live if a32[j][1]["iterations"] == 0 and 0 < a32[j][1]["correspondences"] < 6]
    stepped = [j for j in live if a32[j][1]["iterations"] >= 1]
    # a member that steps and then loses its correspondences inside the call, while the others go on
    lost = [j for j in stepped if a32[j][1]["correspondences"] < 6]
    assert len(stopped) >= 1 and len(stepped) >= 10 and len(lost) >= 1, (stopped, stepped, lost)
    at_truth, far = kinds.index("truth"), kinds.index("far")
    slowest = max(a32[j][1]["iterations"] for j in stepped)
    assert a32[at_truth][1]["converged"] and a32[at_truth][1]["iterations"] <= slowest - 4, (a32[at_truth][1], slowest)
    assert slowest > 4                                                  # past the first read of the "all done" word
    assert a32[far][1]["correspondences"] == 0 and a32[far][1]["iterations"] == 0 and a32[far][1]["fitness"] == 0.0
    assert np.array_equal(a32[far][0], c["T_in"][far])
    held = []
    for j in live:
        (W64, w64), (W32, w32) = a64[j], a32[j]
        s_ang, s_dt = R.pose_error(W32, W64)
        print("member %2d n %4d %-5s: iterations %d / %d, correspondences %d / %d, cond %.3e, spread of the final pose float32 "
              "sums vs float64 %.3e deg %.3e d_dist" % (j, X.MEMBERS[j][0], kinds[j], w32["iterations"], w64["iterations"],
                                                        w32["correspondences"], w64["correspondences"], w32["cond"], s_ang,
                                                        s_dt / c["d"]))
        assert abs(w32["iterations"] - w64["iterations"]) <= 1 and w32["fitness_in"] == float(F(w64["fitness_in"]))
        if j in stepped and w32["cond"] <= X.COND_BITS:
            held.append(j)
    assert tuple(held) == X.BITS_HELD, held
    # plain index-order float32 sums instead of the tree: the 29 sums of a first step differ in bits
    differ = 0
    for j in stepped:
        n = X.MEMBERS[j][0]
        terms, ok = R.terms_at(c["mp"][:n], c["mn"][:n], c["sp"], c["sn"], c["T_in"][j], c["d"])
        pad = np.zeros(((n + 255) // 256 * 256, terms.shape[1]), np.float32)
        pad[:n] = terms
        plain = np.cumsum(pad.reshape(-1, 256, terms.shape[1]), axis=1, dtype=np.float32)[:, -1]
        tree = R.block_sums_f32(terms)
        assert tree[:, 27].sum() == ok.sum() == plain[:, 27].sum()
        differ += plain.tobytes() != tree.tobytes()
    assert differ >= 1
    # the other schedules of the GPU test: one step, and either side of the host's read after 4 iterations
    for max_it in X.MEMBER_SCHEDULES[1:]:
        for j, got in enumerate(X.member_answers(synth, max_it, "f32")):
            if got is not None:
                assert got[1]["iterations"] == min(max_it, a32[j][1]["iterations"]), (max_it, j)
