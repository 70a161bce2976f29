"""GPU: the refinement stage at its edges (inputs: tests/refine_edge_inputs.py; tests/test_refine_edge_inputs.py shows on
the CPU that they reach their paths) against the numpy restatement of tests/refine_ref.py: the scene grid's scan on the
borders of its two levels and on the cell limit, exact ties across cells, the closed ball and the cells outside the box,
the grid cache, and the members of one database call against their single calls and the sums="f32" restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_edge_inputs as X  # noqa: E402
import refine_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
DYN = ("launches", "ms_total")
GRID_SLOTS = 4                  # oslam_refine.c
BUILD_LAUNCHES = 5              # include/oslam.h at oslam_refine_result: what a call that builds the scene grid adds to `launches`


def plain(res):
    return {k: v for k, v in res.items() if k not in DYN}


def assert_taps_equal(ppf, model, scene, mp, mn, sp, sn, T, radius, gates=X.GATES):
    """refine_correspondences twice per gate: equal bytes, and the restatement's indices.  -> {gate: indices}"""
    q, m = R.transform_f32(T, mp, mn)
    out = {}
    for gate in gates:
        got = ppf.refine_correspondences(model, scene, T, radius, gate)
        again = ppf.refine_correspondences(model, scene, T, radius, gate)
        with np.errstate(all="ignore"):
            want, _ = R.correspondences(q, m, sp, sn, radius, gate)
        assert got.tobytes() == again.tobytes(), (radius, gate)
        assert np.array_equal(got, want), (radius, gate, np.flatnonzero(got != want)[:8])
        out[gate] = got
    return out


@pytest.mark.parametrize("name", list(X.GRID_CASES))
def test_grid_cases_equal_brute_force(built_lib, ppf, synth, name):
    c = X.grid_case(synth, name)
    sp, sn = c["sp"], c["sn"]
    model = ppf.Model(sp, sn, d_dist=c["d"])
    scene = ppf.Scene(sp, sn, d_dist=0.0)
    _, first, count = np.unique(sp, axis=0, return_index=True, return_counts=True)
    alone = np.zeros(len(sp), bool)
    alone[first[count == 1]] = True
    for pname, T in c["poses"].items():
        got = assert_taps_equal(ppf, model, scene, sp, sn, sp, sn, T, c["radius"])
        for gate, idx in got.items():
            assert (idx >= 0).all(), (name, pname, gate)                 # every model point finds an index
            if pname == "identity":                                      # itself, or the first of its exact copies
                me = np.arange(len(sp))
                assert np.array_equal(sp[idx], sp) and (idx <= me).all() and np.array_equal(idx[alone], me[alone])
    model.close()
    scene.close()


def test_tie_lattice_and_face_queries_equal_brute_force(built_lib, ppf, synth):
    sp, sn, _ = X.tie_scene(synth)
    scene = ppf.Scene(sp, sn, d_dist=0.0)
    q, m, kind = X.tie_queries()
    model = ppf.Model(q, m, d_dist=X.H)
    for pname, T in X.tie_poses().items():
        got = assert_taps_equal(ppf, model, scene, q, m, sp, sn, T, X.H)
        assert (got[-2.0] >= 0).sum() >= 3000 and not np.array_equal(got[0.8], got[-2.0]), pname
    model.close()
    fq, fm, labels = X.face_queries()
    model = ppf.Model(fq, fm, d_dist=X.H)
    for pname, T in X.face_poses().items():
        got = assert_taps_equal(ppf, model, scene, fq, fm, sp, sn, T, X.H)
        if pname == "identity":
            for (what, off), idx in zip(labels, got[-2.0]):
                assert (idx >= 0) == (off == "0.5 r" or (off == "r" and what.startswith("face"))), (what, off, idx)
        else:
            assert (got[0.8] == -1).all() and (got[-2.0] == -1).all(), pname           # translations of 1e30 and 3e38
    model.close()
    scene.close()


def test_grid_cache_serves_and_evicts(built_lib, ppf, synth):
    """Five radii on one scene, each more than twice the last (one more than GRID_SLOTS), then the first again: every
    result is exact whichever slot was rebuilt.  In Model.refine a call whose radius a cached grid serves enqueues
    BUILD_LAUNCHES fewer launches than the one that built it."""
    c = X.member_case(synth)
    mp, mn = c["mp"][:513], c["mn"][:513]
    model = ppf.Model(mp, mn, d_dist=c["d"])
    scene = ppf.Scene(c["sp"], c["sn"], d_dist=0.0)
    T = c["truth"].astype(np.float32)
    assert len(X.CACHE_RADII) == GRID_SLOTS + 2 and all(b > 2 * a for a, b in zip(X.CACHE_RADII[:-2], X.CACHE_RADII[1:-1]))
    for k in X.CACHE_RADII:
        got = assert_taps_equal(ppf, model, scene, mp, mn, c["sp"], c["sn"], T, k * c["d"])
        assert (got[0.8] >= 0).sum() >= 500
    scene.close()
    scene = ppf.Scene(c["sp"], c["sn"], d_dist=0.0)
    launches = []
    for mcd in (2.0, 2.0, 1.3, 0.4, 1.3):                # builds; the same radius; a smaller one it serves; a new grid; served
        par = ppf.default_refine_params(max_iterations=1, max_corr_dist=mcd, inlier_dist=0.25)
        launches.append(model.refine(scene, T, par)[1]["launches"])
    assert launches == [4 + BUILD_LAUNCHES, 4, 4, 4 + BUILD_LAUNCHES, 4], launches
    model.close()
    scene.close()


def test_clamped_grid_is_cached(built_lib, ppf, synth):
    """The grid of the clamped case has an edge above twice its radius (asserted on the CPU).  The call that repeats its
    radius must find it: it enqueues BUILD_LAUNCHES fewer launches and leaves the other slots alone."""
    c = X.grid_case(synth, X.CLAMPED)
    kw, radius = X.clamped_call(c)
    model = ppf.Model(c["sp"], c["sn"], d_dist=c["d"])
    scene = ppf.Scene(c["sp"], c["sn"], d_dist=0.0)
    T = np.eye(4, dtype=np.float32)
    other = ppf.default_refine_params(max_iterations=1, max_corr_dist=float(F(0.01 / c["d"])), inlier_dist=float(F(0.005 / c["d"])))
    par = ppf.default_refine_params(**kw)
    seen = [model.refine(scene, T, p)[1] for p in (other, par, par, other, par)]
    assert [r["launches"] for r in seen] == [4 + BUILD_LAUNCHES, 4 + BUILD_LAUNCHES, 4, 4, 4], [r["launches"] for r in seen]
    assert plain(seen[1]) == plain(seen[2]) == plain(seen[4]) and seen[1]["inliers"] == len(c["sp"]), seen[1]
    q, m = R.transform_f32(T, c["sp"], c["sn"])
    assert np.array_equal(ppf.refine_correspondences(model, scene, T, radius, 0.8),
                          R.correspondences(q, m, c["sp"], c["sn"], radius, 0.8)[0])
    model.close()
    scene.close()


@pytest.fixture(scope="module")
def members(built_lib, ppf, synth):
    c = X.member_case(synth)
    models = [ppf.Model(c["mp"][:n], c["mn"][:n], d_dist=c["d"]) for n, _ in X.MEMBERS]
    db = ppf.Database(models)
    scene = ppf.Scene(c["sp"], c["sn"], d_dist=0.0)
    yield dict(c, models=models, db=db, scene=scene)
    db.close()
    scene.close()
    for m in models:
        m.close()


@pytest.mark.parametrize("max_it", X.MEMBER_SCHEDULES)
def test_members_of_one_call(ppf, synth, members, max_it):
    c = members
    d, sp, sn = c["d"], c["sp"], c["sn"]
    par = ppf.default_refine_params(max_iterations=max_it)
    Td, res, found = c["db"].refine(c["scene"], c["T_in"], par)
    a64, a32 = X.member_answers(synth, max_it, "f64"), X.member_answers(synth, max_it, "f32")
    p = R.default_params()
    stopped = stepped = held = 0
    for j, (n, kind) in enumerate(X.MEMBERS):
        mp, mn = c["mp"][:n], c["mn"][:n]
        if kind == "zero":
            assert not Td[j].any() and not found[j] and res[j]["iterations"] == 0 and res[j]["fitness"] == 0, (j, res[j])
            assert res[j]["correspondences"] == 0 and res[j]["inliers"] == 0 and res[j]["fitness_in"] == 0, (j, res[j])
            continue
        Ts, rs = c["models"][j].refine(c["scene"], c["T_in"][j], par)
        assert Ts.tobytes() == Td[j].tobytes() and plain(rs) == plain(res[j]), (j, rs, res[j])
        (W64, w64), (W32, w32) = a64[j], a32[j]
        # the score of the device's own pose: fitness, inliers and rmse bit for bit
        fit, n_in, rmse = R.score(mp, mn, sp, sn, Td[j], F(p["inlier_dist"]) * F(d), p["min_normal_dot"], sums="f32")
        print("member %2d n %4d %-5s max_it %2d: iterations %d / %d, correspondences %d / %d, fitness %.6f / %.6f, rmse %.6e / %.6e, "
              "pose bits %s" % (j, n, kind, max_it, res[j]["iterations"], w32["iterations"], res[j]["correspondences"],
                                w32["correspondences"], res[j]["fitness"], fit, res[j]["rmse"], rmse,
                                "equal" if Td[j].tobytes() == W32.tobytes() else "differ"))
        assert (F(res[j]["fitness"]), res[j]["inliers"], F(res[j]["rmse"])) == (F(fit), n_in, F(rmse)), (j, res[j], fit, n_in, rmse)
        assert F(res[j]["fitness_in"]) == F(w32["fitness_in"]), (j, res[j], w32)
        if w32["iterations"] == 0:
            # fewer than 6 correspondences stop the first step: T_in comes back bit for bit
            assert w32["correspondences"] < 6 and res[j]["iterations"] == 0 and not res[j]["converged"], (j, res[j])
            assert res[j]["correspondences"] == w32["correspondences"], (j, res[j], w32)
            assert Td[j].tobytes() == c["T_in"][j].tobytes(), j
            stopped += 1
            continue
        stepped += 1
        if max_it == 1:
            assert res[j]["correspondences"] == w32["correspondences"] and res[j]["iterations"] == 1, (j, res[j], w32)
        s_ang, s_dt = R.pose_error(W32, W64)
        ang, dt = R.pose_error(Td[j], W64)
        b_ang, b_dt = max(0.01, 8.0 * s_ang), max(1e-3 * d, 8.0 * s_dt)
        print("    device vs float64 sums %.3e deg %.3e d_dist; spread of the restatement %.3e deg %.3e d_dist; bound %.3e deg "
              "%.3e d_dist; cond %.3e" % (ang, dt / d, s_ang, s_dt / d, b_ang, b_dt / d, w32["cond"]))
        assert abs(res[j]["iterations"] - w64["iterations"]) <= 1, (j, res[j], w64)
        assert ang <= b_ang and dt <= b_dt, (j, ang, dt / d, b_ang, b_dt / d)
        if j in X.BITS_HELD:
            assert w32["cond"] <= X.COND_BITS
            assert Td[j].tobytes() == W32.tobytes(), (j, Td[j], W32)
            assert (res[j]["iterations"], res[j]["correspondences"], bool(res[j]["converged"])) == \
                (w32["iterations"], w32["correspondences"], bool(w32["converged"])), (j, res[j], w32)
            held += 1
    assert stopped >= 3 and stepped >= 10 and held == len(X.BITS_HELD), (stopped, stepped, held)
