"""CPU: the refinement stage's yardstick and its arguments (include/oslam.h at oslam_refine).

The numpy restatement (tests/refine_ref.py), started from the oracle's voting pose, is checked against the ground
truth on seeded scenes (model 0, tau_d 0.05).  Measured on the CPU when these bounds were set (rotation error in
degrees, translation error in units of d_dist, fitness at the refined pose; model 3, absent, refined from its own
voting pose):

    M/S/seed/noise/occlusion   vote -> refined           fitness present / absent
    600/3000/11/0.00/0.0       10.47, 0.46 -> 0.23, 0.02   0.59 / 0.06
    600/3000/12/0.10/0.0        1.15, 0.14 -> 0.30, 0.04   0.60 / 0.11
    1000/5000/13/0.10/0.5       3.57, 0.26 -> 0.20, 0.11   0.39 / 0.13
    600/3000/14/0.05/0.3        3.67, 0.59 -> 0.92, 0.13   0.43 / 0.07
    600/3000/15/0.10/0.3        3.10, 0.33 -> 0.53, 0.12   0.37 / 0.06
    800/4000/16/0.05/0.5        7.21, 0.64 -> 1.21, 0.06   0.33 / 0.25
    600/3000/17/0.00/0.2        2.59, 0.38 -> 0.40, 0.04   0.48 / 0.05
    600/3000/18/0.10/0.1        3.70, 0.50 -> 0.91, 0.05   0.51 / 0.08

Every trial is under 1.3 degrees and 0.14 d_dist (median 0.46 degrees), and none got worse than its vote: the GPU
ground-truth test uses 2 degrees / 0.25 d_dist / median 1 degree.  The smallest present fitness (0.33) and the
largest absent one (0.25) put the default min_fitness at 0.3.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as R  # noqa: E402

CASES = [(600, 3000, 11, 0.0, 0.0), (600, 3000, 12, 0.1, 0.0), (1000, 5000, 13, 0.1, 0.5), (600, 3000, 14, 0.05, 0.3),
         (600, 3000, 15, 0.1, 0.3), (800, 4000, 16, 0.05, 0.5), (600, 3000, 17, 0.0, 0.2), (600, 3000, 18, 0.1, 0.1)]


def make_trial(synth, M, S, seed, noise, occ, model_id=0):
    mp, mn = synth.make_model(model_id, M)
    d = synth.d_dist_for(mp, 0.05)
    sp, sn, poses = synth.make_scene([model_id], S, seed, instance_points=M, noise_sigma=noise * d, occlusion=occ)
    return mp, mn, d, sp, sn, poses[0][1]


def test_restatement_reaches_ground_truth_and_separates_absent_models(oracle, synth):
    rot, trans, present, absent = [], [], [], []
    for M, S, seed, noise, occ in CASES:
        mp, mn, d, sp, sn, truth = make_trial(synth, M, S, seed, noise, occ)
        cells, _ = oracle.votes_fused(mp, mn, sp, sn, 1, d, 0.4)
        _, T0 = oracle.pose_from_cells(cells, mp, mn, sp, sn, d)
        T1, info = R.refine(mp, mn, sp, sn, T0, d)
        a0, _ = R.pose_error(T0, truth)
        a1, e1 = R.pose_error(T1, truth)
        assert a1 <= a0, (seed, a0, a1)
        rot.append(a1)
        trans.append(e1 / d)
        present.append(info["fitness"])
        assert info["fitness"] >= info["fitness_in"] or a0 < 1.5, (seed, info)
        ap, an = synth.make_model(3, M)
        da = synth.d_dist_for(ap, 0.05)
        c3, _ = oracle.votes_fused(ap, an, sp, sn, 1, da, 0.4)
        _, T3 = oracle.pose_from_cells(c3, ap, an, sp, sn, da)
        absent.append(R.refine(ap, an, sp, sn, T3, da)[1]["fitness"])
    assert max(rot) < 2.0 and max(trans) < 0.25 and np.median(rot) < 1.0, (rot, trans)
    min_fit = R.default_params()["min_fitness"]
    assert min(present) >= min_fit > max(absent), (present, absent)


def test_correspondence_rule_by_hand():
    """The restatement's rule on a hand-made case: nearest qualifying point, normal gate, tie to the lowest index."""
    sp = np.float32([[0.1, 0, 0], [0.05, 0, 0], [-0.05, 0, 0], [0, 0.02, 0], [3, 3, 3]])
    sn = np.float32([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 1]])
    q = np.float32([[0, 0, 0], [3, 3, 3], [9, 9, 9]])
    m = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1]])
    idx, d2 = R.correspondences(q, m, sp, sn, 0.2, 0.8)
    # point 1 is nearer but faces away; points 2 and 3 are not tied (0.05^2 vs 0.02^2): 3 wins; 4 is exact; none at 9
    assert list(idx) == [3, 4, -1]
    sp2 = np.float32([[0.03, 0, 0], [-0.03, 0, 0]])
    sn2 = np.float32([[0, 0, 1], [0, 0, 1]])
    idx, _ = R.correspondences(q[:1], m[:1], sp2[::-1].copy(), sn2, 0.2, 0.8)
    assert list(idx) == [0]                            # equal d2: the lower scene index


def test_refine_params_default(built_lib, ppf):
    p = ppf.default_refine_params()
    assert p.max_iterations == 30
    assert (p.max_corr_dist, p.min_normal_dot, p.inlier_dist) == (np.float32(2.0), np.float32(0.8), np.float32(0.5))
    assert p.min_fitness == np.float32(R.default_params()["min_fitness"])
    assert (p.stop_rot, p.stop_trans) == (np.float32(1e-5), np.float32(1e-4))
    assert list(p.reserved) == [0, 0, 0, 0]
    assert ppf.default_refine_params(max_iterations=5).max_iterations == 5
    with pytest.raises(TypeError):
        ppf.default_refine_params(no_such_field=1)


def test_refine_rejects_bad_arguments_before_touching_handles(built_lib, ppf):
    """Argument checks run before any handle is read or any device call is made: stand-in handles (zeroed host
    memory) are never looked at, on a machine with or without a GPU."""
    L = ppf.lib()
    fake_m = C.create_string_buffer(4096)
    fake_s = C.create_string_buffer(4096)
    m, s = C.cast(fake_m, C.c_void_p), C.cast(fake_s, C.c_void_p)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    res = ppf.RefineResult()
    p = ppf.default_refine_params()

    def call(T, params=p, mm=m, ss=s, To=out):
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        return L.oslam_refine(mm, ss, ppf._p(T), C.byref(params) if params is not None else None,
                              ppf._p(To) if To is not None else None, C.byref(res))

    assert call(eye, mm=None) == ppf.OSLAM_E_INVALID
    assert call(eye, ss=None) == ppf.OSLAM_E_INVALID
    assert call(eye, To=None) == ppf.OSLAM_E_INVALID
    assert L.oslam_refine(m, s, None, C.byref(p), ppf._p(out), C.byref(res)) == ppf.OSLAM_E_INVALID
    bad = []
    T = eye.copy(); T[3] = np.nan; bad.append(T)                                    # not finite
    T = eye.copy(); T[5] = np.inf; bad.append(T)
    T = (2 * np.eye(4, dtype=np.float32)).reshape(16); T[15] = 1; bad.append(T)    # scaled
    T = eye.copy(); T[1] = 0.01; bad.append(T)                                      # sheared beyond 1e-3
    T = eye.copy(); T[0] = -1; bad.append(T)                                        # reflection
    T = eye.copy(); T[12] = 0.5; bad.append(T)                                      # last row
    bad.append(np.zeros(16, np.float32))                                            # a single call has no "skipped"
    for T in bad:
        assert call(T) == ppf.OSLAM_E_INVALID, T
    for kw in (dict(max_corr_dist=0.0), dict(max_corr_dist=-1.0), dict(inlier_dist=0.0), dict(inlier_dist=3.0),
               dict(max_corr_dist=float("nan")), dict(min_normal_dot=float("inf")), dict(max_iterations=5000),
               dict(stop_rot=-1.0)):
        assert call(eye, params=ppf.default_refine_params(**kw)) == ppf.OSLAM_E_INVALID, kw
    # the tap: radius <= 0, bad pose, NULL output
    idx = np.zeros(8, np.int32)
    for radius, T in ((0.0, eye), (-1.0, eye), (float("nan"), eye), (0.1, bad[2])):
        assert L.oslam_refine_correspondences(m, s, ppf._p(np.ascontiguousarray(T)), radius, 0.8, ppf._p(idx)) == ppf.OSLAM_E_INVALID
    assert L.oslam_refine_correspondences(m, s, ppf._p(eye), 0.1, 0.8, None) == ppf.OSLAM_E_INVALID
    # the database form: NULL handles and outputs, bad parameters
    Tn = np.zeros((2, 16), np.float32)
    assert L.oslam_db_refine(None, s, ppf._p(Tn), None, ppf._p(Tn), None) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_refine(m, None, ppf._p(Tn), None, ppf._p(Tn), None) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_refine(m, s, None, None, ppf._p(Tn), None) == ppf.OSLAM_E_INVALID
    assert L.oslam_db_refine(m, s, ppf._p(Tn), C.byref(ppf.default_refine_params(inlier_dist=9.0)), ppf._p(Tn),
                             None) == ppf.OSLAM_E_INVALID
    with pytest.raises(ppf.OslamError) as e:
        L2 = ppf.default_refine_params(max_corr_dist=-1.0)
        ppf._check(L.oslam_refine(m, s, ppf._p(eye), C.byref(L2), ppf._p(out), C.byref(res)))
    assert e.value.code == ppf.OSLAM_E_INVALID and "max_corr_dist" in str(e.value)
