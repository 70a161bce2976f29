"""GPU: every instance of a model in a scene (oslam_align_instances, oslam_db_align_instances).  On seeded scenes with
several copies of a model, the refined instances find every copy and nothing else, where oslam_align finds one; instance
0 is oslam_align's pose on either pose tail; the device selection (k_pose_instances) equals the host rule
(oslam_select_instances) on the candidates the taps report; refinement equals oslam_refine per instance; the database
form equals the single-model form member by member."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DYN_REFINE = ("launches", "ms_total")


def strict(T, truth, ext):
    """the 12 degree / 0.1 extent rule of tools/bench_configs.py:found_at_reference_criterion"""
    from importlib import import_module
    ppf = import_module("objective-slam_amd").ppf
    dt, dr = ppf.ht_dist(np.asarray(T, np.float32), np.asarray(truth, np.float32))
    return dr < np.radians(12) and dt < 0.1 * ext


def same_stats(a, b):
    """counters equal (times aside, and num_emitted: the number of peak records emitted differs from one oslam_align
    to the next of the same pair); -> the differing fields"""
    return {k: (a[k], b[k]) for k in a if not k.startswith("ms_") and k != "num_emitted" and a[k] != b[k]}


def inst_equal(a, b, dyn=DYN_REFINE):
    (Ta, ia), (Tb, ib) = a, b
    ra = {k: v for k, v in ia["refine"].items() if k not in dyn}
    rb = {k: v for k, v in ib["refine"].items() if k not in dyn}
    return (np.array_equal(Ta, Tb) and np.array_equal(ia["T_vote"], ib["T_vote"]) and ia["score"] == ib["score"]
            and ia["candidate"] == ib["candidate"] and ra == rb)


def multi_scene(synth, model_ids, k, seed, S=30000, M=1000, noise=0.05):
    models = {mid: synth.make_model(mid, M) for mid in model_ids}
    d = synth.d_dist_for(models[model_ids[0]][0], 0.05)
    sp, sn, poses = synth.make_scene(model_ids, S, seed, n_instances=k, noise_sigma=noise * d)
    return models, d, sp, sn, poses


# model 1 has a near two-fold symmetry: its copies are found (fitness ~0.9) but often in the pose turned by 180 degrees,
# which the 12 degree rule calls wrong; the two-model scene uses models 0 and 2
SCENES = [([0], 2, 3101), ([0], 3, 3102), ([0, 2], 2, 3103)]


@pytest.mark.parametrize("ids,k,seed", SCENES)
def test_every_copy_is_found_once(ppf, synth, built_lib, ids, k, seed):
    models, d, sp, sn, poses = multi_scene(synth, ids, k, seed)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=2)
    for mid in ids:
        mp, mn = models[mid]
        ext = synth.bbox_extent(mp)
        truths = [T for m, T in poses if m == mid]
        mo = ppf.Model(mp, mn, d_dist=d)
        T = mo.ppf_lookup(sc)
        assert sum(strict(T, G, ext) for G in truths) == 1          # the single pose finds one copy
        found = mo.find_instances(sc)
        assert all(info["refine"]["found"] for _, info in found)
        matched, unmatched = pkg_eval().match_instances(found, truths, ext, dist_thresh_factor=0.1,
                                                        rot_thresh=np.radians(12))
        assert all(m is not None for m in matched), (mid, matched, [i["score"] for _, i in found])
        assert unmatched == [], (mid, unmatched)
        mo.close()
    sc.close()


def pkg_eval():
    from importlib import import_module
    return import_module("objective-slam_amd.evaluate")


FLAGS = [dict(pose_gpu_min=2), dict(pose_gpu_min=1 << 30), dict(pose_gpu_min=2, use_l1_norm=1),
         dict(use_averaged_clusters=1), dict(cpu_clustering=1)]


@pytest.mark.parametrize("flags", FLAGS)
def test_instance_0_is_the_registration_pose(ppf, synth, built_lib, flags):
    models, d, sp, sn, _ = multi_scene(synth, [0], 3, 3102)
    mp, mn = models[0]
    p = ppf.default_params(**flags)
    mo = ppf.Model(mp, mn, d_dist=d, params=p, cpu_clustering=bool(p.cpu_clustering), use_l1_norm=bool(p.use_l1_norm),
                   use_averaged_clusters=bool(p.use_averaged_clusters))
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=2)
    mo.ppf_lookup(sc)                       # the first call grows the scratch pool
    T = mo.ppf_lookup(sc).copy()
    st = dict(mo.stats)
    ip = ppf.default_instance_params(max_instances=16, min_score_ratio=0.2)
    found = mo.find_instances(sc, refine=False, params=ip)
    assert len(found) >= 2, flags
    assert np.array_equal(found[0][1]["T_vote"], T) and np.array_equal(found[0][0], T)
    assert not same_stats(st, mo.stats)
    if not p.cpu_clustering:
        # the host rule on what the taps report: kept cells' poses, clustering-stage translations and scores
        cells, poses = mo.last_cells()
        tr, _, scores, best = mo.last_result(sc)
        cand = R.default_candidates(poses, tr)
        idx = ppf.select_instances(cand, scores, R.centroid(mp), R.extent(mp), params=ip)
        assert [info["candidate"] for _, info in found] == list(idx)
        assert idx[0] == best
        for (_, info), i in zip(found, idx):
            assert np.array_equal(info["T_vote"], cand[i]) and info["score"] == scores[i]
    else:
        assert len({info["candidate"] for _, info in found}) == len(found)
        assert [info["score"] for _, info in found] == sorted([info["score"] for _, info in found], reverse=True)
    mo.close()
    sc.close()


def test_bench_registration_instance_0(ppf, synth, built_lib):
    mp, mn = synth.make_model(0, 5000)
    d = synth.d_dist_for(mp, 0.025)
    sp, sn, _ = synth.make_scene([0], 100000, 2002, instance_points=5000, noise_sigma=0.1 * d)
    mo = ppf.Model(mp, mn, d_dist=d)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=8)
    T = mo.ppf_lookup(sc).copy()
    found = mo.find_instances(sc, refine=False)
    assert np.array_equal(found[0][1]["T_vote"], T)
    mo.close()
    sc.close()


def test_device_selection_equals_host_rule_on_a_large_candidate_set(ppf, synth, built_lib):
    """an absent model with a low vote threshold: 10^5 kept cells and more, through the device tail"""
    mp, mn = synth.make_model(1, 1000)
    d = synth.d_dist_for(mp, 0.05)
    sp, sn, _ = synth.make_scene([0], 40000, 3201, noise_sigma=0.05 * d)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=2)
    n_kept = 0
    for thr in (0.3, 0.15, 0.05):
        mo = ppf.Model(mp, mn, d_dist=d, vote_count_threshold=thr)
        mo.ppf_lookup(sc)
        n_kept = mo.stats["num_top"]
        if n_kept >= 100000:
            break
        mo.close()
    assert n_kept >= 100000, n_kept
    for ip in (ppf.default_instance_params(max_instances=16, min_score_ratio=0.0), ppf.default_instance_params(max_instances=64, min_score_ratio=0.0,
                                                                                          min_separation=0.05, max_angle=0.5)):
        found = mo.find_instances(sc, refine=False, params=ip)
        cells, poses = mo.last_cells()
        tr, _, scores, best = mo.last_result(sc)
        idx = ppf.select_instances(R.default_candidates(poses, tr), scores, R.centroid(mp), R.extent(mp), params=ip)
        assert [info["candidate"] for _, info in found] == list(idx)
        assert len(found) >= 2
    mo.close()
    sc.close()


def test_refinement_equals_oslam_refine_and_dedup(ppf, synth, built_lib):
    """min_separation small enough that several candidates of one copy are accepted: refined, they converge onto it
    and all but the first are dropped"""
    models, d, sp, sn, poses = multi_scene(synth, [0], 2, 3101)
    mp, mn = models[0]
    mo = ppf.Model(mp, mn, d_dist=d, params=ppf.default_params(pose_gpu_min=2))
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=2)
    ip = ppf.default_instance_params(max_instances=24, min_separation=0.02, min_score_ratio=0.3, keep_not_found=1)
    votes = mo.find_instances(sc, refine=False, params=ip)
    refined = mo.find_instances(sc, refine=True, params=ip)
    assert len(votes) >= 4
    # the restatement: oslam_refine per instance, then dedup in acceptance order
    c, ext = R.centroid(mp), R.extent(mp)
    sep2, cos_thr, rot_on = R.thresholds(ip.min_separation, ip.max_angle, ext)
    kept = []
    for T_v, info in votes:
        Tr, res = mo.refine(sc, info["T_vote"])
        p = R.transformed_centroid(Tr, c)
        if any(R.same_instance(p, Tr, R.transformed_centroid(Tk, c), Tk, sep2, cos_thr, rot_on) for Tk, _, _ in kept):
            continue
        kept.append((Tr, res, info))
    assert len(kept) < len(votes)                                     # some converged onto one copy
    assert len(refined) == len(kept)
    for (T, info), (Tr, res, vi) in zip(refined, kept):
        assert np.array_equal(T, Tr) and np.array_equal(info["T_vote"], vi["T_vote"]) and info["candidate"] == vi["candidate"]
        assert {k: v for k, v in info["refine"].items() if k not in DYN_REFINE} == \
            {k: v for k, v in res.items() if k not in DYN_REFINE}
    # the presence filter
    ip.keep_not_found = 0
    only = mo.find_instances(sc, refine=True, params=ip)
    assert [i["candidate"] for _, i in only] == [i["candidate"] for _, i in refined if i["refine"]["found"]]
    mo.close()
    sc.close()


def no_vote_model(ppf, d):
    """points 1000 d_dist apart: no scene pair has such a distance"""
    mp = np.zeros((16, 3), np.float32)
    mp[:, 0] = np.arange(16) * 1000.0 * d
    mn = np.tile(np.float32([0, 0, 1]), (16, 1))
    return ppf.Model(mp, mn, d_dist=d)


def check_db(ppf, models, sc, ip, refine):
    db = ppf.Database(models)
    got = db.find_instances(sc, refine=refine, params=ip)
    again = db.find_instances(sc, refine=refine, params=ip)
    db.close()
    for j, mo in enumerate(models):
        one = mo.find_instances(sc, refine=refine, params=ip)
        assert len(one) == len(got[j]) == len(again[j]), j
        for a, b, c in zip(one, got[j], again[j]):
            assert inst_equal(a, b) and inst_equal(b, c), j
    return got


def test_database_equals_single_models_on_a_point_cloud(ppf, synth, built_lib):
    models, d, sp, sn, _ = multi_scene(synth, [0, 1], 2, 3103)
    sc = ppf.Scene(sp, sn, d_dist=0.0, ref_point_downsample_factor=2)      # a database scene: models of two d_dists
    ms = [ppf.Model(models[0][0], models[0][1], d_dist=d, params=ppf.default_params(pose_gpu_min=2)),
          ppf.Model(models[1][0], models[1][1], d_dist=d),
          ppf.Model(models[1][0], models[1][1], d_dist=1.25 * d, params=ppf.default_params(pose_gpu_min=2)),
          no_vote_model(ppf, d),
          ppf.Model(models[0][0], models[0][1], d_dist=d, cpu_clustering=True)]
    assert np.all(ms[3].ppf_lookup(sc, allow_no_votes=True) == 0)
    ip = ppf.default_instance_params(max_instances=6, min_score_ratio=0.3)
    for refine in (False, True):
        got = check_db(ppf, ms, sc, ip, refine)
        assert len(got[3]) == 0 and len(got[0]) >= 2
    for m in ms:
        m.close()
    sc.close()


def test_database_equals_single_models_on_a_depth_frame(ppf, synth, built_lib):
    raw = [synth.make_model(k, 1500) for k in range(4)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth.random_rotation(synth.SplitMix64(93))
    T[:3, 3] = [0.5, 0.0, 5.5]
    img = synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1)
    sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                              z_min=0.5, z_max=12.0, max_jump=0.08)
    ms = [ppf.Model(g[0], g[1], d_dist=d, params=ppf.default_params(pose_gpu_min=2)) for g in grids]
    ms.append(ppf.Model(grids[1][0], grids[1][1], d_dist=1.5 * d))
    ms.append(no_vote_model(ppf, d))
    ip = ppf.default_instance_params(max_instances=4)
    for refine in (False, True):
        got = check_db(ppf, ms, sc, ip, refine)
        assert len(got[-1]) == 0
    assert any(strict(Ti, T, synth.bbox_extent(grids[0][0])) for Ti, _ in got[0])
    for m in ms:
        m.close()
    sc.close()


def test_repeatable_and_no_side_effects_on_align(ppf, synth, built_lib):
    models, d, sp, sn, _ = multi_scene(synth, [0], 3, 3102)
    for flags in (dict(pose_gpu_min=2), dict(pose_gpu_min=1 << 30)):
        mo = ppf.Model(models[0][0], models[0][1], d_dist=d, params=ppf.default_params(**flags))
        sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=2)
        mo.ppf_lookup(sc)                   # the first call grows the scratch pool
        T1 = mo.ppf_lookup(sc).copy()
        s1 = dict(mo.stats)
        c1, p1 = mo.last_cells()
        a = mo.find_instances(sc)
        b = mo.find_instances(sc)
        assert len(a) == len(b) and all(inst_equal(x, y) for x, y in zip(a, b))
        c_i, p_i = mo.last_cells()
        assert np.array_equal(c1, c_i) and np.array_equal(p1, p_i)
        T2 = mo.ppf_lookup(sc).copy()
        c2, p2 = mo.last_cells()
        assert np.array_equal(T1, T2) and not same_stats(s1, mo.stats)
        assert np.array_equal(c1, c2) and np.array_equal(p1, p2)
        mo.close()
        sc.close()
