"""Secondary measurements on one MI355X: BASELINE.json configs[1..4] (bench.py measures the headline
configuration; these are not bench lines).  Needs a HIP device.

  python tools/bench_configs.py cfg2     single 5k model vs 50k voxel-gridded scene
  python tools/bench_configs.py cfg3     10-model database vs 100k scene, all tables resident
  python tools/bench_configs.py cfg4     a 1-GPU slice of the 100-model / 500k-scene job: this rank's
                                         share (1/8 of the reference points) of N models, ref_point_df 20
  python tools/bench_configs.py cfg5     streaming: 640x480 depth frames -> points+normals -> voxel grid
                                         -> registration against a resident model database; frames/s
  python tools/bench_configs.py refine   the refinement stage: oslam_refine on the bench registration (5k model, 100k
                                         scene) from its voting pose, and the db50 stream with db.align + db.refine
  python tools/bench_configs.py arbitrate   the db50 stream with db.align + db.refine + db.verify + db.arbitrate per frame and
                                         with db.detect: frames/s, arbitrate ms per frame, the found sets before and after
  python tools/bench_configs.py verify   the db50 stream with db.align + db.refine + db.verify per frame: frames/s, verify
                                         ms per frame, and the found sets of refine and of verify on every frame
  python tools/bench_configs.py instances  oslam_align_instances next to oslam_align (bench registration, a scene
                                         with 3 copies: recall and false detections) and db.find_instances on db50
  python tools/bench_configs.py track    the db50 stream with smooth motion over 30 frames: db.detect on every frame next
                                         to Tracker.step (detect_every 10, the scene built on search frames only), and
                                         db.track per call for 1 and 50 hypotheses next to db.refine + db.verify
  python tools/bench_configs.py camera   a static world seen from a moving camera (3 degrees and 3 cm per frame, 30 frames
                                         at 640x480): oslam_view_egomotion per call, and Tracker.step on one object
                                         with and without the camera's motion
  python tools/bench_configs.py fusion   a 256^3 TSDF volume over the room of the camera configuration and its 640x480
                                         stream: integrate, raycast, track per call, Volume.step in frames/s, and the
                                         bytes per second the integration rule loads and stores
  python tools/bench_configs.py surface  the fusion configuration's 256^3 volume after its stream: Volume.surface and
                                         Scene.from_volume per call next to one integrate (all three stream the volume)
  python tools/bench_configs.py mesh     the same volume: Volume.mesh with and without normals and, in the same run,
                                         Volume.surface and one integrate; median of 20 calls each
  python tools/bench_configs.py pyramid  the camera configuration's 640x480 stream: Pyramid(view), egomotion_pyramid and,
                                         in the same run, egomotion on the same pair; median of 20 calls each
  python tools/bench_configs.py shift    the same volume: Volume.shift by (8, 0, 0) and (-8, 0, 0) alternately,
                                         Volume.leaving((8, 0, 0)) and, in the same run, one integrate and Volume.surface;
                                         median of 20 calls each, and the bytes per second the shift loads and stores
  python tools/bench_configs.py explain  the db50 stream with the twin: db.align + db.refine + db.verify per frame, then
                                         db.arbitrate and db.explain over what verification found: who is verified, who
                                         each stage keeps and both stages' ms per frame; and ms_total of explain,
                                         arbitrate and render for 1 and 50 hypotheses, median of 20 calls each
  python tools/bench_configs.py bilateral  the camera configuration's 640x480 stream: bilateral_view, Pyramid(view) as the
                                         yardstick, and egomotion on the raw and on the filtered first pair, in the same
                                         run; median of 20 calls each
  python tools/bench_configs.py normals  oslam_cloud_normals on the 100k-point bench scene and on the 500k-point slice's
                                         scene (points only), at radii of 2 and 4 times the median spacing: whole call,
                                         grid build and kernel, median of 20 calls after 5, and the neighbours visited and
                                         accepted per second of kernel time
  python tools/bench_configs.py colour   the fusion configuration's 256^3 volume and 640x480 stream with a colour image per
                                         frame: integrate without and with colour, paint on a ray-cast view, colours on
                                         the surface's points, median of 20 calls each, Volume.step in frames/s without
                                         and with colour, and the coloured mesh of the calibration room written as PLY
                                         with its colour error
  python tools/bench_configs.py findplanes  frame 0 of the camera configuration's room at 640x480: find_planes and
                                         remove_planes, median of 20 calls each, the scene points before and after, and
                                         the recognition chain on the full scene next to plane finding + removal + the
                                         chain on the reduced scene, alternating (`planes` is the plane-dominated clouds)
  python tools/bench_configs.py segments  the same frame: find_planes + find_segments(view, planes) + select_segments,
                                         median of 20 calls each, the chain of the three models on the reduced scene next
                                         to the chain of each model on each of the three largest segments' scenes,
                                         alternating (`segments only`: the find_segments calls alone)
One JSON line each."""
import importlib, json, os, sys, time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("objective-slam_amd")
ppf, synth = pkg.ppf, pkg.synth
evaluate = importlib.import_module("objective-slam_amd.evaluate")


def found_at_reference_criterion(T, truth, pts):
    dt, dr = ppf.ht_dist(T, truth)
    return bool(dr < np.radians(12) and dt < 0.1 * synth.bbox_extent(pts))


def align_all(models, dd, sp, sn, df, params=None):
    out = []
    for mo, d in zip(models, dd):
        sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=df, params=params)
        out.append((mo.ppf_lookup(sc, allow_no_votes=True).copy(), dict(mo.stats)))
        sc.close()
    return out


def cfg2():
    mp, mn = synth.make_model(0, 5000)
    d = synth.d_dist_for(mp, 0.025)
    raw_p, raw_n, poses = synth.make_scene([0], 200000, 2002, instance_points=20000, noise_sigma=0.1 * d)
    t = time.perf_counter(); sp, sn = ppf.voxel_grid(raw_p, raw_n, leaf=0.6 * d); t_vox = time.perf_counter() - t
    mo = ppf.Model(mp, mn, d_dist=d)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=5)
    mo.ppf_lookup(sc)
    t = time.perf_counter(); T = mo.ppf_lookup(sc); el = time.perf_counter() - t
    st = mo.stats
    return {"config": "cfg2: 5k model vs voxel-gridded scene", "scene_points_after_voxel_grid": len(sp), "voxel_grid_s": t_vox,
            "ref_point_df": 5, "align_s": el, "scene_ppfs_per_s": st["num_scene_ppfs"] / el, "votes_per_s": st["num_votes"] / el,
            "wide_workgroups": st["wide_workgroups"], "found": found_at_reference_criterion(T, poses[0][1], mp)}


def cfg3():
    ids = list(range(10))
    clouds = [synth.make_model(k, 5000) for k in ids]
    dd = [synth.d_dist_for(c[0], 0.025) for c in clouds]
    sp, sn, poses = synth.make_scene([0, 4, 8], 100000, 2003, instance_points=5000, noise_sigma=0.1 * dd[0])
    t = time.perf_counter(); models = [ppf.Model(c[0], c[1], d_dist=d) for c, d in zip(clouds, dd)]; t_build = time.perf_counter() - t
    align_all(models[:1], dd[:1], sp, sn, 10)
    t = time.perf_counter(); res = align_all(models, dd, sp, sn, 10); el = time.perf_counter() - t
    return {"config": "cfg3: 10-model database vs 100k scene", "db_models": 10, "ref_point_df": 10,
            "db_bytes_in_hbm": sum(m.table_bytes() for m in models), "build_all_s": t_build, "frame_s": el,
            "scene_ppfs_per_s": sum(s["num_scene_ppfs"] for _, s in res) / el, "votes_per_s": sum(s["num_votes"] for _, s in res) / el,
            "instances_found": {mid: found_at_reference_criterion(res[mid][0], T, clouds[mid][0]) for mid, T in poses}}


def cfg3db():
    """cfg3 through the database object, once with every model's own d_dist (ten groups of one) and once with ONE
    d_dist for the whole database (one group: one scene pass per frame for all ten models)."""
    ids = list(range(10))
    clouds = [synth.make_model(k, 5000) for k in ids]
    dd = [synth.d_dist_for(c[0], 0.025) for c in clouds]
    sp, sn, poses = synth.make_scene([0, 4, 8], 100000, 2003, instance_points=5000, noise_sigma=0.1 * dd[0])
    sc = ppf.Scene(sp, sn, d_dist=0.0, ref_point_downsample_factor=10)
    out = {"config": "cfg3 through oslam_db: 10-model database vs 100k scene", "ref_point_df": 10}
    for name, dds in (("own_d_dist", dd), ("common_d_dist", [dd[0]] * 10)):
        models = [ppf.Model(c[0], c[1], d_dist=d) for c, d in zip(clouds, dds)]
        db = ppf.Database(models)
        db.align(sc)
        t = time.perf_counter(); T, stats = db.align(sc); el = time.perf_counter() - t
        out[name] = {"groups": db.n_groups, "frame_s": el, "votes_per_s": sum(s["num_votes"] for s in stats) / el,
                     "key_kernels_ms": sum(s["ms_key_kernel"] for s in stats), "vote_kernels_ms": sum(s["ms_vote_kernel"] for s in stats),
                     "instances_found": {mid: found_at_reference_criterion(T[mid], Tt, clouds[mid][0]) for mid, Tt in poses}}
        db.close()
        for m in models:
            m.close()
    return out


def cfg4(n_models=4):
    ids = list(range(n_models))
    clouds = [synth.make_model(k, 5000) for k in ids]
    dd = [synth.d_dist_for(c[0], 0.025) for c in clouds]
    sp, sn, poses = synth.make_scene(ids[:2], 500000, 2004, instance_points=5000, noise_sigma=0.1 * dd[0])
    par = ppf.default_params(shard_rank=0, shard_world=8)          # this GPU's eighth of the reference points
    models = [ppf.Model(c[0], c[1], d_dist=d, params=par) for c, d in zip(clouds, dd)]
    align_all(models[:1], dd[:1], sp, sn, 20, params=par)         # scratch pool sized before the clock starts
    t = time.perf_counter(); res = align_all(models, dd, sp, sn, 20, params=par); el = time.perf_counter() - t
    ppfs = sum(s["num_scene_ppfs"] for _, s in res)
    return {"config": "cfg4 slice: %d of 100 models vs 500k scene, rank 0 of 8 (1/8 of the reference points), local votes + "
                      "host stage on the local peaks only" % n_models, "ref_point_df": 20,
            "ref_points_this_rank": int(res[0][1]["num_scene_ppfs"] // (len(sp) - 1)), "seconds_per_model": el / n_models,
            "projected_seconds_for_100_models_per_gpu": 100 * el / n_models, "scene_ppfs_per_s": ppfs / el,
            "votes_per_s": sum(s["num_votes"] for _, s in res) / el,
            "vote_launches_per_model": res[0][1]["vote_launches"],
            "ms_key_kernels_per_model": sum(s["ms_key_kernel"] for _, s in res) / n_models,
            "ms_vote_kernels_per_model": sum(s["ms_vote_kernel"] for _, s in res) / n_models}


def cfg5(n_models=4, frames=8):
    ids = list(range(0, 2 * n_models, 2))
    clouds = [synth.make_model(k, 1500) for k in ids]
    dd = [synth.d_dist_for(c[0], 0.05) for c in clouds]
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c, d in zip(clouds, dd)]
    models = [ppf.Model(g[0], g[1], d_dist=d) for g, d in zip(grids, dd)]
    dense = [synth.make_model(k, 300000)[0] for k in ids[:2]]
    rng = synth.SplitMix64(55)
    imgs, truths = [], []
    for f in range(frames):                                    # two objects drifting in front of a wall
        pts, tr = [], []
        for j, dn in enumerate(dense):
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = synth.random_rotation(rng)
            T[:3, 3] = [-2.0 + 4.0 * j + 0.05 * f, 0.3 * j - 0.1, 7.0 + 0.5 * j]
            pts.append(dn @ T[:3, :3].T + T[:3, 3])
            tr.append(T)
        imgs.append(synth.render_depth(np.concatenate(pts), background_z=10.0, splat=1))
        truths.append(tr)
    leaf = min(dd)                                                 # one scene_leaf_size for all models (alignment.cpp:265-271)
    wide = 0
    def one(img):
        t0 = time.perf_counter()
        # depth -> points + normals -> voxel grid -> scene in one call (d_dist 0: a scene for every model)
        sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=leaf, d_dist=0.0, ref_point_downsample_factor=2,
                                  z_min=0.5, z_max=12.0, max_jump=0.08)
        t1 = time.perf_counter()
        nonlocal wide
        out, votes = [], 0
        for mo in models:
            out.append(mo.ppf_lookup(sc, allow_no_votes=True).copy())
            votes += mo.stats["num_votes"]
            wide += mo.stats["wide_workgroups"]
        n_scene = sc.numPoints()
        sc.close()
        t2 = time.perf_counter()
        return out, t1 - t0, 0.0, t2 - t0, 0, n_scene, t2 - t1, votes
    one(imgs[0])
    t = time.perf_counter(); res = [one(im) for im in imgs]; el = time.perf_counter() - t
    ok = sum(found_at_reference_criterion(r[0][j], truths[f][j], clouds[j][0]) for f, r in enumerate(res) for j in range(2))
    return {"config": "cfg5: 640x480 depth frames vs a %d-model database (oslam_scene_from_depth, then one align per model)" % n_models,
            "frames": frames, "frames_per_s": frames / el, "ms_per_frame": 1e3 * el / frames,
            "ms_depth_to_scene": 1e3 * np.mean([r[1] for r in res]),
            "ms_registration_all_models": 1e3 * np.mean([r[6] for r in res]), "votes_per_frame": int(np.mean([r[7] for r in res])),
            "scene_points_after_voxel_grid": int(np.mean([r[5] for r in res])), "wide_workgroups_per_frame": wide / float(frames + 1),
            "objects_found": "%d of %d" % (ok, 2 * frames)}


def _planes_and_object(n, rng, extent, obj_id=0, obj_frac=0.25):
    """A floor (z = 0), a wall (x = 0) and a table top (z = 0.8) of `extent`, with an object standing on the table: the
    kind of cloud a depth camera sees indoors.  Large planes in BOTH clouds put more than 65 535 votes into single
    accumulator cells (every in-plane pair has the same feature), which is what the 32-bit re-vote passes exist for."""
    n_obj = int(n * obj_frac)
    n_pl = (n - n_obj) // 3
    u = rng.uniform(0, extent, (3, n_pl, 2))
    floor = np.concatenate([u[0], np.zeros((n_pl, 1))], 1)
    wall = np.concatenate([np.zeros((n_pl, 1)), u[1]], 1)
    table = np.concatenate([0.3 * extent + 0.4 * u[2], np.full((n_pl, 1), 0.8)], 1)
    op, on = synth.make_model(obj_id, n - 3 * n_pl)
    op = op * (0.25 * extent / synth.bbox_extent(op)) + np.array([0.5 * extent, 0.5 * extent, 0.8 + 0.2 * extent])
    pts = np.concatenate([floor, wall, table, op]).astype(np.float32)
    nrm = np.concatenate([np.tile([0, 0, 1.0], (n_pl, 1)), np.tile([1.0, 0, 0], (n_pl, 1)), np.tile([0, 0, 1.0], (n_pl, 1)), on]).astype(np.float32)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(nrm[order])


def planes(M=5000, S=100000, df=8):
    """The re-vote path where it matters: a plane-dominated model (object on a table in a room corner) against a
    plane-dominated scene of the same room.  Reports wide_workgroups and the time per registration."""
    rng = np.random.default_rng(7)
    mp, mn = _planes_and_object(M, rng, 3.5)
    sp0, sn0 = _planes_and_object(S, rng, 3.5)
    R = synth.random_rotation(synth.SplitMix64(5))
    sp = (sp0 @ R.T + np.float32([0.4, -0.2, 0.1])).astype(np.float32)
    sn = (sn0 @ R.T).astype(np.float32)
    sp += (0.002 * rng.normal(size=sp.shape)).astype(np.float32)
    d = synth.d_dist_for(mp, 0.025)
    mo = ppf.Model(mp, mn, d_dist=d)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=df)
    mo.ppf_lookup(sc, allow_no_votes=True)
    t = time.perf_counter(); T = mo.ppf_lookup(sc, allow_no_votes=True); el = time.perf_counter() - t
    st = mo.stats
    Tt = np.eye(4); Tt[:3, :3] = R; Tt[:3, 3] = [0.4, -0.2, 0.1]
    dt, dr = ppf.ht_dist(T, Tt)
    return {"config": "plane-dominated model (%d points) vs plane-dominated scene (%d points): floor + wall + table + object in both" % (M, S),
            "ref_point_df": df, "align_s": el, "ms_vote_kernels": st["ms_vote_kernel"], "ms_key_kernels": st["ms_key_kernel"],
            "votes": st["num_votes"], "max_cell": st["max_count"], "wide_workgroups": st["wide_workgroups"],
            "vote_workgroups": int(st["num_scene_ppfs"] // (S - 1)) * ((M + 2045) // 2046), "votes_per_s": st["num_votes"] / el,
            "rot_err_deg": float(np.degrees(dr)), "trans_err": float(dt)}


def db50(frames=10):
    """configs[4] at database size (tests/test_gpu_database.py measures the same): 640x480 depth frames against 50
    models with one d_dist -- all 50 on one GPU, and the 7 models one of 8 GPUs holds when the database is split by model."""
    n_models, world = 50, 8
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    imgs = []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        imgs.append(synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1))
    out = {"config": "cfg5 at database size: 640x480 depth frames vs a 50-model database, one d_dist", "frames": frames}
    for name, ids in (("all_50_on_one_gpu", list(range(n_models))), ("shard_of_7_models", list(range(0, n_models, world)))):
        models = [ppf.Model(grids[j][0], grids[j][1], d_dist=d) for j in ids]
        db = ppf.Database(models)
        def frame(img):
            sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                      z_min=0.5, z_max=12.0, max_jump=0.08)
            T, stats = db.align(sc)
            n = sc.numPoints()
            sc.close()
            return stats, n
        frame(imgs[0])
        t = time.perf_counter(); res = [frame(im) for im in imgs]; el = time.perf_counter() - t
        out[name] = {"frames_per_s": frames / el, "ms_per_frame": 1e3 * el / frames, "scene_points": res[0][1],
                     "ms_key_kernels": float(np.mean([sum(s["ms_key_kernel"] for s in r[0]) for r in res])),
                     "ms_vote_kernels": float(np.mean([sum(s["ms_vote_kernel"] for s in r[0]) for r in res])),
                     "wide_workgroups_per_frame": float(np.mean([sum(s["wide_workgroups"] for s in r[0]) for r in res])),
                     "model_points": int(np.mean([len(grids[j][0]) for j in ids]))}
        db.close()
        for m in models:
            m.close()
    return out


def refine(calls=20, frames=10):
    """The refinement stage (oslam_refine): one model on the bench registration, refined from its voting pose (median
    over `calls` calls, the scene grid already cached), and the db50 stream with db.align + db.refine per frame."""
    def err(T, truth, d):
        dt, dr = ppf.ht_dist(T, truth)
        return float(np.degrees(dr)), float(dt / d)
    mp, mn = synth.make_model(0, 5000)
    d = synth.d_dist_for(mp, 0.025)
    sp, sn, poses = synth.make_scene([0], 100000, 2002, instance_points=5000, noise_sigma=0.1 * d)
    mo = ppf.Model(mp, mn, d_dist=d)
    sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=8)
    T0 = mo.ppf_lookup(sc).copy()
    t = time.perf_counter(); _, first = mo.refine(sc, T0); ms_first = 1e3 * (time.perf_counter() - t)
    ts, lib_ms = [], []
    for _ in range(calls):
        t = time.perf_counter(); T1, info = mo.refine(sc, T0); ts.append(1e3 * (time.perf_counter() - t))
        lib_ms.append(info["ms_total"])
    r0, t0 = err(T0, poses[0][1], d)
    r1, t1 = err(T1, poses[0][1], d)
    out = {"config": "refinement stage (oslam_refine / oslam_db_refine)",
           "bench_registration": {"model_points": 5000, "scene_points": 100000, "calls": calls,
                                  "median_ms": float(np.median(ts)), "median_ms_total_in_library": float(np.median(lib_ms)),
                                  "first_call_ms_with_grid_build": ms_first, "launches": info["launches"],
                                  "launches_first_call": first["launches"], "iterations": info["iterations"],
                                  "converged": bool(info["converged"]), "fitness_in": info["fitness_in"],
                                  "fitness": info["fitness"], "rmse_over_d_dist": info["rmse"] / d,
                                  "rot_err_deg_vote": r0, "trans_err_d_vote": t0, "rot_err_deg_refined": r1,
                                  "trans_err_d_refined": t1}}
    mo.close()
    sc.close()
    n_models = 50
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    imgs, truths = [], []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        imgs.append(synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1))
        truths.append(T)
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)

    def frame(img):
        sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                  z_min=0.5, z_max=12.0, max_jump=0.08)
        Ta, _ = db.align(sc)
        t = time.perf_counter(); Tr, res, found = db.refine(sc, Ta); ms = 1e3 * (time.perf_counter() - t)
        sc.close()
        return Tr, res, found, ms
    frame(imgs[0])
    t = time.perf_counter(); rs = [frame(im) for im in imgs]; el = time.perf_counter() - t
    out["db50_stream"] = {"frames": frames, "models": n_models, "frames_per_s": frames / el,
                          "ms_refine_per_frame": float(np.mean([r[3] for r in rs])),
                          "ms_refine_per_frame_median": float(np.median([r[3] for r in rs])),
                          "launches_per_call": [r[1][0]["launches"] for r in rs],
                          "iterations_model0": [r[1][0]["iterations"] for r in rs],
                          "found_members_per_frame": [[int(j) for j in np.flatnonzero(r[2])] for r in rs],
                          "fitness_model0": [round(r[1][0]["fitness"], 3) for r in rs],
                          "max_fitness_absent": [round(max(x["fitness"] for x in r[1][1:]), 3) for r in rs],
                          "rot_err_deg_model0_refined": [round(err(r[0][0], truths[f], d)[0], 3) for f, r in enumerate(rs)]}
    db.close()
    for m in models:
        m.close()
    return out


def verify(frames=10):
    """Verification against the depth image (oslam_db_verify) on the db50 stream: db.align + db.refine + db.verify per
    frame (the view is built from the frame's image inside the timed loop), the found sets of refine and of verify
    against the truth (model 0 is the only object in every frame)."""
    n_models = 50
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    imgs = []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        imgs.append(synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1))
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)

    def frame(img):
        sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                  z_min=0.5, z_max=12.0, max_jump=0.08)
        Ta, _ = db.align(sc)
        Tr, _, found_r = db.refine(sc, Ta)
        t = time.perf_counter()
        view = ppf.View(img, 525.0, 525.0, 319.5, 239.5, z_min=0.5, z_max=12.0)
        t_view = time.perf_counter()
        res, found_v = db.verify(view, Tr)
        t_end = time.perf_counter()
        _, found_tight = db.verify(view, Tr, ppf.default_verify_params(depth_tol=0.5))
        view.close()
        sc.close()
        return found_r, found_v, res, 1e3 * (t_end - t), 1e3 * (t_end - t_view), found_tight
    frame(imgs[0])
    t = time.perf_counter(); rs = [frame(im) for im in imgs]; el = time.perf_counter() - t
    out = {"config": "verification (oslam_db_verify) on the db50 stream", "frames": frames, "models": n_models,
           "frames_per_s_align_refine_verify": frames / el,
           "ms_verify_per_frame_with_view": float(np.mean([r[3] for r in rs])),
           "ms_verify_per_frame_call_only": float(np.mean([r[4] for r in rs])),
           "ms_verify_in_library": float(np.mean([r[2][0]["ms_total"] for r in rs])),
           "launches_per_call": [r[2][0]["launches"] for r in rs],
           "found_refine": [[int(j) for j in np.flatnonzero(r[0])] for r in rs],
           "found_verify": [[int(j) for j in np.flatnonzero(r[1])] for r in rs],
           "found_verify_depth_tol_0.5": [[int(j) for j in np.flatnonzero(r[5])] for r in rs],
           "view_fitness_model0": [round(r[2][0]["view_fitness"], 3) for r in rs],
           "coverage_model0": [round(r[2][0]["coverage"], 3) for r in rs],
           "max_view_fitness_absent": [round(max(x["view_fitness"] for x in r[2][1:]), 3) for r in rs],
           "max_coverage_absent": [round(max(x["coverage"] for x in r[2][1:]), 3) for r in rs]}
    out["frames_model0_found_refine"] = sum(0 in f for f in out["found_refine"])
    out["frames_model0_found_verify"] = sum(0 in f for f in out["found_verify"])
    out["false_detections_refine"] = sum(len([j for j in f if j]) for f in out["found_refine"])
    out["false_detections_verify"] = sum(len([j for j in f if j]) for f in out["found_verify"])
    db.close()
    for m in models:
        m.close()
    return out


def instances(calls=10, frames=10):
    """Every instance of a model (oslam_align_instances): ms without and with refinement next to oslam_align on the
    bench registration and on a 100k scene with 3 copies of the bench model (plus recall and false detections there,
    12 degree / 0.1 extent rule), the selection kernel alone on the largest kept-cell set of the tail, and the db50
    stream with db.find_instances per frame."""
    def med(f):
        f()
        ts = []
        for _ in range(calls):
            t = time.perf_counter(); f(); ts.append(1e3 * (time.perf_counter() - t))
        return float(np.median(ts))
    mp, mn = synth.make_model(0, 5000)
    d = synth.d_dist_for(mp, 0.025)
    ext = synth.bbox_extent(mp)
    out = {"config": "instance search (oslam_align_instances / oslam_db_align_instances)"}
    for name, k in (("bench_registration", 1), ("three_copies", 3)):
        sp, sn, poses = synth.make_scene([0], 100000, 2002, n_instances=k, instance_points=5000 if k == 1 else None,
                                         noise_sigma=0.1 * d)
        mo = ppf.Model(mp, mn, d_dist=d)
        sc = ppf.Scene(sp, sn, d_dist=d, ref_point_downsample_factor=8)
        T = mo.ppf_lookup(sc).copy()
        n_top = mo.stats["num_top"]
        r = {"kept_cells": int(n_top), "ms_align": med(lambda: mo.ppf_lookup(sc)),
             "ms_instances": med(lambda: mo.find_instances(sc, refine=False)),
             "ms_instances_refined": med(lambda: mo.find_instances(sc, refine=True))}
        found = mo.find_instances(sc)
        truths = [P for _, P in poses]
        matched, unmatched = evaluate.match_instances(found, truths, ext, dist_thresh_factor=0.1, rot_thresh=np.radians(12))
        r.update({"instances": len(found), "recall": sum(m is not None for m in matched) / len(truths),
                  "false_detections": len(unmatched), "align_recall": sum(found_at_reference_criterion(T, P, mp) for P in truths) / len(truths),
                  "scores": [round(i["score"], 1) for _, i in found], "fitness": [round(i["refine"]["fitness"], 3) for _, i in found]})
        out[name] = r
        mo.close()
        sc.close()
    n_models = 50
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    imgs = []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        imgs.append(synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1))
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)
    for tag, fn in (("align", lambda sc: db.align(sc)), ("find_instances", lambda sc: db.find_instances(sc)),
                    ("find_instances_no_refine", lambda sc: db.find_instances(sc, refine=False))):
        def frame(img):
            sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                      z_min=0.5, z_max=12.0, max_jump=0.08)
            r = fn(sc)
            sc.close()
            return r
        frame(imgs[0])
        t = time.perf_counter(); rs = [frame(im) for im in imgs]; el = time.perf_counter() - t
        out["db50_" + tag] = {"frames_per_s": frames / el}
        if tag == "find_instances":
            out["db50_" + tag]["instances_per_frame"] = [sum(len(x) for x in r) for r in rs]
    db.close()
    for m in models:
        m.close()
    return out


def arbitrate(frames=10):
    """Arbitration (oslam_db_arbitrate) on the db50 stream: db.align + db.refine + db.verify + db.arbitrate per frame
    (the members verification did not find are passed as skipped), the found sets before and after arbitration, and
    the same frames through the one call (db.detect).  Member 36 is the near twin of the rendered model 0."""
    n_models = 50
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    imgs = []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        imgs.append(synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1))
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)

    def scene_of(img):
        return ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                    z_min=0.5, z_max=12.0, max_jump=0.08)

    def frame(img):
        sc = scene_of(img)
        Ta, _ = db.align(sc)
        Tr, _, _ = db.refine(sc, Ta)
        view = ppf.View(img, 525.0, 525.0, 319.5, 239.5, z_min=0.5, z_max=12.0)
        _, found = db.verify(view, Tr)
        t = time.perf_counter()
        res, kept = db.arbitrate(view, np.where(found[:, None, None], Tr, np.float32(0)))
        ms = 1e3 * (time.perf_counter() - t)
        view.close()
        sc.close()
        return found, kept, res, ms

    def detect(img):
        sc = scene_of(img)
        view = ppf.View(img, 525.0, 525.0, 319.5, 239.5, z_min=0.5, z_max=12.0)
        det = db.detect(sc, view)
        view.close()
        sc.close()
        return det
    frame(imgs[0])
    t = time.perf_counter(); rs = [frame(im) for im in imgs]; el = time.perf_counter() - t
    detect(imgs[0])
    t = time.perf_counter(); ds = [detect(im) for im in imgs]; el_d = time.perf_counter() - t
    out = {"config": "arbitration (oslam_db_arbitrate) on the db50 stream", "frames": frames, "models": n_models,
           "frames_per_s_align_refine_verify_arbitrate": frames / el,
           "frames_per_s_detect": frames / el_d,
           "ms_arbitrate_per_frame_median": float(np.median([r[3] for r in rs])),
           "ms_arbitrate_in_library_median": float(np.median([r[2][0]["ms_total"] for r in rs])),
           "launches_per_call": [r[2][0]["launches"] for r in rs],
           "tile": [r[2][0]["tile"] for r in rs], "rounds": [r[2][0]["rounds"] for r in rs],
           "found_verify": [[int(j) for j in np.flatnonzero(r[0])] for r in rs],
           "kept_arbitrate": [[int(j) for j in np.flatnonzero(r[1])] for r in rs],
           "share_model0": [round(r[2][0]["share"], 3) for r in rs],
           "share_model36": [round(r[2][36]["share"], 3) for r in rs],
           "detect": [[(g["model"], g["instance"]) for g in det] for det in ds]}
    db.close()
    for m in models:
        m.close()
    return out


def explain(frames=10, calls=20):
    """The explain stage (oslam_db_explain) next to arbitration on the db50 stream (member 36 is the near twin of the
    rendered model 0): per frame the members verification found, the ones db.arbitrate keeps and the ones db.explain
    keeps over the same list, and both calls' ms; then ms_total of ppf.explain, ppf.arbitrate and ppf.render in the same
    run for 1 and 50 hypotheses (every member at its refined pose of frame 0), median of `calls` calls after 5."""
    n_models = 50
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    rng = synth.SplitMix64(93)
    imgs = []
    for f in range(frames):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = [0.5 * np.cos(0.7 * f), 0.3 * np.sin(0.7 * f), 5.5 + 0.1 * f]
        imgs.append(synth.render_depth(dense @ T[:3, :3].T + T[:3, 3], background_z=9.0, splat=1))
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)

    def frame(img):
        sc = ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                  z_min=0.5, z_max=12.0, max_jump=0.08)
        Ta, _ = db.align(sc)
        Tr, _, _ = db.refine(sc, Ta)
        view = ppf.View(img, 525.0, 525.0, 319.5, 239.5, z_min=0.5, z_max=12.0)
        _, found = db.verify(view, Tr)
        Tf = np.where(found[:, None, None], Tr, np.float32(0))
        t = time.perf_counter(); ares, akept = db.arbitrate(view, Tf); ms_a = 1e3 * (time.perf_counter() - t)
        t = time.perf_counter(); eres = db.explain(view, Tf); ms_e = 1e3 * (time.perf_counter() - t)
        view.close()
        sc.close()
        return dict(verified=[int(j) for j in np.flatnonzero(found)], kept_arbitrate=[int(j) for j in np.flatnonzero(akept)],
                    kept_explain=[j for j, r in enumerate(eres) if r["kept"]], ms_arbitrate=round(ms_a, 3), ms_explain=round(ms_e, 3),
                    conflict_rate={j: round(eres[j]["conflict_q"] / 65535.0, 3) for j in np.flatnonzero(found).tolist()},
                    share_explain={j: round(eres[j]["share"], 3) for j in np.flatnonzero(found).tolist()}), Tr
    frame(imgs[0])
    rows = []
    for f, im in enumerate(imgs):
        row, Tr = frame(im)
        rows.append(dict(frame=f, **row))
        if f == 0:
            T0 = Tr
    view = ppf.View(imgs[0], 525.0, 525.0, 319.5, 239.5, z_min=0.5, z_max=12.0)
    per_call = {}
    for n in (1, n_models):
        ms = {"explain": [], "arbitrate": [], "render": []}
        for k in range(calls + 5):
            ms["explain"].append(ppf.explain(models[:n], view, T0[:n])[0]["ms_total"])
            ms["arbitrate"].append(ppf.arbitrate(models[:n], view, T0[:n])[0][0]["ms_total"])
            r = ppf.render(models[:n], T0[:n], view)
            ms["render"].append(r.results[0]["ms_total"])
            r.close()
        per_call[n] = {k: round(float(np.median(v[5:])), 4) for k, v in ms.items()}
        per_call[n]["launches_explain"] = ppf.explain(models[:n], view, T0[:n])[0]["launches"]
    view.close()
    db.close()
    for m in models:
        m.close()
    return {"config": "explain (oslam_db_explain) next to arbitrate on the db50 stream", "frames": frames, "models": n_models,
            "per_frame": rows, "ms_total_median_640x480": per_call}


def track(frames=30, calls=20):
    """Tracking (oslam_db_track, oslam_tracker_step) on the db50 stream with smooth motion (synth.smooth_motion_poses: 3
    degrees and 0.5 d_dist per frame): (a) db.detect on every frame, (b) Tracker.step with detect_every 10, building the
    scene only on search frames, (c) db.track alone per call, inside the library and from Python, for 1 and for 50
    hypotheses, next to db.refine + db.verify on the same poses."""
    n_models = 50
    raw = [synth.make_model(k, 1500) for k in range(n_models)]
    d = synth.d_dist_for(raw[0][0], 0.05)
    grids = [ppf.voxel_grid(c[0], c[1], leaf=d) for c in raw]
    dense, _ = synth.make_model(0, 300000)
    poses = synth.smooth_motion_poses(d, frames=frames)
    imgs = [synth.render_depth(dense @ T[:3, :3].T.astype(np.float64) + T[:3, 3], background_z=9.0, splat=1) for T in poses]
    models = [ppf.Model(g[0], g[1], d_dist=d) for g in grids]
    db = ppf.Database(models)

    def scene_of(img):
        return ppf.Scene.from_depth(img, 525.0, 525.0, 319.5, 239.5, leaf=d, d_dist=0.0, ref_point_downsample_factor=4,
                                    z_min=0.5, z_max=12.0, max_jump=0.08)

    def view_of(img):
        return ppf.View(img, 525.0, 525.0, 319.5, 239.5, z_min=0.5, z_max=12.0, max_jump=0.08)

    def detect(img):
        sc, view = scene_of(img), view_of(img)
        det = db.detect(sc, view)
        view.close()
        sc.close()
        return det

    def tracked():
        tracker = ppf.Tracker(db, ppf.default_tracker_params(detect_every=10))
        rows = []
        for f, img in enumerate(imgs):
            view = view_of(img)
            sc = scene_of(img) if f % 10 == 0 or not rows or not rows[-1][0] else None
            tr, searched = tracker.step(view, sc)
            rows.append((tr, searched))
            if sc is not None:
                sc.close()
            view.close()
        tracker.close()
        return rows

    def err(T, f):
        Rd = T[:3, :3].astype(np.float64) @ poses[f][:3, :3].astype(np.float64).T
        s = np.linalg.norm([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]) / 2
        return (float(np.degrees(np.arctan2(s, (np.trace(Rd) - 1) / 2))), float(np.linalg.norm(T[:3, 3] - poses[f][:3, 3]) / d))
    detect(imgs[0])
    t = time.perf_counter(); ds = [detect(im) for im in imgs]; el_a = time.perf_counter() - t
    tracked()
    t = time.perf_counter(); rows = tracked(); el_b = time.perf_counter() - t
    errs = [max([err(x["T"], f) for x in tr if x["model"] == 0 and x["found"]] or [(None, None)]) for f, (tr, _) in enumerate(rows)]

    # (c) one call: frame 1 from the poses of frame 0 (every member at the rendered object's pose), 1 and 50 hypotheses
    view, sc = view_of(imgs[1]), scene_of(imgs[1])
    per_call = {}
    for H in (1, n_models):
        T0 = np.repeat(poses[0][None], H, axis=0)
        members = np.arange(H)
        sub = db if H == n_models else None
        db.track(view, members, T0)
        py, lib_ms, launches = [], [], 0
        for _ in range(calls):
            t = time.perf_counter()
            _, res, _ = db.track(view, members, T0)
            py.append(1e3 * (time.perf_counter() - t))
            lib_ms.append(res[0]["ms_total"])
            launches = res[0]["launches"]
        per_call["track_%d" % H] = {"ms_python_median": float(np.median(py)), "ms_library_median": float(np.median(lib_ms)),
                                    "launches": launches, "iterations": [r["iterations"] for r in res][:4]}
        if sub is not None:
            Tr, rr, _ = db.refine(sc, T0)
            py_r, lib_r, py_v, lib_v = [], [], [], []
            for _ in range(calls):
                t = time.perf_counter(); Tr, rr, _ = db.refine(sc, T0); py_r.append(1e3 * (time.perf_counter() - t))
                lib_r.append(rr[0]["ms_total"])
                t = time.perf_counter(); vr, _ = db.verify(view, Tr); py_v.append(1e3 * (time.perf_counter() - t))
                lib_v.append(vr[0]["ms_total"])
            per_call["refine_%d" % H] = {"ms_python_median": float(np.median(py_r)), "ms_library_median": float(np.median(lib_r)),
                                         "launches": rr[0]["launches"]}
            per_call["verify_%d" % H] = {"ms_python_median": float(np.median(py_v)), "ms_library_median": float(np.median(lib_v)),
                                         "launches": vr[0]["launches"]}
    m0 = models[0]
    Tr, rr = m0.refine(sc, poses[0]); m0.verify(view, Tr)
    py_r, lib_r, py_v, lib_v = [], [], [], []
    for _ in range(calls):
        t = time.perf_counter(); Tr, rr = m0.refine(sc, poses[0]); py_r.append(1e3 * (time.perf_counter() - t)); lib_r.append(rr["ms_total"])
        t = time.perf_counter(); vr = m0.verify(view, Tr); py_v.append(1e3 * (time.perf_counter() - t)); lib_v.append(vr["ms_total"])
    per_call["refine_1"] = {"ms_python_median": float(np.median(py_r)), "ms_library_median": float(np.median(lib_r)), "launches": rr["launches"]}
    per_call["verify_1"] = {"ms_python_median": float(np.median(py_v)), "ms_library_median": float(np.median(lib_v)), "launches": vr["launches"]}
    view.close()
    sc.close()
    out = {"config": "tracking (oslam_db_track, oslam_tracker_step) on the db50 stream with smooth motion", "frames": frames,
           "models": n_models, "frames_per_s_detect_every_frame": frames / el_a, "frames_per_s_tracker_detect_every_10": frames / el_b,
           "searched_frames": [f for f, (_, s) in enumerate(rows) if s],
           "tracks_per_frame": [[(x["id"], x["model"], x["found"]) for x in tr] for tr, _ in rows],
           "model0_rot_deg_trans_d_dist": [(None if e[0] is None else round(e[0], 3), None if e[1] is None else round(e[1], 3)) for e in errs],
           "detect": [[(g["model"], g["instance"]) for g in det] for det in ds], "per_call": per_call}
    db.close()
    for m in models:
        m.close()
    return out


def camera(frames=30, calls=20):
    """Camera motion (oslam_view_egomotion, oslam_tracker_step_cam) on the static world of tests/camera_ref.py: the camera
    sweeps 9 frames of 3 degrees and 3 cm out and back again, 30 frames in all.  (a) egomotion per call on one pair, inside
    the library and from Python, with the launches; (b) the stream: egomotion on every pair and its chained error;
    (c) Tracker.step on one object of a 3-model database with T_cam from (b) and without."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import refine_ref
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    order = [abs((f + 9) % 18 - 9) for f in range(frames)]          # 0 1 .. 9 8 .. 0 1 ..
    rendered = [E.render(synth, world, T) for T in sweep]
    traj, imgs = [sweep[k] for k in order], [rendered[k] for k in order]
    cam = E.CAM

    def view_of(img):
        return ppf.View(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"], z_max=cam["z_max"],
                        max_jump=E.MAX_JUMP)
    views = [view_of(im) for im in imgs]
    ppf.egomotion(views[0], views[1])
    py, lib_ms = [], []
    for _ in range(calls):
        t = time.perf_counter(); _, r = ppf.egomotion(views[0], views[1]); py.append(1e3 * (time.perf_counter() - t))
        lib_ms.append(r["ms_total"])
    per_call = {"ms_python_median": float(np.median(py)), "ms_library_median": float(np.median(lib_ms)),
                "launches": r["launches"], "iterations": r["iterations"]}
    t = time.perf_counter()
    motions = [ppf.egomotion(views[f - 1], views[f]) for f in range(1, frames)]
    el = time.perf_counter() - t
    chain, errs = np.eye(4), []
    for f, (T, r) in enumerate(motions, 1):
        chain = T.astype(np.float64) @ chain
        e = refine_ref.pose_error(T, E.truth(traj[f - 1], traj[f])) + refine_ref.pose_error(chain, E.truth(traj[0], traj[f]))
        errs.append([round(x, 5) for x in e] + [round(r["overlap"], 3), r["ok"]])

    clouds = [synth.make_model(k, 1500) for k in range(3)]
    clouds = [(np.ascontiguousarray(p * np.float32(E.OBJECT_SCALE)), n) for p, n in clouds]
    d = synth.d_dist_for(clouds[0][0], 0.05)
    models = [ppf.Model(p, n, d_dist=d) for p, n in clouds]
    db = ppf.Database(models)
    k = 1                                                           # the object nearest the camera
    poses = [(np.linalg.inv(Twc) @ E.object_pose(synth, 0, k)).astype(np.float32) for Twc in traj]
    streams = {}
    for name in ("with_T_cam", "without"):
        tracker = ppf.Tracker(db)
        tracker.update([dict(model=k, T=poses[0])])
        rows = []
        t = time.perf_counter()
        for f in range(1, frames):
            T, r = motions[f - 1]
            tr, _ = tracker.step(views[f], T_cam=T if name == "with_T_cam" and r["ok"] else None)
            rows.append(tr)
        el_t = time.perf_counter() - t
        streams[name] = {"frames_per_s_tracker_step": (frames - 1) / el_t,
                         "found_frames": sum(bool(tr and tr[0]["found"]) for tr in rows),
                         "rot_deg_trans_d_dist": [None if not (tr and tr[0]["found"]) else
                                                  [round(refine_ref.pose_error(tr[0]["T"], poses[f])[0], 3),
                                                   round(refine_ref.pose_error(tr[0]["T"], poses[f])[1] / d, 3)]
                                                  for f, tr in enumerate(rows, 1)]}
        if name == "with_T_cam":
            streams[name]["camera_rot_deg_trans_m"] = [round(x, 5) for x in refine_ref.pose_error(tracker.camera(), traj[-1])]
        tracker.close()
    out = {"config": "camera motion (oslam_view_egomotion, oslam_tracker_step_cam): static world, 3 degrees and 3 cm per frame",
           "frames": frames, "egomotion_per_call": per_call, "egomotion_pairs_per_s": (frames - 1) / el,
           "pair_rot_deg_trans_m_chained_rot_trans_overlap_ok": errs, "tracked_object": k, "tracker": streams}
    for v in views:
        v.close()
    db.close()
    for m in models:
        m.close()
    return out


def fusion(calls=20):
    """The fusion stage (oslam_volume_integrate / _raycast / _track) on the static world of tests/camera_ref.py: a 256^3
    volume of 3.6 cm voxels over the room, the 640x480 stream out and back.  The integration figure counts the words the
    rule loads and stores (8 bytes per updated voxel); once the 64 MiB volume is resident it is a cache figure."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import refine_ref
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    order = list(range(10)) + list(range(8, -1, -1))
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    eye = np.eye(4, dtype=np.float32)

    def raycast(T):
        return vol.raycast(T, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 640, 480, z_min=cam["z_min"], z_max=cam["z_max"],
                           max_jump=E.MAX_JUMP)
    vol.integrate(rendered[0], eye)
    integ, upd = [], 0
    for _ in range(calls):
        r = vol.integrate(rendered[0], eye)
        integ.append(r["ms_total"])
        upd = r["updated"]
    rays = []
    for _ in range(calls + 1):
        v, r = raycast(eye)
        rays.append(r["ms_total"])
        hits = (r["hits"], r["normals"])
        v.close()
    trk = [vol.track(rendered[1], eye)[1] for _ in range(calls + 1)]
    vol.reset()
    t = time.perf_counter()
    steps = [vol.step(rendered[k]) for k in order]
    el = time.perf_counter() - t
    end = refine_ref.pose_error(steps[-1][0], sweep[0])
    ms_i = float(np.median(integ))
    out = {"config": "fusion (oslam_volume): 256^3 volume of 3.6 cm voxels, 640x480 stream, 3 degrees and 3 cm per frame",
           "volume": spec, "integrate_ms_median": ms_i, "integrate_voxels_updated": upd,
           "integrate_rule_bytes_per_s": 8.0 * upd / (ms_i * 1e-3), "hbm_peak_bytes_per_s": 8e12,
           "raycast_ms_median": float(np.median(rays[1:])), "raycast_hits_normals": hits,
           "track_ms_median": float(np.median([r["ms_total"] for r in trk[1:]])), "track_launches": trk[-1]["launches"],
           "track_iterations": trk[-1]["iterations"], "step_frames_per_s": len(order) / el,
           "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "step_overlap": [None if r is None else round(r["overlap"], 3) for _, r in steps],
           "end_pose_rot_deg_trans_m": [round(x, 5) for x in end]}
    for v in rendered:
        v.close()
    vol.close()
    return out


def colour(calls=20):
    """Colour next to the TSDF (oslam_volume_integrate_colour, oslam_volume_paint_view, oslam_volume_colours) on the fusion
    configuration's volume and stream; every frame carries the colour image of tests/colour_world.py.  The yardstick of
    the colour pass is the plain integrate of the same volume in the same run: the pass walks the same voxels, loads and
    stores one word per voxel inside its band and does integer arithmetic on it.  Then the calibration room of
    tests/test_colour_host.py (320x240, 5 cm voxels, ten frames at their true poses) as a coloured mesh, written with
    ply_write_mesh(..., rgb=), and its colour error against the colour function."""
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import colour_world as W
    import volume_ref as V
    world = E.make_world(synth, 0)
    rgb = W.world_colours(world, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    order = list(range(10)) + list(range(8, -1, -1))
    cam = E.CAM
    rendered = []
    for T in sweep:
        depth, img, ok = W.render(synth, world, rgb, T)
        v = ppf.View(depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"], z_max=cam["z_max"], max_jump=E.MAX_JUMP)
        v.set_colour(img, ok)
        rendered.append(v)
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    vol.enable_colour()
    eye = np.eye(4, dtype=np.float32)
    vol.integrate(rendered[0], eye)
    vol.integrate(rendered[0], eye, colour=rendered[0])
    plain, both, r = [], [], None
    for _ in range(calls):                                       # alternately, so that both see the same machine
        plain.append(vol.integrate(rendered[0], eye)["ms_total"])
        r = vol.integrate(rendered[0], eye, colour=rendered[0])
        both.append(r["ms_total"])
    rv, rres = vol.raycast(eye, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 640, 480, z_min=cam["z_min"], z_max=cam["z_max"],
                           max_jump=E.MAX_JUMP)
    paint, painted = [], 0
    for _ in range(calls + 1):
        t = time.perf_counter()
        painted = vol.paint(rv, eye)
        paint.append((time.perf_counter() - t) * 1e3)
    rv.close()
    xyz, _, sres = vol.surface()
    cols, valid = [], None
    for _ in range(calls + 1):
        t = time.perf_counter()
        _, valid = vol.colours(xyz)
        cols.append((time.perf_counter() - t) * 1e3)
    fps = {}
    for name, kw in (("plain", lambda k: {}), ("colour", lambda k: dict(colour=rendered[k]))):
        for _ in range(2):                                        # the first pass warms up
            vol.reset()
            t = time.perf_counter()
            steps = [vol.step(rendered[k], **kw(k)) for k in order]
            fps[name] = len(order) / (time.perf_counter() - t)
        fps[name + "_ok"] = [None if r_ is None else r_["ok"] for _, r_ in steps]
    ms_p, ms_b = float(np.median(plain)), float(np.median(both))
    out = {"config": "colour (oslam_volume_integrate_colour): the fusion configuration's 256^3 volume and 640x480 stream with colour",
           "volume": spec, "colour_params": {"max_weight": vol.colour_params.max_weight, "band": vol.colour_params.band},
           "integrate_ms_median": ms_p, "integrate_colour_ms_median": ms_b, "colour_pass_ms": ms_b - ms_p,
           "colour_pass_over_integrate": (ms_b - ms_p) / ms_p, "voxels_updated": r["updated"], "voxels_coloured": r["coloured"],
           "paint_ms_median": float(np.median(paint[1:])), "paint_pixels": painted, "raycast_hits": rres["hits"],
           "colours_ms_median": float(np.median(cols[1:])), "colours_points": len(xyz), "colours_valid": int(valid.sum()),
           "step_frames_per_s": fps["plain"], "step_colour_frames_per_s": fps["colour"], "step_ok": fps["plain_ok"],
           "step_colour_ok": fps["colour_ok"]}
    for v in rendered:
        v.close()
    vol.close()
    # the calibration room as a coloured mesh
    room = V.room_volume(0, cls=ppf.Volume)
    room.enable_colour()
    for T in sweep:
        depth, img, ok = W.render(synth, world, rgb, T, **V.SMALL)
        c = V.SMALL_CAM
        v = ppf.View(depth, c["fx"], c["fy"], c["cx"], c["cy"], z_min=c["z_min"], z_max=c["z_max"], max_jump=E.MAX_JUMP)
        v.set_colour(img, ok)
        room.integrate(v, T.astype(np.float32), colour=v)
        v.close()
    mx, mn, tri, mres, mrgb, mvalid = room.mesh(colour=True)
    err = np.abs(mrgb[mvalid].astype(np.float64) - W.colour(mx.astype(np.float64), 0)[mvalid])
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "room.ply")
        ppf.ply_write_mesh(f, mx, mn, tri, rgb=mrgb)
        size = os.path.getsize(f)
        back = ppf.ply_read_mesh(f)
    out["calibration_mesh"] = {"vertices": len(mx), "triangles": len(tri), "with_colour": float(mvalid.mean()),
                               "error_median_levels": float(np.median(err)), "error_p95_levels": float(np.percentile(err, 95)),
                               "ply_bytes": size, "ply_geometry_read_back": bool(back[0].tobytes() == mx.tobytes() and
                                                                                 back[2].tobytes() == tri.tobytes())}
    room.close()
    return out


def surface(calls=20):
    """Whole-volume surface extraction (oslam_volume_surface / oslam_scene_from_volume) on the fusion configuration's
    256^3 volume after its out-and-back stream.  The yardstick is one integrate on the same volume: both stream the
    64 MiB of words, the extraction twice (count and emit)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    integ = [vol.integrate(rendered[0], vol.T)["ms_total"] for _ in range(calls + 1)]
    leaf = 0.1
    vol.surface()
    ppf.Scene.from_volume(vol, leaf).close()
    surf, scene, n_scene = [], [], 0
    for _ in range(calls):
        t = time.perf_counter()
        xyz, nrm, res = vol.surface()
        surf.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        sc = ppf.Scene.from_volume(vol, leaf)
        scene.append((time.perf_counter() - t) * 1e3)
        n_scene = sc.numPoints()
        sc.close()
    out = {"config": "surface (oslam_volume_surface): the fusion configuration's 256^3 volume after its 19-frame stream",
           "volume": spec, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "crossings": res["crossings"], "points": res["points"], "launches": res["launches"],
           "surface_ms_median": float(np.median(surf)), "surface_ms_median_library": res["ms_total"],
           "scene_from_volume_ms_median": float(np.median(scene)), "scene_leaf": leaf, "scene_points": n_scene,
           "integrate_ms_median": float(np.median(integ[1:])), "volume_bytes": 4 * 256 ** 3}
    for v in rendered:
        v.close()
    vol.close()
    return out


def mesh(calls=20):
    """Whole-volume mesh extraction (oslam_volume_mesh) on the fusion configuration's 256^3 volume after its out-and-back
    stream: the median of `calls` calls of Volume.mesh with and without normals and, in the same run, of Volume.surface
    and of one integrate (the yardsticks).  Each Volume call is the two library calls it makes (count, then fill); the
    four alternate, so that drift hits them alike."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    vol.integrate(rendered[0], vol.T)
    vol.mesh()
    vol.mesh(normals=False)
    vol.surface()
    with_n, without_n, surf, integ = [], [], [], []
    for _ in range(calls):
        t = time.perf_counter(); xyz, nrm, tri, res = vol.mesh(); with_n.append(1e3 * (time.perf_counter() - t))
        lib_n = res["ms_total"]
        t = time.perf_counter(); _, _, _, res0 = vol.mesh(normals=False); without_n.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); _, _, sres = vol.surface(); surf.append(1e3 * (time.perf_counter() - t))
        integ.append(vol.integrate(rendered[0], vol.T)["ms_total"])
    referenced = int(len(np.unique(tri)))
    out = {"config": "mesh (oslam_volume_mesh): the fusion configuration's 256^3 volume after its 19-frame stream",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "vertices": res["vertices"], "triangles": res["triangles"], "cubes": res["cubes"], "launches": res["launches"],
           "vertices_referenced": referenced, "vertices_with_normal": int((nrm != 0).any(axis=1).sum()),
           "mesh_ms_median": float(np.median(with_n)), "mesh_second_call_ms_library": lib_n,
           "mesh_without_normals_ms_median": float(np.median(without_n)), "mesh_without_normals_second_call_ms_library": res0["ms_total"],
           "surface_ms_median": float(np.median(surf)), "surface_points": sres["points"],
           "integrate_ms_median": float(np.median(integ)), "volume_bytes": 4 * 256 ** 3,
           "mesh_over_surface": float(np.median(with_n) / np.median(surf))}
    for v in rendered:
        v.close()
    vol.close()
    return out


def shift(calls=20):
    """The shifting window (oslam_volume_shift, oslam_volume_leaving) on the fusion configuration's 256^3 volume after its
    out-and-back stream: the median of `calls` calls of Volume.shift, by (8, 0, 0) and (-8, 0, 0) alternately, of
    Volume.leaving((8, 0, 0)) and, in the same run, of one integrate and of Volume.surface (the yardsticks); the four
    alternate, so that drift hits them alike.  The shift's rule figure counts 4 bytes loaded and 4 stored per kept voxel
    (w > 0 after the shift) and 4 stored per other one; its traffic figure counts what the kernel moves, 4 loaded and 4
    stored per word that comes from inside the volume, seen or not, and 4 stored per word that does not.  The two
    64 MiB buffers fit the Infinity Cache, so both are cache figures.  The first shifts clear the slabs that went out; the volume is restored
    before leaving and surface are timed."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    q, w = vol.voxels()
    vol.integrate(rendered[0], vol.T)
    vol.surface()
    vol.leaving((8, 0, 0))
    vol.shift((8, 0, 0))                                            # allocates the second buffer
    vol.shift((-8, 0, 0))
    vol.set_voxels(q, w)
    leave, surf, integ = [], [], []
    for _ in range(calls):
        t = time.perf_counter(); _, _, lres = vol.leaving((8, 0, 0)); leave.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); _, _, sres = vol.surface(); surf.append(1e3 * (time.perf_counter() - t))
        integ.append(vol.integrate(rendered[0], vol.T)["ms_total"])
    fwd, back, kept = [], [], 0
    for k in range(calls):
        r = vol.shift((8, 0, 0) if k % 2 == 0 else (-8, 0, 0))
        (fwd if k % 2 == 0 else back).append(r["ms_total"])
        kept = r["kept"]
    n_vox = 256 ** 3
    moved = (256 - 8) * 256 * 256                                   # words that come from inside the volume
    ms_s = float(np.median(fwd + back))
    out = {"config": "shift (oslam_volume_shift, oslam_volume_leaving): the fusion configuration's 256^3 volume after its 19-frame stream",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "shift_ms_median": ms_s, "shift_plus8_ms_median": float(np.median(fwd)), "shift_minus8_ms_median": float(np.median(back)),
           "shift_kept_last": kept, "shift_rule_bytes_per_s": (8.0 * kept + 4.0 * (n_vox - kept)) / (ms_s * 1e-3),
           "shift_traffic_bytes": 8 * moved + 4 * (n_vox - moved),
           "shift_traffic_bytes_per_s": (8.0 * moved + 4.0 * (n_vox - moved)) / (ms_s * 1e-3), "hbm_peak_bytes_per_s": 8e12,
           "leaving_ms_median": float(np.median(leave)), "leaving_second_call_ms_library": lres["ms_total"],
           "leaving_crossings": lres["crossings"], "leaving_points": lres["points"], "leaving_launches": lres["launches"],
           "surface_ms_median": float(np.median(surf)), "surface_crossings": sres["crossings"], "surface_points": sres["points"],
           "integrate_ms_median": float(np.median(integ)), "volume_bytes": 4 * n_vox,
           "shift_over_integrate": ms_s / float(np.median(integ)),
           "leaving_over_surface": float(np.median(leave) / np.median(surf))}
    for v in rendered:
        v.close()
    vol.close()
    return out


def reload(calls=20):
    """The shift through the voxel store (oslam_volume_shift_world) on the shift configuration's 256^3 volume after its
    out-and-back stream: the median of `calls` calls of Volume.shift(+-8 on one axis, world=w), out and back alternately,
    and, in the same run and interleaved with them, of the plain Volume.shift by the same steps (the yardstick); what
    the store adds is the ratio of the two medians.  The pair runs on x and, where another axis has more seen voxels in
    its outer 8 planes, on that axis too, so that records really go out and come back; which axis that is, and the
    counts, are in the output.  stored and reloaded are per call; the store's bytes are read after an outward call.
    The volume is restored between the two kinds of shift: the plain one forgets."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    q, w = vol.voxels()
    seen = w > 0                                                    # [nz, ny, nx]
    slab = {"x-": int(seen[:, :, :8].sum()), "x+": int(seen[:, :, -8:].sum()), "y-": int(seen[:, :8, :].sum()),
            "y+": int(seen[:, -8:, :].sum()), "z-": int(seen[:8, :, :].sum()), "z+": int(seen[-8:, :, :].sum())}
    best = max(slab, key=lambda k: slab[k])
    axis, sign = "xyz".index(best[0]), 1 if best[1] == "-" else -1  # a positive shift moves the low planes out
    pairs = [("x", (8, 0, 0))]
    if best != "x-":
        s = [0, 0, 0]
        s[axis] = 8 * sign
        pairs.append((best, tuple(s)))
    store = ppf.World(vol)
    out = {"config": "reload (oslam_volume_shift_world): the shift configuration's 256^3 volume after its 19-frame stream",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "seen_in_the_outer_8_planes": slab, "axis_with_surface": best, "pairs": []}
    for name, s in pairs:
        back = tuple(-x for x in s)
        vol.shift(s, store); vol.shift(back, store)                 # the second buffer, the staging buffers, the bricks
        vol.shift(s); vol.shift(back)
        vol.set_voxels(q, w)
        ms_w, ms_p, lib_w, stored, reloaded, launches, store_bytes, store_voxels = [], [], [], [], [], [], 0, 0
        for k in range(calls):
            t = time.perf_counter(); r = vol.shift(s if k % 2 == 0 else back, store); ms_w.append(1e3 * (time.perf_counter() - t))
            lib_w.append(r["ms_total"]); stored.append(r["stored"]); reloaded.append(r["reloaded"]); launches.append(r["launches"])
            if k % 2 == 0:
                st = store.stats()
                store_bytes, store_voxels = st["bytes"], st["voxels"]
        for k in range(calls):                                      # the plain shift forgets: timed after, on the same window
            t = time.perf_counter(); vol.shift(s if k % 2 == 0 else back); ms_p.append(1e3 * (time.perf_counter() - t))
        vol.set_voxels(q, w)
        inter_w, inter_p = [], []
        for k in range(calls):                                      # interleaved: one pair through the store, one plain pair
            t = time.perf_counter(); vol.shift(s, store); vol.shift(back, store); inter_w.append(0.5e3 * (time.perf_counter() - t))
            t = time.perf_counter(); vol.shift(s); vol.shift(back); inter_p.append(0.5e3 * (time.perf_counter() - t))
            vol.set_voxels(q, w)
        out["pairs"].append({"axis": name, "shift": list(s), "world_shift_ms_median": float(np.median(ms_w)),
                             "world_shift_ms_library_median": float(np.median(lib_w)), "plain_shift_ms_median": float(np.median(ms_p)),
                             "world_over_plain": float(np.median(ms_w) / np.median(ms_p)),
                             "interleaved_world_ms_median": float(np.median(inter_w)), "interleaved_plain_ms_median": float(np.median(inter_p)),
                             "interleaved_world_over_plain": float(np.median(inter_w) / np.median(inter_p)),
                             "stored_out_back": [stored[0], stored[1]], "reloaded_out_back": [reloaded[0], reloaded[1]],
                             "launches_out_back": [launches[0], launches[1]], "store_bytes": store_bytes, "store_voxels": store_voxels})
        store.clear()
    for v in rendered:
        v.close()
    store.close()
    vol.close()
    return out


def worldsurface(calls=20):
    """The surface of the whole map (oslam_world_surface) on the reload configuration's map after its stream: the 256^3
    volume after the out-and-back stream, shifted through a store by (64, 0, 0) so that a slab of the surface lies in
    the store.  In one run and alternately, so that drift hits both alike: the median of `calls` calls of
    World.surface(vol) and of Volume.surface(), which sees the window alone (the yardstick).  The brick counts, the
    points of both and the library's own clock are in the output."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    store = ppf.World(vol)
    _, _, before = vol.surface()
    moved = vol.shift((64, 0, 0), store)
    store.surface(vol)                                              # the staging buffer and the kept device blocks
    vol.surface()
    ms_w, ms_v, lib_w = [], [], []
    for _ in range(calls):
        t = time.perf_counter(); pw, _ = store.surface(vol); ms_w.append(1e3 * (time.perf_counter() - t))
        lib_w.append(store.last_surface["ms_total"])
        t = time.perf_counter(); pv, _, vres = vol.surface(); ms_v.append(1e3 * (time.perf_counter() - t))
    t = time.perf_counter(); store.surface(vol, keys=True); ms_keys = 1e3 * (time.perf_counter() - t)
    wres, st = store.last_surface, store.stats()
    out = {"config": "worldsurface (oslam_world_surface): the reload configuration's 256^3 map after its 19-frame stream, shifted by (64, 0, 0) through the store",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "stored_by_the_shift": moved["stored"], "store": st,
           "world_surface_ms_median": float(np.median(ms_w)), "world_surface_ms_library_median": float(np.median(lib_w)),
           "world_surface_with_keys_ms_once": ms_keys, "volume_surface_ms_median": float(np.median(ms_v)),
           "world_over_volume": float(np.median(ms_w) / np.median(ms_v)),
           "bricks": wres["bricks"], "window_bricks": wres["window_bricks"], "store_bricks": st["bricks"], "launches": wres["launches"],
           "world_crossings": wres["crossings"], "world_points": len(pw), "window_crossings": vres["crossings"], "window_points": len(pv),
           "points_before_the_shift": before["points"], "brick_bytes_on_device": 2048 * wres["bricks"], "store_bytes_over_the_link": 2048 * st["bricks"]}
    for v in rendered:
        v.close()
    store.close()
    vol.close()
    return out


def worldraycast(calls=20):
    """The ray cast of the whole map (oslam_world_raycast) on worldsurface's map: the reload configuration's 256^3 volume
    after its out-and-back stream, shifted through a store by (64, 0, 0).  In one run and alternately, so that drift hits
    both alike: the median of `calls` calls of World.raycast(vol) at 640 x 480 from the current camera pose and of
    Volume.raycast of the same window from the same pose (the yardstick: code this configuration's subject does not
    touch).  The same pair once from the stream's first pose, where the window alone sees little.  The map's share of a
    call is the median of the same call with an image of one pixel: the table, the bricks over the host link and
    k_brick_window are all there, the march is not.  Kernel times proper come from a kernel trace of this configuration in
    a run of its own."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    store = ppf.World(vol)
    moved = vol.shift((64, 0, 0), store)
    kw = dict(z_min=cam["z_min"], z_max=cam["z_max"], max_jump=E.MAX_JUMP)
    size = (cam["fx"], cam["fy"], cam["cx"], cam["cy"], 640, 480)

    def both(T, n):
        ms_w, ms_v, lib_w, lib_v, ms_1 = [], [], [], [], []
        for _ in range(n):
            t = time.perf_counter(); v, wres = store.raycast(T, *size, vol=vol, **kw); ms_w.append(1e3 * (time.perf_counter() - t))
            v.close(); lib_w.append(wres["ms_total"])
            t = time.perf_counter(); v, vres = vol.raycast(T, *size, **kw); ms_v.append(1e3 * (time.perf_counter() - t))
            v.close(); lib_v.append(vres["ms_total"])
            t = time.perf_counter(); v, _ = store.raycast(T, cam["fx"], cam["fy"], 0.0, 0.0, 1, 1, vol=vol, **kw)
            ms_1.append(1e3 * (time.perf_counter() - t)); v.close()
        return {"world_raycast_ms_median": float(np.median(ms_w)), "world_raycast_ms_library_median": float(np.median(lib_w)),
                "volume_raycast_ms_median": float(np.median(ms_v)), "volume_raycast_ms_library_median": float(np.median(lib_v)),
                "world_over_volume": float(np.median(ms_w) / np.median(ms_v)),
                "world_raycast_one_pixel_ms_median": float(np.median(ms_1)),
                "world_raycast_minus_one_pixel_ms": float(np.median(ms_w) - np.median(ms_1)),
                "world_hits": wres["hits"], "world_normals": wres["normals"], "window_hits": vres["hits"], "window_normals": vres["normals"],
                "launches": wres["launches"], "box_lo": wres["box_lo"], "box_hi": wres["box_hi"]}

    both(vol.T, 3)                                                  # the staging buffer, the kept device blocks, the code objects
    now = both(vol.T, calls)
    first = both(np.eye(4, dtype=np.float32), 3)
    st = store.stats()
    out = {"config": "worldraycast (oslam_world_raycast): the reload configuration's 256^3 map after its 19-frame stream, shifted by (64, 0, 0) through the store",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps], "image": [640, 480],
           "stored_by_the_shift": moved["stored"], "store": st, "store_bricks": st["bricks"],
           "store_bytes_over_the_link": 2048 * st["bricks"], "current_pose": now, "first_pose_3_calls": first}
    for v in rendered:
        v.close()
    store.close()
    vol.close()
    return out


def worldmesh(calls=20):
    """The mesh of the whole map (oslam_world_mesh) on worldsurface's map: the reload configuration's 256^3 volume after
    its out-and-back stream, shifted through a store by (64, 0, 0).  In one run and alternately, so that drift hits
    both alike: the median of `calls` calls of World.mesh(vol) and of World.surface(vol); then, alternately as well,
    Volume.mesh() and Volume.surface(), which see the window alone.  Vertices, triangles, cubes, bricks and the
    library's own clock are in the output."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    world = E.make_world(synth, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                         z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in sweep]
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    steps = [vol.step(rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    store = ppf.World(vol)
    moved = vol.shift((64, 0, 0), store)
    store.mesh(vol); store.surface(vol)                             # the staging buffer and the kept device blocks
    vol.mesh(); vol.surface()
    ms_m, ms_s, lib_m, lib_s, ms_vm, ms_vs = [], [], [], [], [], []
    for _ in range(calls):
        t = time.perf_counter(); store.mesh(vol); ms_m.append(1e3 * (time.perf_counter() - t))
        lib_m.append(store.last_mesh["ms_total"])
        t = time.perf_counter(); store.surface(vol); ms_s.append(1e3 * (time.perf_counter() - t))
        lib_s.append(store.last_surface["ms_total"])
    for _ in range(calls):
        t = time.perf_counter(); _, _, _, vm = vol.mesh(); ms_vm.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); _, _, vs = vol.surface(); ms_vs.append(1e3 * (time.perf_counter() - t))
    t = time.perf_counter(); store.mesh(vol, normals=False); ms_bare = 1e3 * (time.perf_counter() - t)
    mres, sres, st = store.last_mesh, store.last_surface, store.stats()
    out = {"config": "worldmesh (oslam_world_mesh): the reload configuration's 256^3 map after its 19-frame stream, shifted by (64, 0, 0) through the store",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "stored_by_the_shift": moved["stored"], "store": st,
           "world_mesh_ms_median": float(np.median(ms_m)), "world_mesh_ms_library_median": float(np.median(lib_m)),
           "world_surface_ms_median": float(np.median(ms_s)), "world_surface_ms_library_median": float(np.median(lib_s)),
           "world_mesh_over_world_surface": float(np.median(ms_m) / np.median(ms_s)),
           "world_mesh_without_normals_ms_once": ms_bare,
           "volume_mesh_ms_median": float(np.median(ms_vm)), "volume_surface_ms_median": float(np.median(ms_vs)),
           "volume_mesh_over_volume_surface": float(np.median(ms_vm) / np.median(ms_vs)),
           "world_mesh_over_volume_mesh": float(np.median(ms_m) / np.median(ms_vm)),
           "vertices": mres["vertices"], "triangles": mres["triangles"], "cubes": mres["cubes"], "bricks": mres["bricks"],
           "window_bricks": mres["window_bricks"], "store_bricks": st["bricks"], "launches": mres["launches"],
           "world_surface_points": sres["points"], "window_vertices": vm["vertices"], "window_triangles": vm["triangles"],
           "window_cubes": vm["cubes"], "window_points": vs["points"]}
    for v in rendered:
        v.close()
    store.close()
    vol.close()
    return out


def worldcolour(calls=20):
    """Colour through the voxel store and the colour of the whole map (oslam_volume_shift_world with a colour store,
    oslam_world_colours) on the reload and worldmesh configurations' 256^3 map, fused with the colour images of
    tests/colour_world.py.  Two measurements, each against its yardstick in the same run and alternately, so that drift
    hits both alike.  The shift pair (+-8 on x and, as in reload, on the axis with the most seen voxels in its outer 8
    planes) of the coloured volume through a colour store next to the same pair through a plain store: medians of `calls`
    pairs, the records and launches of both.  Then, with the window moved by (64, 0, 0) through the colour store:
    World.colours on the vertices of World.mesh(vol) next to Volume.colours on the vertices of Volume.mesh(), per call
    and per point."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import colour_world as W
    world = E.make_world(synth, 0)
    rgb = W.world_colours(world, 0)
    sweep = E.trajectory(synth, 0, frames=10)
    cam = E.CAM
    rendered = []
    for T in sweep:
        depth, img, ok = W.render(synth, world, rgb, T)
        v = ppf.View(depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"], z_max=cam["z_max"], max_jump=E.MAX_JUMP)
        v.set_colour(img, ok)
        rendered.append(v)
    spec = dict(nx=256, ny=256, nz=256, voxel=0.036, origin=[-2.9, -4.3, 0.3], mu=0.288)
    vol = ppf.Volume(**spec)
    vol.enable_colour()
    steps = [vol.step(rendered[k], colour=rendered[k]) for k in list(range(10)) + list(range(8, -1, -1))]
    q, w = vol.voxels()
    c = vol.colour_words()
    seen = w > 0                                                    # [nz, ny, nx]
    slab = {"x-": int(seen[:, :, :8].sum()), "x+": int(seen[:, :, -8:].sum()), "y-": int(seen[:, :8, :].sum()),
            "y+": int(seen[:, -8:, :].sum()), "z-": int(seen[:8, :, :].sum()), "z+": int(seen[-8:, :, :].sum())}
    best = max(slab, key=lambda k: slab[k])
    axis, sign = "xyz".index(best[0]), 1 if best[1] == "-" else -1  # a positive shift moves the low planes out
    pairs = [("x", (8, 0, 0))]
    if best != "x-":
        s = [0, 0, 0]
        s[axis] = 8 * sign
        pairs.append((best, tuple(s)))
    cstore, pstore = ppf.World(vol, colour=True), ppf.World(vol)
    out = {"config": "worldcolour (oslam_volume_shift_world through a colour store, oslam_world_colours): the reload configuration's 256^3 "
                     "volume after its 19-frame stream, fused with colour",
           "volume": spec, "calls": calls, "step_ok": [None if r is None else r["ok"] for _, r in steps],
           "coloured_voxels": int((c >> np.uint32(24) != 0).sum()), "seen_voxels": int(seen.sum()),
           "seen_in_the_outer_8_planes": slab, "axis_with_surface": best, "pairs": []}

    def restore():
        vol.set_voxels(q, w)
        vol.set_colour_words(c)

    for name, s in pairs:
        back = tuple(-x for x in s)
        for store in (cstore, pstore):                              # the second buffers, the staging buffers, the bricks
            vol.shift(s, store); vol.shift(back, store)
            restore()
        ms_c, ms_p, lib_c, lib_p, rc_out, rc_back, rp_out = [], [], [], [], None, None, None
        for k in range(calls):                                      # alternately: a pair through the colour store, a pair through the plain one
            t = time.perf_counter(); rc_out = vol.shift(s, cstore); rc_back = vol.shift(back, cstore); ms_c.append(0.5e3 * (time.perf_counter() - t))
            lib_c.append(0.5 * (rc_out["ms_total"] + rc_back["ms_total"]))
            if k == 0:
                same = bool((vol.colour_words() == c)[seen].all())  # the seen voxels' colours came back
                restore()
            t = time.perf_counter(); rp_out = vol.shift(s, pstore); rp_back = vol.shift(back, pstore); ms_p.append(0.5e3 * (time.perf_counter() - t))
            lib_p.append(0.5 * (rp_out["ms_total"] + rp_back["ms_total"]))
            restore()
        vol.shift(s, cstore)
        bytes_c = cstore.stats()["bytes"]
        vol.shift(back, cstore)
        vol.shift(s, pstore)
        bytes_p = pstore.stats()["bytes"]
        vol.shift(back, pstore)
        restore()
        out["pairs"].append({"axis": name, "shift": list(s), "colour_store_shift_ms_median": float(np.median(ms_c)),
                             "plain_store_shift_ms_median": float(np.median(ms_p)),
                             "colour_over_plain": float(np.median(ms_c) / np.median(ms_p)),
                             "colour_store_shift_ms_library_median": float(np.median(lib_c)),
                             "plain_store_shift_ms_library_median": float(np.median(lib_p)),
                             "stored_out_back": [rc_out["stored"], rc_back["stored"]], "reloaded_out_back": [rc_out["reloaded"], rc_back["reloaded"]],
                             "launches_out_back": [rc_out["launches"], rc_back["launches"]],
                             "plain_store_launches_out_back": [rp_out["launches"], rp_back["launches"]],
                             "record_bytes_over_the_link_out": [12 * rc_out["stored"], 8 * rp_out["stored"]],
                             "colour_store_bytes": bytes_c, "plain_store_bytes": bytes_p,
                             "seen_colours_restored_bit_for_bit": same})
    # the colour of the whole map's mesh vertices next to the window's
    moved = vol.shift((64, 0, 0), cstore)
    wx, _, wt, wres = cstore.mesh(vol, normals=False)
    vx, _, vt, vres = vol.mesh(normals=False)
    cstore.colours(wx, vol); vol.colours(vx)
    ms_w, ms_v, wvalid, vvalid = [], [], None, None
    for _ in range(calls):
        t = time.perf_counter(); _, wvalid = cstore.colours(wx, vol); ms_w.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); _, vvalid = vol.colours(vx); ms_v.append(1e3 * (time.perf_counter() - t))
    t = time.perf_counter(); cstore.mesh_colour(vol); ms_mesh_colour = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter(); cstore.mesh(vol); ms_mesh = 1e3 * (time.perf_counter() - t)
    inside = vol.colours(wx)[1]
    st = cstore.stats()
    out["colours"] = {"stored_by_the_shift": moved["stored"], "store": st,
                      "world_colours_ms_median": float(np.median(ms_w)), "volume_colours_ms_median": float(np.median(ms_v)),
                      "world_vertices": len(wx), "window_vertices": len(vx),
                      "world_colours_ns_per_point": float(1e6 * np.median(ms_w) / max(len(wx), 1)),
                      "volume_colours_ns_per_point": float(1e6 * np.median(ms_v) / max(len(vx), 1)),
                      "world_over_volume_per_point": float((np.median(ms_w) / max(len(wx), 1)) / (np.median(ms_v) / max(len(vx), 1))),
                      "world_vertices_with_colour": int(wvalid.sum()), "window_vertices_with_colour": int(vvalid.sum()),
                      "world_vertices_coloured_only_through_the_store": int((wvalid & ~inside).sum()),
                      "bricks": wres["bricks"], "window_bricks": wres["window_bricks"], "store_bricks": st["bricks"],
                      "colour_brick_bytes_over_the_link": 2048 * st["bricks"], "point_bytes_over_the_link": 12 * len(wx),
                      "world_mesh_with_colour_ms_once": ms_mesh_colour, "world_mesh_ms_once": ms_mesh}
    for v in rendered:
        v.close()
    cstore.close()
    pstore.close()
    vol.close()
    return out


def pyramid(calls=20):
    """Image pyramids (oslam_pyramid_create, oslam_pyramid_egomotion) on frames 0 and 1 of the camera configuration's
    640x480 stream: the median of `calls` calls of Pyramid(view), of egomotion_pyramid and, in the same run, of egomotion
    on the same pair (the yardstick).  Host clock around calls that end in a host wait; every shape is warmed up first."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import refine_ref
    world = E.make_world(synth, 0)
    traj = E.trajectory(synth, 0, frames=2)
    cam = E.CAM
    views = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                      z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in traj]
    pyrs = [ppf.Pyramid(v) for v in views]
    ppf.egomotion_pyramid(pyrs[0], pyrs[1])
    ppf.egomotion(views[0], views[1])
    ppf.Pyramid(views[0]).close()
    make, ego_p, ego_p_lib, ego_v, ego_v_lib = [], [], [], [], []
    for _ in range(calls):                                          # the three alternate, so that drift hits them alike
        t = time.perf_counter(); q = ppf.Pyramid(views[0]); make.append(1e3 * (time.perf_counter() - t)); q.close()
        t = time.perf_counter(); Tp, rp = ppf.egomotion_pyramid(pyrs[0], pyrs[1]); ego_p.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); Tv, rv = ppf.egomotion(views[0], views[1]); ego_v.append(1e3 * (time.perf_counter() - t))
        ego_p_lib.append(rp["ms_total"])
        ego_v_lib.append(rv["ms_total"])
    G = E.truth(traj[0], traj[1])
    out = {"config": "pyramid (oslam_pyramid_create, oslam_pyramid_egomotion): 640x480, 3 levels, the camera stream's first pair",
           "calls": calls, "pyramid_create_ms_median": float(np.median(make)),
           "egomotion_pyramid_ms_median": float(np.median(ego_p)), "egomotion_pyramid_ms_library_median": float(np.median(ego_p_lib)),
           "egomotion_ms_median": float(np.median(ego_v)), "egomotion_ms_library_median": float(np.median(ego_v_lib)),
           "egomotion_pyramid": {"launches": rp["launches"], "iterations": rp["iterations"], "overlap": round(rp["overlap"], 3),
                                 "rot_deg_trans_m": [round(x, 5) for x in refine_ref.pose_error(Tp, G)]},
           "egomotion": {"launches": rv["launches"], "iterations": rv["iterations"], "overlap": round(rv["overlap"], 3),
                         "rot_deg_trans_m": [round(x, 5) for x in refine_ref.pose_error(Tv, G)]}}
    for q in pyrs:
        q.close()
    for v in views:
        v.close()
    return out


def bilateral(calls=20):
    """The bilateral depth filter (oslam_view_bilateral) on frames 0 and 1 of the camera configuration's 640x480 stream:
    the median of `calls` calls of bilateral_view at the default parameters and at radius 8, of Pyramid(view) (the
    yardstick: another one-kernel call over the same image) and of egomotion on the raw and on the filtered pair, all in
    the same run.  Host clock around calls that end in a host wait; every shape is warmed up first."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import refine_ref
    world = E.make_world(synth, 0)
    traj = E.trajectory(synth, 0, frames=2)
    cam = E.CAM
    views = [ppf.View(E.render(synth, world, T), cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_min=cam["z_min"],
                      z_max=cam["z_max"], max_jump=E.MAX_JUMP) for T in traj]
    filt = [ppf.bilateral_view(v)[0] for v in views]
    ppf.bilateral_view(views[0], radius=8)[0].close()
    ppf.Pyramid(views[0]).close()
    ppf.egomotion(views[0], views[1])
    ppf.egomotion(filt[0], filt[1])
    t6, t6_lib, t8, make, ego_r, ego_f = [], [], [], [], [], []
    for _ in range(calls):                                          # the five alternate, so that drift hits them alike
        t = time.perf_counter(); f, r6 = ppf.bilateral_view(views[0]); t6.append(1e3 * (time.perf_counter() - t)); f.close()
        t6_lib.append(r6["ms_total"])
        t = time.perf_counter(); f, r8 = ppf.bilateral_view(views[0], radius=8); t8.append(1e3 * (time.perf_counter() - t)); f.close()
        t = time.perf_counter(); q = ppf.Pyramid(views[0]); make.append(1e3 * (time.perf_counter() - t)); q.close()
        t = time.perf_counter(); Tr, rr = ppf.egomotion(views[0], views[1]); ego_r.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); Tf, rf = ppf.egomotion(filt[0], filt[1]); ego_f.append(1e3 * (time.perf_counter() - t))
    G = E.truth(traj[0], traj[1])
    out = {"config": "bilateral (oslam_view_bilateral): 640x480, the camera stream's first pair", "calls": calls,
           "library": os.path.basename(ppf.LIB_PATH),
           "bilateral_r6_ms_median": float(np.median(t6)), "bilateral_r6_ms_library_median": float(np.median(t6_lib)),
           "bilateral_r8_ms_median": float(np.median(t8)), "pyramid_create_ms_median": float(np.median(make)),
           "egomotion_raw_ms_median": float(np.median(ego_r)), "egomotion_filtered_ms_median": float(np.median(ego_f)),
           "bilateral_r6": {"valid": r6["valid"], "taps": r6["taps"], "launches": r6["launches"]},
           "bilateral_r8": {"valid": r8["valid"], "taps": r8["taps"], "launches": r8["launches"]},
           "egomotion_raw": {"iterations": rr["iterations"], "overlap": round(rr["overlap"], 3),
                             "rot_deg_trans_m": [round(x, 5) for x in refine_ref.pose_error(Tr, G)]},
           "egomotion_filtered": {"iterations": rf["iterations"], "overlap": round(rf["overlap"], 3),
                                  "rot_deg_trans_m": [round(x, 5) for x in refine_ref.pose_error(Tf, G)]}}
    for v in filt + views:
        v.close()
    return out


def _spacing(p, sample=500):
    """median distance to the nearest other point, from a seeded sample"""
    q = p.astype(np.float64)
    idx = np.random.default_rng(1).choice(len(q), size=min(sample, len(q)), replace=False)
    best = np.full(len(idx), np.inf)
    for b in range(0, len(q), 1 << 14):
        d2 = ((q[idx, None, :] - q[None, b:b + (1 << 14), :]) ** 2).sum(axis=2)
        d2[d2 == 0.0] = np.inf
        best = np.minimum(best, d2.min(axis=1))
    return float(np.median(np.sqrt(best)))


def _visited(p, edge):
    """the points in the 27 cells around every point's cell, summed: what the kernel's walk loads"""
    q = p.astype(np.float64)
    cell = np.floor((q - q.min(axis=0)) / edge).astype(np.int64) + 1
    dim = cell.max(axis=0) + 2
    key = np.sort((cell[:, 2] * dim[1] + cell[:, 1]) * dim[0] + cell[:, 0])
    total = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            k0 = key + (dz * dim[1] + dy) * dim[0] - 1
            total += int((np.searchsorted(key, k0 + 2, "right") - np.searchsorted(key, k0, "left")).sum())
    return total


def normals(calls=20, warm=5):
    mp, _ = synth.make_model(0, 5000)
    d = synth.d_dist_for(mp, 0.05)
    clouds = {"bench_scene_100k": synth.make_scene([0], 100000, 2002, instance_points=5000, noise_sigma=0.1 * d)[0],
              "slice_scene_500k": synth.make_scene([0, 1], 500000, 2004, instance_points=5000, noise_sigma=0.1 * d)[0]}
    out = {"config": "oslam_cloud_normals, points only, viewpoint at the origin; median of %d calls after %d" % (calls, warm),
           "sweeps": ppf.NORMALS_SWEEPS, "clouds": {}}
    for name, p in clouds.items():
        sp = _spacing(p)
        rows = []
        for k in (2.0, 4.0):
            radius = k * sp
            res, t = {}, {"ms_total": [], "ms_grid": [], "ms_kernel": []}
            for c in range(warm + calls):
                ppf.estimate_normals(p, radius, result=res)
                if c >= warm:
                    for key in t:
                        t[key].append(res[key])
            med = {key: float(np.median(v)) for key, v in t.items()}
            accepted = int(ppf.normal_moments(p, radius)[:, 0].sum())
            visited = _visited(p, res["edge"])
            rows.append({"radius_spacings": k, "radius": radius, **med, "n_valid": res["n_valid"], "n_cells": res["n_cells"],
                         "edge": res["edge"], "neighbours_accepted": accepted, "neighbours_visited": visited,
                         "accepted_per_s": accepted / (med["ms_kernel"] * 1e-3), "visited_per_s": visited / (med["ms_kernel"] * 1e-3)})
        out["clouds"][name] = {"points": len(p), "median_spacing": sp, "radii": rows}
    return out


def findplanes(calls=20, warm=3):
    """The planes stage (oslam_view_planes, oslam_view_remove_planes) on frame 0 of the camera configuration's room at
    640x480: the median of `calls` calls of find_planes (host clock and the library's) and of remove_planes, the scene
    points before and after, and the recognition chain (align + refine + verify of the room's three objects, the
    verification against the original view) on the full scene next to plane finding + removal + the chain on the reduced
    scene, the two alternating in one process.  `findplanes only` runs the find_planes calls alone, for a kernel trace."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import planes_inputs as PI
    import refine_ref
    img, cam = PI.room_frame(synth, 0, "full")
    view = PI.view_of(ppf, dict(depth=img, cam=cam, max_jump=E.MAX_JUMP))
    for _ in range(warm):
        ppf.find_planes(view).close()
    t_find, t_lib, t_rm = [], [], []
    for _ in range(calls):
        t = time.perf_counter(); pl = ppf.find_planes(view); t_find.append(1e3 * (time.perf_counter() - t))
        t_lib.append(pl.result["ms_total"])
        if len(sys.argv) > 2 and sys.argv[2] == "only":
            pl.close()
            continue
        t = time.perf_counter(); rv = ppf.remove_planes(view, pl); t_rm.append(1e3 * (time.perf_counter() - t))
        last = (pl.planes, pl.result, rv.mask_result)
        rv.close()
        pl.close()
    out = {"config": "planes stage (oslam_view_planes): frame 0 of the room, 640x480", "calls": calls,
           "library": os.path.basename(ppf.LIB_PATH), "find_planes_ms_median": float(np.median(t_find)),
           "find_planes_ms_library_median": float(np.median(t_lib))}
    if not t_rm:
        return out
    planes, res, mres = last
    out.update({"remove_planes_ms_median": float(np.median(t_rm)),
                "planes": [{"support": p["support"], "pixels": p["pixels"], "rms_mm": round(1e3 * p["rms"], 3)} for p in planes],
                "result": {k: res[k] for k in ("n_planes", "valid_in", "labelled", "launches")},
                "mask": {k: mres[k] for k in ("valid_in", "object_pixels", "valid_out")}})
    models, d, truth = PI.room_models(ppf, synth)

    def full_chain():
        sc = ppf.Scene.from_view(view, None, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
        r = PI.chain(ppf, models, sc, view)
        n = sc.numPoints()
        sc.close()
        return r, n

    def reduced_chain():
        pl = ppf.find_planes(view)
        sc = ppf.Scene.from_view(view, pl, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
        r = PI.chain(ppf, models, sc, view)
        n = sc.numPoints()
        sc.close()
        pl.close()
        return r, n

    full_chain(); reduced_chain()
    t_full, t_red = [], []
    for _ in range(calls):                                          # the two alternate, so that drift hits them alike
        t = time.perf_counter(); ra, na = full_chain(); t_full.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); rb, nb = reduced_chain(); t_red.append(1e3 * (time.perf_counter() - t))
    n_before = len(ppf.view_to_cloud(view)[0])
    pl = ppf.find_planes(view)
    rv = ppf.remove_planes(view, pl)
    n_after = len(ppf.view_to_cloud(rv)[0])
    rv.close(); pl.close()

    def report(r):
        return [{"found": x["found"], "rot_deg_trans_m": [round(e, 5) for e in refine_ref.pose_error(x["T"], truth[k])]}
                for k, x in enumerate(r)]
    out.update({"points_with_normal_before": n_before, "points_with_normal_after": n_after,
                "scene_points_full": na, "scene_points_reduced": nb, "leaf": d, "ref_point_df": PI.E2E_DF,
                "chain_full_ms_median": float(np.median(t_full)), "chain_reduced_with_planes_ms_median": float(np.median(t_red)),
                "ratio_full_over_reduced": float(np.median(t_full) / np.median(t_red)),
                "full": report(ra), "reduced": report(rb)})
    for m in models:
        m.close()
    view.close()
    return out


def segments(calls=20, warm=3):
    """The segments stage (oslam_view_segments, oslam_view_select_segments) on frame 0 of the camera configuration's room
    at 640x480: the medians of `calls` calls of find_planes, find_segments(view, planes) and select_segments, the chain
    align + refine + verify of the room's three models on the reduced scene of the planes stage, and the same chain with
    each model against the scene of each of the three largest segments (nine small registrations), the two alternating
    in one process.  `segments only` runs the find_segments calls alone, for a kernel trace."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import camera_ref as E
    import planes_inputs as PI
    import refine_ref
    img, cam = PI.room_frame(synth, 0, "full")
    view = PI.view_of(ppf, dict(depth=img, cam=cam, max_jump=E.MAX_JUMP))
    pl = ppf.find_planes(view)
    for _ in range(warm):
        ppf.find_segments(view, pl).close()
    t_seg, t_lib = [], []
    for _ in range(calls):
        t = time.perf_counter(); sg = ppf.find_segments(view, pl); t_seg.append(1e3 * (time.perf_counter() - t))
        t_lib.append(sg.result["ms_total"])
        sg.close()
    out = {"config": "segments stage (oslam_view_segments): frame 0 of the room, 640x480", "calls": calls,
           "library": os.path.basename(ppf.LIB_PATH), "find_segments_ms_median": float(np.median(t_seg)),
           "find_segments_ms_library_median": float(np.median(t_lib))}
    if len(sys.argv) > 2 and sys.argv[2] == "only":
        pl.close(); view.close()
        return out
    pl.close()
    t_find, t_sel, t_all = [], [], []
    for _ in range(calls):
        t0 = time.perf_counter(); pl = ppf.find_planes(view); t_find.append(1e3 * (time.perf_counter() - t0))
        sg = ppf.find_segments(view, pl)
        t = time.perf_counter(); sv = ppf.select_segments(view, sg, "keep", 0); t_sel.append(1e3 * (time.perf_counter() - t))
        t_all.append(1e3 * (time.perf_counter() - t0))
        last = (sg.segments, sg.result, sv.mask_result)
        sv.close(); sg.close(); pl.close()
    segs, res, mres = last
    out.update({"find_planes_ms_median": float(np.median(t_find)), "select_segments_ms_median": float(np.median(t_sel)),
                "planes_segments_select_ms_median": float(np.median(t_all)),
                "segments": [{"pixels": s["pixels"], "box": list(s["box"]), "centroid": [round(c, 4) for c in s["centroid"]],
                              "sides": s["sides"]} for s in segs],
                "result": {k: res[k] for k in ("n_segments", "n_components", "n_candidates", "valid_in", "labelled", "launches")},
                "mask": {k: mres[k] for k in ("valid_in", "object_pixels", "valid_out")}})
    models, d, truth = PI.room_models(ppf, synth)

    def reduced_chain():
        pl = ppf.find_planes(view)
        sc = ppf.Scene.from_view(view, pl, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
        r = PI.chain(ppf, models, sc, view)
        n = sc.numPoints()
        sc.close(); pl.close()
        return r, n

    def segment_chain():
        pl = ppf.find_planes(view)
        sg = ppf.find_segments(view, pl)
        r, n = [], []
        for k in range(min(3, len(sg.segments))):
            sc = ppf.Scene.from_view(view, segments=sg, only=k, leaf=d, d_dist=d, ref_point_downsample_factor=PI.E2E_DF)
            r.append(PI.chain(ppf, models, sc, view))
            n.append(sc.numPoints())
            sc.close()
        sg.close(); pl.close()
        return r, n

    reduced_chain(); segment_chain()
    t_red, t_sg = [], []
    for _ in range(calls):                                          # the two alternate, so that drift hits them alike
        t = time.perf_counter(); ra, na = reduced_chain(); t_red.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); rb, nb = segment_chain(); t_sg.append(1e3 * (time.perf_counter() - t))

    def report(r):
        return [{"found": x["found"], "rot_deg_trans_m": [round(e, 5) for e in refine_ref.pose_error(x["T"], truth[k])]
                 if x["T"].any() else None} for k, x in enumerate(r)]
    out.update({"scene_points_reduced": na, "scene_points_segments": nb, "leaf": d, "ref_point_df": PI.E2E_DF,
                "chain_reduced_with_planes_ms_median": float(np.median(t_red)),
                "chain_nine_on_segments_with_planes_and_segments_ms_median": float(np.median(t_sg)),
                "reduced": report(ra), "segments_by_rank": [report(r) for r in rb]})
    for m in models:
        m.close()
    view.close()
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    print(json.dumps({"cfg2": cfg2, "cfg3": cfg3, "cfg3db": cfg3db, "cfg4": cfg4, "cfg5": cfg5, "planes": planes, "db50": db50,
                      "refine": refine, "verify": verify, "instances": instances, "arbitrate": arbitrate, "explain": explain, "track": track, "camera": camera,
                      "fusion": fusion, "colour": colour, "surface": surface, "mesh": mesh, "shift": shift, "reload": reload, "worldsurface": worldsurface, "worldraycast": worldraycast, "worldmesh": worldmesh, "worldcolour": worldcolour, "pyramid": pyramid, "bilateral": bilateral, "normals": normals, "findplanes": findplanes, "segments": segments}[which]()), flush=True)
