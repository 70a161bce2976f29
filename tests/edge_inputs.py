"""Deterministic inputs at the edges of the view kernels (k_view_z, k_verify, k_claim, k_arbitrate, k_view_normals,
k_track, k_track_corr): ragged images, points on and one pixel outside every border, model sizes around the wave and
block sizes, 255..1024 hypotheses, identical hypotheses and claims tables with exact ties.

Every builder returns its inputs together with the restatement's answer (view_ref, arbitrate_ref, track_ref), so that
tests/test_edge_inputs.py can assert on a machine without a GPU that the inputs reach the branches they are meant for,
and tests/test_gpu_view_edges.py compares the device with the same answer.  numpy only; seeded (synth.SplitMix64)."""
import itertools

import numpy as np

import arbitrate_ref as A
import refine_ref
import track_ref as K
import view_ref as V

F = np.float32

SHAPES = [(1, 1), (1, 40), (3, 3), (7, 31), (8, 32), (9, 33), (61, 83), (481, 641)]      # (h, w)
MODEL_SIZES = [1, 2, 5, 6, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
MANY_H = [255, 256, 257, 1024]
PLANE_Z = 2.0                   # metres: the plane the border model lies on and the image shows
BORDER_D = 0.02                 # d_dist of the border model: tol = 0.02 m at depth_tol 1
MAX_JUMP = 0.05


def cam_of(h, w):
    """One camera per shape, the principal point off-centre."""
    f = 0.9 * max(h, w) + 3.0
    return dict(fx=f, fy=1.03 * f, cx=0.37 * w + 0.25, cy=0.58 * h - 0.125, depth_scale=0.001, z_min=0.5, z_max=12.0)


def images_of(h, w):
    """(uint16 image, float32 image in metres): a plane at PLANE_Z with a few millimetres of relief, a nearer block, a
    farther block and an invalid block where the image is large enough for them, and the values 0 and 65535; the float
    image sprinkled with NaN, -1, inf and 0 by flat index."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    img = (2000 + (u * 7 + v * 13) % 5).astype(np.uint16)
    if h >= 40 and w >= 40:
        img[h // 2 - 3: h // 2 + 4, w // 4 - 3: w // 4 + 4] = 1500          # nearer: what lies behind is OCCLUDED
        img[h // 2 - 3: h // 2 + 4, w // 2 - 3: w // 2 + 4] = 2600          # farther: what lies before is CONFLICT
        img[h // 4 - 3: h // 4 + 4, w // 2 - 3: w // 2 + 4] = 0             # not valid: UNKNOWN
    flat = img.reshape(-1)
    if flat.size >= 3:
        flat[0] = 0
        flat[-1] = 65535
    fimg = img.astype(np.float32) * F(0.001)
    ff = fimg.reshape(-1)
    idx = np.arange(ff.size)
    ff[idx % 11 == 3] = np.nan
    ff[idx % 13 == 5] = -1.0
    ff[idx % 17 == 7] = np.inf
    ff[idx % 19 == 9] = 0.0
    return img, fimg


def _samples(n):
    """pixel coordinates -1 .. n along one axis: all of them on a short axis, the ends and 40 between on a long one"""
    if n <= 64:
        return list(range(-1, n + 1))
    return sorted(set([-1, 0, 1, n - 2, n - 1, n] + [int(x) for x in np.linspace(2, n - 3, 40)]))


def border_model(h, w, synth, seed=7):
    """Model points back-projected from pixel centres of a grid one pixel larger than the image (the four border rows
    and columns, the four corners and the ring one pixel outside), on the plane z = PLANE_Z with normals towards the
    camera, then seeded random points with random normals around the plane for the other classes.  In camera
    coordinates: the identity pose puts every grid point on its pixel."""
    cam = cam_of(h, w)
    us, vs = _samples(w), _samples(h)
    edge_u, edge_v = {-1, 0, w - 1, w}, {-1, 0, h - 1, h}
    small = (w + 2) * (h + 2) <= 1500             # a small image: every pixel of the grid; a large one: every third sample
    iu, iv = (us, vs) if small else (us[::3], vs[::3])
    pix = set((a, b) for b in edge_v for a in us)
    pix |= set((a, b) for a in edge_u for b in vs)
    pix |= set((a, b) for a in iu for b in iv)
    pix = sorted(pix)
    pu = np.array([p[0] for p in pix], np.float64)
    pv = np.array([p[1] for p in pix], np.float64)
    grid = np.stack([(pu - cam["cx"]) * PLANE_Z / cam["fx"], (pv - cam["cy"]) * PLANE_Z / cam["fy"],
                     np.full(len(pix), PLANE_Z)], axis=1)
    rng = synth.SplitMix64(seed + 1000 * h + w)
    n_rand = 160
    r = rng.uniform(3 * n_rand).reshape(-1, 3)
    ru, rv = r[:, 0] * (w + 4) - 2.5, r[:, 1] * (h + 4) - 2.5
    rz = PLANE_Z + (r[:, 2] - 0.5) * 0.2
    rand = np.stack([(ru - cam["cx"]) * rz / cam["fx"], (rv - cam["cy"]) * rz / cam["fy"], rz], axis=1)
    nr = rng.normal(3 * n_rand).reshape(-1, 3)
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    mp = np.ascontiguousarray(np.concatenate([grid, rand]), np.float32)
    mn = np.ascontiguousarray(np.concatenate([np.tile([[0.0, 0.0, -1.0]], (len(grid), 1)), nr]), np.float32)
    return mp, mn, len(grid)


def rigid(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4, dtype=np.float64)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T.astype(np.float32)


def border_poses(h, w):
    """identity; one pixel to the right and down; 0.3 m towards the camera and away from it; a tilt of 2 degrees about
    the point the optical axis meets the plane"""
    cam = cam_of(h, w)
    R = K.axis_rotation((0.3, -1.0, 0.4), 2.0)
    c = np.array([0.0, 0.0, PLANE_Z])
    return {"identity": rigid(), "shift": rigid(t=(PLANE_Z / cam["fx"], PLANE_Z / cam["fy"], 0.0)),
            "toward": rigid(t=(0.0, 0.0, -0.3)), "behind": rigid(t=(0.0, 0.0, 0.3)), "tilt": rigid(R, c - R @ c)}


def project(mp, mn, T, cam):
    """(fu, fv, pz, back) of every model point in the restatement's float32 sequence (view_ref.classify), before any
    range check: for the conditions on where the points of a builder land."""
    q, m = refine_ref.transform_f32(T, mp, mn)
    with np.errstate(all="ignore"):
        dot = (m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2]
        fu = np.floor(((q[:, 0] * F(cam["fx"])) / q[:, 2] + F(cam["cx"])) + F(0.5))
        fv = np.floor(((q[:, 1] * F(cam["fy"])) / q[:, 2] + F(cam["cy"])) + F(0.5))
    return fu, fv, q[:, 2], dot >= F(0)


def ref_classes(mp, mn, T, img, cam, d, window=1, depth_tol=1.0):
    z = V.view_z(img, cam["depth_scale"], cam["z_min"], cam["z_max"])
    with np.errstate(all="ignore"):
        return V.classify(mp, mn, T, z, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["z_min"], cam["z_max"],
                          V.tolerance(depth_tol, d), window)


def shape_case(h, w, synth):
    """Everything the per-shape comparisons need: both images with their cameras, the border model, its poses."""
    cam = cam_of(h, w)
    img, fimg = images_of(h, w)
    mp, mn, n_grid = border_model(h, w, synth)
    return dict(h=h, w=w, cam=cam, fcam=dict(cam, depth_scale=1.0), img=img, fimg=fimg, mp=mp, mn=mn, n_grid=n_grid,
                d=BORDER_D, poses=border_poses(h, w))


# ---------------------------------------------------------------- model sizes on the smooth stream
RAGGED = dict(width=333, height=251, fx=270.0, fy=274.0, cx=160.3, cy=131.7)


def ragged_cam():
    return dict(fx=RAGGED["fx"], fy=RAGGED["fy"], cx=RAGGED["cx"], cy=RAGGED["cy"], depth_scale=0.001, z_min=0.5, z_max=12.0)


def size_case(synth, frame=2, dense_points=200000):
    """The MODEL_SIZES prefixes of one synth.make_model cloud on the smooth stream of tests/track_ref.py: frame `frame`
    rendered at 640x480 (the stream's camera) and at 333x251 (a ragged one), tracked from the pose of frame - 1."""
    mp, mn = synth.make_model(0, max(MODEL_SIZES))
    d = synth.d_dist_for(mp, 0.05)
    dense, _ = synth.make_model(0, dense_points)
    poses = K.smooth_poses(synth, d, frames=frame + 1)
    T = np.asarray(poses[frame], np.float64)
    pts = dense @ T[:3, :3].T + T[:3, 3]
    full = synth.render_depth(pts, background_z=K.STREAM_WALL, splat=1)
    rag = synth.render_depth(pts, background_z=K.STREAM_WALL, splat=1, **RAGGED)
    return dict(mp=mp, mn=mn, d=d, truth=poses[frame], previous=poses[frame - 1],
                frames={"640x480": (full, dict(K.STREAM_CAM)), "333x251": (rag, ragged_cam())})


# ---------------------------------------------------------------- many hypotheses
MANY_F = 47.0
MANY_VIEWS = {"96x64/16": (96, 64, 16), "160x32/32": (160, 32, 32), "192x32/32": (192, 32, 32)}     # w, h, tile
MANY_MODELS = (0, 36, 2)        # model 0, its near twin, another shape
MANY_PARAMS = dict(min_tiles=1)  # at tile 32 an object of 30 pixels claims one or two tiles


def many_cam(w, h):
    return dict(fx=MANY_F, fy=MANY_F, cx=0.47 * w + 0.3, cy=0.52 * h - 0.2, depth_scale=0.001, z_min=0.5, z_max=12.0)


def many_scene(synth, key, dense_points=120000):
    """Two objects before a wall in a small image: model 0 on the left (pose TA), model 2 on the right (pose TB)."""
    w, h, tile = MANY_VIEWS[key]
    cam = many_cam(w, h)
    clouds = [synth.make_model(k, 300) for k in MANY_MODELS]
    d = synth.d_dist_for(clouds[0][0], 0.05)
    rng = synth.SplitMix64(4242)
    TA = rigid(synth.random_rotation(rng), (-4.0, 0.1, 5.5))
    TB = rigid(synth.random_rotation(rng), (4.0, -0.1, 5.6))
    pts = []
    for k, T in ((0, TA), (2, TB)):
        dense, _ = synth.make_model(k, dense_points)
        pts.append(dense @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64))
    img = synth.render_depth(np.concatenate(pts), width=w, height=h, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"],
                             background_z=K.STREAM_WALL, splat=1)
    return dict(cam=cam, img=img, tile=tile, clouds=[(p, n, d) for p, n in clouds], d=d, TA=TA, TB=TB)


def many_hypotheses(sc, H):
    """-> (member index [H] into sc['clouds'], T [H,4,4]).  By index mod 4:
      1  the true pose of the left object;
      2  a small deterministic nudge of a true pose with one of the three models (the right object's model pushed back
         by 0.6 d_dist below index 256);
      3  an exact duplicate of the entry two before;
      0  the right object's model: pushed back by half a d_dist below index 300, close to its true pose from there on
         and at it in every 16th entry, so that the right object's survivor has an index above 256.
    All-zero (skipped) poses at 0, 255, 256, H - 1 and wherever index mod 17 is 5."""
    d = sc["d"]
    mem = np.zeros(H, np.int64)
    T = np.zeros((H, 4, 4), np.float32)
    for i in range(H):
        if i in (0, 255, 256, H - 1) or i % 17 == 5:
            continue
        k = i % 4
        if k == 1:
            mem[i], T[i] = 0, sc["TA"]
        elif k == 2:
            mem[i] = (i // 4) % 3
            base = sc["TB"] if mem[i] == 2 else sc["TA"]
            T[i] = base
            T[i, 2, 3] += F(0.05 * d * ((i // 4) % 7 - 3))
            T[i, 0, 3] += F(0.03 * d * ((i // 12) % 5 - 2))
            if mem[i] == 2 and i < 256:
                T[i, 2, 3] += F(0.6 * d)
        elif k == 3:
            mem[i], T[i] = mem[i - 2], T[i - 2]
        else:
            mem[i], T[i] = 2, sc["TB"]
            if i < 300:
                T[i, 0, 3] += F(0.1 * d * (1 + (i // 4) % 3))
                T[i, 2, 3] += F(0.5 * d)
            elif i % 16 != 12:
                T[i, 2, 3] += F(0.02 * d * ((i // 4) % 5 - 2))
    return mem, T


def many_case(synth, key, H):
    sc = many_scene(synth, key)
    mem, T = many_hypotheses(sc, H)
    clouds = [sc["clouds"][m] for m in mem]
    want, kept = A.arbitrate(clouds, T, sc["img"], sc["cam"], tile=sc["tile"], **MANY_PARAMS)
    return dict(sc, mem=mem, T=T, want=want, kept=kept)


def identical_case(synth, H, key="96x64/16"):
    """H copies of model 0 at the left object's true pose."""
    sc = many_scene(synth, key)
    T = np.repeat(sc["TA"][None], H, axis=0)
    order = []
    cnt, sm, tile, tols = A.claims([sc["clouds"][0]] * H, T, sc["img"], sc["cam"], tile=sc["tile"])
    res, rounds = A.eliminate(cnt, sm, [False] * H, tols, order=order, **MANY_PARAMS)
    for r in res:
        r["tile"], r["rounds"] = tile, rounds
    return dict(sc, T=T, want=res, rounds=rounds, order=order)


def identical_answer(H):
    """(kept, suppressed_by) known without running anything"""
    return [True] + [False] * (H - 1), [-1] + [0] * (H - 1)


# ---------------------------------------------------------------- claims tables for the table tap
def tie_tables():
    """Named (cnt, sm, skipped, min_tiles, min_owned_share) with exact ties; Python integers are the truth
    (arbitrate_ref.eliminate)."""
    out = {}
    words = [(1, 2), (2, 4), (3, 6)]                     # the same mean residual 2 in three different words
    for k, perm in enumerate(itertools.permutations(range(3))):
        cnt = np.array([[words[p][0]] * 4 for p in perm], np.int64)
        sm = np.array([[words[p][1]] * 4 for p in perm], np.int64)
        out["mean tie %d" % k] = (cnt, sm, None, 1, 0.52)
    big_c, big_s = (1 << 24) - 1, ((1 << 24) - 1) * 65535
    # products of 2^24 - 1 and (2^24 - 1) * 65535 reach 2^64: one unit less in a sum must still win
    cnt = np.full((4, 3), big_c, np.int64)
    sm = np.full((4, 3), big_s, np.int64)
    sm[2, 0] -= 1
    sm[3, 1] -= 1
    cnt[1, 2] -= 1                                       # the same sum over fewer points: a larger mean
    out["large counts"] = (cnt, sm, None, 1, 0.52)
    for gap in (256, 512):
        # share ties across the thread stride: h and h + gap claim the same two tiles and own one each (share 0.5 <
        # 0.52); the larger index leaves, then the smaller owns both.  Which of the two is kept shows the rule.
        H = gap + 40
        cnt = np.zeros((H, 8), np.int64)
        sm = np.zeros((H, 8), np.int64)
        for h, t in ((3, 0), (17, 2), (39, 4)):
            cnt[h, t:t + 2], cnt[h + gap, t:t + 2] = 1, 1
            sm[h, t:t + 2], sm[h + gap, t:t + 2] = (1, 2), (2, 1)
        out["share tie +%d" % gap] = (cnt, sm, None, 1, 0.52)
        # beat ties: h and h + gap each own two of the loser's four tiles; the lower one suppresses
        cnt = np.zeros((H, 8), np.int64)
        sm = np.zeros((H, 8), np.int64)
        cnt[H - 1, :4], sm[H - 1, :4] = 3, 30            # the loser: the worst everywhere it claims
        cnt[5, 0:2], sm[5, 0:2] = 3, 3
        cnt[5 + gap, 2:4], sm[5 + gap, 2:4] = 3, 3
        cnt[5, 4:6], sm[5, 4:6] = 1, 1                   # tiles of their own, so that both stay
        cnt[5 + gap, 6:8], sm[5 + gap, 6:8] = 1, 1
        out["beat tie +%d" % gap] = (cnt, sm, None, 1, 0.52)
    rng = np.random.default_rng(5)
    cnt = rng.integers(0, 4, (9, 1))
    out["one tile"] = (cnt, cnt * 2, None, 1, 0.52)
    out["one hypothesis"] = (np.array([[1, 0, 2]]), np.array([[3, 0, 1]]), None, 1, 0.52)
    cnt = rng.integers(0, 4, (12, 6))
    sm = cnt * rng.integers(0, 3, (12, 6))
    sk = np.ones(12, bool)
    sk[7] = False
    cnt[7, 0] = 1
    out["all skipped but one"] = (cnt, sm, sk, 1, 0.52)
    out["min_tiles above every claim"] = (cnt, sm, None, 7, 0.52)
    out["min_owned_share 0"] = (cnt, sm, None, 1, 0.0)
    out["min_owned_share 1"] = (cnt, sm, None, 1, 1.0)
    for name, (H, nt) in {"40960 bytes": (1024, 5), "40968 bytes": (569, 9), "40960 bytes 512x10": (512, 10)}.items():
        assert H * nt * 8 == (40968 if name == "40968 bytes" else 40960)
        cnt = np.zeros((H, nt), np.int64)
        rows = rng.choice(H, 48, replace=False)
        cnt[rows] = rng.integers(0, 4, (48, nt))
        sm = cnt * rng.integers(0, 3, (H, nt))
        out[name] = (cnt, sm, None, 1, 0.52)
    return out


def random_tables(n=200, n_large=5, seed=11):
    """The seeded sweep: H <= 40, n_tiles <= 12, cnt in 0..3, sum = cnt * {0, 1, 2}; then n_large tables with H in
    257..600 and n_tiles <= 8 (mostly empty rows, so that the restatement stays cheap)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n + n_large):
        if k < n:
            H, nt = int(rng.integers(1, 41)), int(rng.integers(1, 13))
            cnt = rng.integers(0, 4, (H, nt))
        else:
            H, nt = int(rng.integers(257, 601)), int(rng.integers(1, 9))
            cnt = np.zeros((H, nt), np.int64)
            rows = rng.choice(H, 40, replace=False)
            cnt[rows] = rng.integers(0, 4, (40, nt))
        sm = cnt * rng.integers(0, 3, (H, nt))
        sk = rng.random(H) < 0.1
        out.append((cnt.astype(np.int64), sm.astype(np.int64), sk, int(rng.integers(0, 4)), float(rng.choice([0.0, 0.3, 0.52, 0.75, 1.0]))))
    return out


def eliminate_table(cnt, sm, skipped=None, min_tiles=4, min_owned_share=0.52):
    """arbitrate_ref.eliminate with tol 1 for every hypothesis: what oslam_arbitrate_table must return"""
    H = cnt.shape[0]
    sk = [False] * H if skipped is None else [bool(x) for x in skipped]
    if all(sk):
        return [dict(claimed=0, owned=0, share=F(0), mean_residual=F(0), kept=False, suppressed_by=-1) for _ in range(H)], 0
    return A.eliminate(np.asarray(cnt, np.int64), np.asarray(sm, np.int64), sk, np.ones(H, np.float32), min_tiles, min_owned_share)


# ---------------------------------------------------------------- front end
def voxel_cases(synth):
    """name -> (points, normals, leaf).  The last point of the clouds of 262145 and ~600000 points lies outside the box
    of all the others, so a bounding box that misses the tail of the cloud puts it into a wrong voxel."""
    out = {}
    rng = synth.SplitMix64(31)
    n_big = 600011
    p = (rng.uniform(3 * n_big).reshape(-1, 3) * 4.0 - 2.0).astype(np.float32)
    nr = rng.normal(3 * n_big).reshape(-1, 3)
    nr = (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(np.float32)
    for n in (262143, 262144, 262145, n_big):
        q = p[:n].copy()
        q[n - 1] = [-2.75, 3.1, -2.6]
        q[n - 2] = [2.9, -2.8, 3.3]
        out["n %d" % n] = (q, nr[:n], 0.11)
    out["shifted"] = (p[:50000] + np.float32([-1000.0, 500.0, 2000.0]), nr[:50000], 0.11)
    k = (rng.uniform(3 * 20000).reshape(-1, 3) * 33).astype(np.int64) - 16
    out["on voxel faces"] = ((k * 0.25).astype(np.float32), nr[:20000], 0.25)
    out["one voxel"] = (np.abs(p[:30000]), nr[:30000], 1000.0)
    out["one point"] = (p[:1], nr[:1], 0.11)
    out["none finite"] = (np.full((500, 3), np.nan, np.float32), nr[:500], 0.11)
    return out
