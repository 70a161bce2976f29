"""The inputs of the whole map's ray cast tests (tests/test_world_raycast_host.py on the CPU, tests/test_gpu_world_raycast.py
on the device): maps, poses and cameras, built once per process and left unchanged.

Analytic maps.  A window of n voxels at an offset that is no multiple of 8 and negative on one axis lies in a region of
3 x 2 x 2 windows.  Over the region a TSDF is laid analytically, in voxel units: a sphere that straddles the window's +x
face, and behind the window a slightly tilted plane with a round hole, d = min(d_sphere, d_plane), F = d / 4 clipped to
[-1, 1] (mu = 4 voxels), q = rint(F * 32767), a voxel seen iff |d| <= 4 and a hash of its coordinates does not knock it
out (1 in 50: trilinear reads that fail, samples that forget), weights 1..3 from the same hash.  The window's part goes
into the window, the rest into the store, brick by brick only where something is seen: free space has no bricks.  One store
entry is planted inside the window's box, at the voxel of a hit, with a word that would change that hit.

The random map is test_world_surface_host.usual(40 x 72 x 24) after the first two shifts of its chain: random 32-bit words
in the window and in a store on every side of it.

Poses are T_vol_cam float32 4x4, the camera looking along its +z, x right, y down.
"""
import numpy as np

import reload_ref as W
import shift_ref as H
import test_world_surface_host as TW
import volume_ref as V

F = np.float32
VOXEL, ORIGIN0, MU = 0.05, (-0.35, 0.15, 0.25), 0.2
SHAPES = {"16^3": ((16, 16, 16), (-13, 5, 3)), "40x72x24": ((40, 72, 24), (-21, 3, 5))}
CAM37 = dict(width=37, height=21, fx=30.0, fy=30.0, cx=18.0, cy=10.0)        # a ragged tile edge; integer cx, cy
CAM64 = dict(width=64, height=16, fx=50.0, fy=50.0, cx=32.0, cy=8.0)         # exact tiles
BASE = dict(z_min=0.1, z_max=10.0, depth_scale=0.001, max_jump=0.05)


def cam_of(c):
    return dict(BASE, **{k: c[k] for k in ("fx", "fy", "cx", "cy")})


def _hash(g):
    g = g.astype(np.int64)
    return ((g[..., 0] * 73856093) ^ (g[..., 1] * 19349663) ^ (g[..., 2] * 83492791)) & 0x7fffffff


def rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def pose(eye_g, R=None):
    """the camera at the global voxel coordinate eye_g (floats), rotated by R"""
    T = np.eye(4)
    T[:3, :3] = np.eye(3) if R is None else R
    T[:3, 3] = np.array(ORIGIN0, np.float64) + np.array(eye_g, np.float64) * VOXEL
    return T.astype(np.float32)


def analytic(name):
    """-> dict(vol, store, sp, region=(lo, hi), geometry...) of the analytic map of SHAPES[name], without the planted entry"""
    n, off = SHAPES[name]
    n, off = np.array(n), np.array(off)
    lo, hi = off - n * np.array([1, 0, 0]), off + 2 * n
    k, j, i = np.indices((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]))
    g = np.stack([i + lo[0], j + lo[1], k + lo[2]], axis=-1)
    c = g + 0.5
    centre = off + n * np.array([1.0, 0.6, 0.9])
    radius = 0.38 * n.min()
    d_s = np.sqrt(((c - centre) ** 2).sum(axis=-1)) - radius
    nrm = np.array([0.08, 0.05, 1.0])
    nrm /= np.sqrt((nrm ** 2).sum())
    p0 = off + n * np.array([0.5, 0.5, 1.5])
    d_p = ((p0 - c) * nrm).sum(axis=-1)
    hole = p0 + np.array([0.8 * n[0], 0.3 * n[1], 0.0])
    in_hole = np.sqrt(((c - hole)[..., :2] ** 2).sum(axis=-1)) < 0.35 * n.min()
    d_p = np.where(in_hole, np.inf, d_p)
    d = np.minimum(d_s, d_p)
    h = _hash(g)
    seen = (np.abs(d) <= 4.0) & (h % 50 != 0)
    q = np.rint(np.clip(np.where(seen, d, 0) / 4.0, -1, 1) * 32767).astype(np.int16)
    w = np.where(seen, 1 + (h >> 8) % 3, 0).astype(np.uint16)
    words = q.view(np.uint16).astype(np.uint32) | (w.astype(np.uint32) << np.uint32(16))
    vol = H.shifted(V.Volume(int(n[0]), int(n[1]), int(n[2]), VOXEL, list(ORIGIN0), mu=MU), tuple(int(x) for x in off))
    inside = ((g >= off) & (g < off + n)).all(axis=-1)
    s = tuple(slice(int(off[a] - lo[a]), int(off[a] - lo[a] + n[a])) for a in (2, 1, 0))
    W.set_words(vol, words[s])
    pick = seen & ~inside
    store = dict(zip(map(tuple, g[pick].tolist()), words[pick].tolist()))
    return dict(name=name, vol=vol, store=store, sp=(vol.voxel, H.state(vol)[0]), n=n, off=off, lo=lo, hi=hi, centre=centre,
                radius=radius, p0=p0, hole=hole)


def cases(m):
    """[(name, T_vol_cam, camera spec, anchor or None, box or None)] for an analytic map"""
    n, off = m["n"].astype(np.float64), m["off"].astype(np.float64)
    cw = off + n / 2
    big = n.max()
    wbox = (tuple(int(x) for x in m["off"]), tuple(int(x) for x in m["off"] + m["n"]))
    return [
        # outside the map, looking in over the sphere and the plane behind it
        ("outside", pose(cw + np.array([0.3 * n[0], 0.1 * n[1], -0.5 * n[2] - 1.2 * big]), rot_y(8) @ rot_x(-4)), CAM37, None, None),
        # inside the window, looking out through its +x and +z faces into the store
        ("inside_out", pose(cw + np.array([0.0, 0.05 * n[1], -0.3 * n[2]]), rot_y(25)), CAM64, (-7, 11, 2), None),
        # identity rotation: column cx has D_x == 0 and row cy D_y == 0; the camera centre inside the slabs
        ("identity_inside", pose(cw + np.array([0.25, 0.25, -1.0 * n[2]])), CAM37, None, None),
        # the same against the window's box with the centre left of it: column cx misses on a zero direction
        ("identity_outside", pose(np.array([off[0] - 5.3, cw[1] + 0.25, off[2] - 0.8 * n[2]])), CAM64, None, wbox),
        # through the hole in the plane: rays that leave the box through its +z face
        ("plus_z", pose(np.array([m["hole"][0] - 0.2 * n[0], m["hole"][1], off[2] - 0.6 * n[2]]), rot_y(4) @ rot_x(2)), CAM37, None, None),
        # behind the plane, looking back: F < 0 comes first
        ("behind", pose(np.array([cw[0], cw[1], off[2] + 2.0 * n[2] + 0.8 * big]), rot_y(186)), CAM64, None, None),
    ]


def planted_entry(m, ts, T, spec):
    """(g, word): the voxel of the first hit of the z image ts whose point lies inside the window's box, and a word that
    is not the window's there: the store entry that must be ignored"""
    vol = m["vol"]
    M = np.asarray(T, np.float32).astype(np.float64)
    off, n = np.array(H.state(vol)[1]), np.array(vol.n)
    for v, u in np.argwhere(ts > 0):
        t = float(ts[v, u])
        p = M[:3, :3] @ np.array([(u - spec["cx"]) / spec["fx"] * t, (v - spec["cy"]) / spec["fy"] * t, t]) + M[:3, 3]
        g = np.floor((p - np.array(ORIGIN0, np.float64)) / VOXEL).astype(np.int64)
        if ((g >= off + 2) & (g < off + n - 2)).all():
            return tuple(int(x) for x in g), (3 << 16) | 20000
    raise AssertionError("no hit inside the window")


def with_planted(m):
    """the analytic map with its planted store entry: -> (store, g, word); found from the "inside_out" case"""
    name, T, spec, anchor, box = cases(m)[1]
    import world_raycast_ref as R
    ts, _, _ = R.raycast(m["store"], m["sp"], T, cam_of(spec), spec["width"], spec["height"], m["vol"], anchor, box)
    g, word = planted_entry(m, ts, T, spec)
    store = dict(m["store"])
    store[g] = word
    return store, g, word


def pin_box(store, vol):
    """(lo, hi): a box with every seen voxel of the map and a margin of at least 1, its sides multiples of 8 and at least
    16: what a dense device volume can be made for (pin (a))"""
    import world_surface_ref as WS
    lo, hi = WS.bounds(store, vol, margin=1)
    return lo, tuple(lo[a] + max(16, -(-(hi[a] - lo[a]) // 8) * 8) for a in range(3))


def dense_of(store, sp, vol, lo, hi, mu):
    """pin (a)'s dense volume_ref.Volume: the map's words over lo <= g < hi, at offset lo, with the map's mu"""
    import world_surface_ref as WS
    return WS.dense(store, sp, vol, lo, hi, lambda nx, ny, nz, voxel, origin: V.Volume(nx, ny, nz, voxel, list(origin), mu=float(mu)))


# the walk of pin (c): three frames of volume_ref.small_stream's world and trajectory fused at their true poses into a
# volume whose sides are multiples of 16, one shift through a store, the ray cast from the first pose with a small camera
WALK_VOL = dict(nx=64, ny=48, nz=64, voxel=0.1, origin=[-3.2, -2.4, 0.3], mu=0.4, max_weight=128)
WALK_SHIFT = (24, 0, 8)
WALK_CAM = dict(width=80, height=60, fx=65.625, fy=65.625, cx=39.5, cy=29.5)
WALK_FRAMES = 3


def walk_frames(synth, seed=0):
    """-> [(depth image uint16 at volume_ref.SMALL, T_vol_cam float32)] of the walk"""
    import camera_ref as E
    world, traj = E.make_world(synth, seed), E.trajectory(synth, seed)
    return [(E.render(synth, world, T, **V.SMALL), np.asarray(T, np.float32)) for T in traj[:WALK_FRAMES]]


def random_map():
    """the random words of test_world_surface_host.usual after the first two shifts of its chain (offset (-4, -4, 3))"""
    vol = TW.usual(TW.RAGGED, 31)
    sp = TW.params_of(vol)
    store, cur = {}, vol
    for s in TW.CHAIN[:2]:
        cur, _, _ = W.shift_world(cur, store, s)
    return dict(name="random", start=vol, vol=cur, store=store, sp=sp)


def random_cases(m):
    vol = m["vol"]
    off, n = np.array(H.state(vol)[1], np.float64), np.array(vol.n, np.float64)
    voxel, origin0 = float(vol.voxel), np.asarray(m["sp"][1], np.float64)

    def at(eye_g, R=None):
        T = np.eye(4)
        T[:3, :3] = np.eye(3) if R is None else R
        T[:3, 3] = origin0 + np.array(eye_g) * voxel
        return T.astype(np.float32)

    cw = off + n / 2
    return [("random_outside", at(cw + np.array([3.0, -2.0, -60.0]), rot_y(5) @ rot_x(3)), CAM37, None, None),
            ("random_inside", at(cw + np.array([0.3, 0.2, 0.1]), rot_y(-40)), CAM64, (5, -3, 1), None)]
