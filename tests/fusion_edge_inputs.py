"""Deterministic inputs at the edges of the camera motion kernels (k_ego_step, k_ego_corr) and of the fusion kernels
(k_tsdf_integrate, k_tsdf_raycast): lattices of one block, of fewer slots than strands, of exactly the slot limit and of a
last workgroup that walks fewer blocks than the others; volumes of the smallest legal size and with 8 live lanes in the
last x tile; cameras inside the volume, on a voxel centre and a hair off the plane of one; weights that saturate and that
cross 255/256; rays with a zero direction component, behind the surface, across an unseen gap and cut by z_min/z_max.

tests/test_fusion_edge_inputs.py asserts on the restatements alone (camera_ref, volume_ref and its trace) that the
inputs reach the paths they are named for; tests/test_gpu_fusion_edges.py compares the device with the same
restatements.  numpy only; the room is camera_ref's seeded world, everything else is analytic."""
import numpy as np

import camera_ref as C
import edge_inputs
import track_ref as K
import volume_ref as V

F = np.float32
THREADS, MAX_SLOTS, STRANDS = C.THREADS, C.MAX_SLOTS, C.STRANDS


# ---------------------------------------------------------------- the lattices of the camera motion stage
def lattice_of(w, h, stride):
    """(lw, n, n_blocks, chunk, n_slots) of a level over a w x h source: set_level of oslam_ego.c."""
    lw = (w + stride - 1) // stride
    n = lw * ((h + stride - 1) // stride)
    n_blocks = (n + THREADS - 1) // THREADS
    chunk = (n_blocks + MAX_SLOTS - 1) // MAX_SLOTS
    n_slots = (n_blocks + chunk - 1) // chunk
    return lw, n, n_blocks, chunk, n_slots


# name -> (w, h, stride of the one-level call, the schedule of the second call, the lattice the stride is meant to give)
EGO_CASES = {
    "1x1": (1, 1, 1, [(2, 2), (1, 3)], (1, 1, 1, 1, 1)),                     # fewer than 6 correspondences
    "16x16": (16, 16, 1, [(2, 2), (1, 3)], (16, 256, 1, 1, 1)),              # one full block, its own last arriver
    "17x16": (17, 16, 1, [(2, 2), (1, 3)], (17, 272, 2, 1, 2)),              # the second block has 16 live indices
    "83x61/4": (83, 61, 4, [(4, 2), (2, 2), (1, 3)], (21, 336, 2, 1, 2)),    # the stride divides neither side
    "48x37": (48, 37, 1, [(2, 2), (1, 3)], (48, 1776, 7, 1, 7)),             # 7, 8 and 9 slots against 8 strands
    "48x42": (48, 42, 1, [(2, 2), (1, 3)], (48, 2016, 8, 1, 8)),
    "48x43": (48, 43, 1, [(2, 2), (1, 3)], (48, 2064, 9, 1, 9)),
    "256x256": (256, 256, 1, [(4, 2), (2, 2), (1, 2)], (256, 65536, 256, 1, 256)),       # exactly the slot limit
    "257x256": (257, 256, 1, [(4, 2), (2, 2), (1, 2)], (257, 65792, 257, 2, 129)),       # the last slot walks one block
    "333x251/16": (333, 251, 16, [(16, 2), (4, 2), (1, 2)], (21, 336, 2, 1, 2)),         # the largest legal stride
    "333x251 skip": (333, 251, 3, [(3, 2), (16, 0), (1, 2)], (111, 9324, 37, 1, 37)),    # a level of 0 iterations between two
    # a wide camera (the floor and the side wall fill the image): well conditioned, so the pose is held to the bits of
    # the sums="f32" restatement on a ragged lattice too; 14 slots: strands of two slots and of one
    "203x151 wide/3": (203, 151, 3, [(3, 2), (1, 2)], (68, 3468, 14, 1, 14)),
}
WIDE_FX = {"203x151 wide/3": 80.0}               # fx of the cases that do not scale edge_inputs.RAGGED
BITS_HELD = ("203x151 wide/3",)                  # the cases whose cond lies below COND_STREAM_640
DIFFERENT_VIEWS = ("83x61/4", "333x251/16")      # the pair with two sizes and cameras: source 83x61, destination 333x251

# The largest cond that camera_ref.egomotion(sums="f32") reports (J^T J of the first step) over the nine consecutive pairs
# of the 640x480 seed-0 stream of tests/test_gpu_camera.py: 3788.79 at frame 1 (1861 .. 3789 over the nine), rounded up.
# tests/test_fusion_edge_inputs.py recomputes it.  Up to here the device's pose is held to the bits of the sums="f32"
# restatement; above it the two solve a system whose rounding the 29 sums no longer fix, and the difference is printed.
# Of the cases above only BITS_HELD lie below it (cond 60); the others lie between 6.1e3 and 1.4e8 (the different views
# 5.7e4 .. 2.4e5), so for them the gate is open and the pose is held to max(ROT_FLOOR, 8 x spread) only, while the integer
# fields, overlap and rmse are held bit for bit everywhere.
COND_STREAM_640 = 3789.0


def ego_size(w, h, fx=None):
    """The keywords of camera_ref.render for a w x h image: edge_inputs.RAGGED at its own size, else its focal length
    scaled with the width so that the room stays in view (or fx), the principal point off-centre."""
    if (w, h) == (edge_inputs.RAGGED["width"], edge_inputs.RAGGED["height"]):
        return dict(edge_inputs.RAGGED)
    s = w / float(edge_inputs.RAGGED["width"]) if fx is None else fx / edge_inputs.RAGGED["fx"]
    return dict(width=w, height=h, fx=270.0 * s, fy=274.0 * s, cx=0.4814 * w, cy=0.5247 * h)


def cam_of_size(size):
    return dict(fx=size["fx"], fy=size["fy"], cx=size["cx"], cy=size["cy"], depth_scale=0.001, z_min=0.5, z_max=12.0)


def ego_world(synth):
    """seed 0 of tests/test_camera_host.py: (world, the first two camera poses)"""
    return C.make_world(synth, 0), C.trajectory(synth, 0, frames=2)


def ego_case(synth, world, traj, name):
    """-> dict(images, cam, maps of frames 0 and 1 at the case's size, stride, schedule, lattice)"""
    w, h, stride, schedule, want = EGO_CASES[name]
    size = ego_size(w, h, WIDE_FX.get(name))
    cam = cam_of_size(size)
    imgs = [C.render(synth, world, T, **size) for T in traj[:2]]
    return dict(name=name, w=w, h=h, stride=stride, schedule=schedule, lattice=want, cam=cam, imgs=imgs,
                maps=[K.view_maps(im, cam, C.MAX_JUMP) for im in imgs])


def scheduled(levels):
    return sum(it for _, it in levels)


# ---------------------------------------------------------------- volumes
VOXEL, MU = 0.125, 0.25                       # binary fractions: voxel centres, depths and sdf == -mu are exact in float
VOLUME_SIZES = [(16, 16, 16), (136, 16, 16), (72, 24, 40)]
MAX_WEIGHTS = (1, 2, 300)
WEIGHT_STEPS = 301
WEIGHT_CHECKS = (1, 2, 255, 256, 257, 300, 301)
# the field's own limit, max_weight 65535, is left out: a weight grows by one per integration, so reaching it takes
# 65535 launches per case.
IMAGE_SHAPES = [(1, 1), (7, 31), (9, 33)]     # (h, w) of the integrated images
SURFACE_Z = 0.5                               # metres before the camera: on the lattice of the voxel centres' depths


def volume_spec(n, max_weight=2):
    """The volume of size n = (nx, ny, nz) centred on the volume frame's x and y axes, z from 0."""
    return dict(nx=n[0], ny=n[1], nz=n[2], voxel=VOXEL, origin=[-0.5 * n[0] * VOXEL, -0.5 * n[1] * VOXEL, 0.0], mu=MU,
                max_weight=max_weight)


def centre_of(spec, i, j, k):
    o = spec["origin"]
    return np.array([o[0] + (i + 0.5) * VOXEL, o[1] + (j + 0.5) * VOXEL, o[2] + (k + 0.5) * VOXEL])


def integration_poses(n):
    """name -> T_vol_cam (float32 4x4).  All look along +z of the volume but "tilted".
      centre      on the centre of voxel (nx/2, ny/2, nz/2): about half of the voxel centres lie behind the camera, a whole
                  z layer lies in its plane and one centre is the camera centre itself;
      near plane  the same, 2^-21 m (4.8e-7) further back: that layer is 4.8e-7 m in front of the camera plane;
      end         6 voxels from the far end of x, 2 from the near end of z: the frustum reaches the last x tile;
      tilted      the centre pose turned 7 degrees about a skew axis: nothing is exact."""
    spec = volume_spec(n)
    c = centre_of(spec, n[0] // 2, n[1] // 2, n[2] // 2)
    out = {"centre": edge_inputs.rigid(t=c), "near plane": edge_inputs.rigid(t=c - np.array([0.0, 0.0, 2.0 ** -21])),
           "end": edge_inputs.rigid(t=centre_of(spec, n[0] - 6, n[1] // 2, 2)),
           "tilted": edge_inputs.rigid(K.axis_rotation((0.5, 1.0, -0.3), 7.0), c)}
    return out


def integration_cam(h, w):
    """edge_inputs.cam_of at half the focal length (the image spans about 95 degrees): the frustum covers a part of the
    volume that is neither empty nor all of it"""
    f = 0.45 * max(h, w) + 1.5
    return dict(edge_inputs.cam_of(h, w), fx=f, fy=1.03 * f, depth_scale=1.0, z_min=0.1, z_max=10.0)


def integration_image(h, w, holes=False, shift=0.0):
    """float32 metres: the plane z = SURFACE_Z, every fifth pixel a few millimetres nearer or farther (so that most
    updates are inexact while the others keep sdf == -mu exact); holes: z = 0 at every fourth pixel; shift: added to
    the right half."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    k = (u * 7 + v * 13) % 5
    z = (SURFACE_Z + np.where(k == 1, 0.003 * ((u + v) % 7 - 3), 0.0)).astype(np.float32)
    z[:, w // 2:] += F(shift)
    if holes:
        z[(u * 3 + v * 5) % 4 == 1] = 0.0
    return z


def integration_cases():
    """[(name, n, T_vol_cam, image, cam)]: every volume, pose and image, and the 9x33 image with holes."""
    out = []
    for n in VOLUME_SIZES:
        for pname, T in integration_poses(n).items():
            for h, w in IMAGE_SHAPES:
                out.append(("%dx%dx%d %s %dx%d" % (n + (pname, h, w)), n, T, integration_image(h, w), integration_cam(h, w)))
            out.append(("%dx%dx%d %s 9x33 holes" % (n + (pname,)), n, T, integration_image(9, 33, holes=True),
                        integration_cam(9, 33)))
    return out


def weight_case():
    """The 16^3 volume from its centre pose, two 9x33 images that differ by 1/32 m in the right half: alternated, F keeps
    moving there and stays exactly -1, 0 or 1 at the left half's exact depths.  -> (n, T, [image A, image B], cam)"""
    n = VOLUME_SIZES[0]
    return n, integration_poses(n)["centre"], [integration_image(9, 33), integration_image(9, 33, shift=0.03125)], \
        integration_cam(9, 33)


# ---------------------------------------------------------------- the fused scene of the ray casts
def scene_of(n):
    """A wall across the volume and a box in front of it, in the volume frame: dict(wall z, box z, box half sizes)."""
    depth = n[2] * VOXEL
    return dict(wall=0.6 * depth, box=0.4 * depth, hx=0.1 * depth, hy=0.08 * depth)


FUSE_CAM = dict(fx=100.0, fy=100.0, cx=63.5, cy=47.5, depth_scale=1.0, z_min=0.1, z_max=10.0)
FUSE_W, FUSE_H = 128, 96
FUSE_AT = [(0.0, 0.0, 0.07), (0.25, 0.05, 0.10), (-0.25, 0.125, 0.05)]     # the three cameras, all looking along +z


def fuse_frames(n):
    """[(z image float32 metres, cam, T_vol_cam)] x 3: the scene of `n` seen from FUSE_AT (scaled with the depth), with a
    few millimetres of relief.  The space behind the box is seen by nobody: an unseen gap before the wall."""
    sc = scene_of(n)
    s = n[2] * VOXEL / 5.0
    u, v = np.meshgrid(np.arange(FUSE_W, dtype=np.float64), np.arange(FUSE_H, dtype=np.float64))
    dx, dy = (u - FUSE_CAM["cx"]) / FUSE_CAM["fx"], (v - FUSE_CAM["cy"]) / FUSE_CAM["fy"]
    out = []
    for c in FUSE_AT:
        c = np.array(c) * s
        zb = sc["box"] - c[2]
        on_box = (np.abs(c[0] + dx * zb) <= sc["hx"]) & (np.abs(c[1] + dy * zb) <= sc["hy"])
        z = np.where(on_box, zb, sc["wall"] - c[2]) + 0.002 * s * (((u * 7 + v * 13) % 5) - 2)
        out.append((z.astype(np.float32), dict(FUSE_CAM), edge_inputs.rigid(t=c)))
    return out


def fused(n, cls=V.Volume, max_weight=2):
    """the restated volume of size n after its three frames"""
    vol = cls(**volume_spec(n, max_weight))
    for z, cam, T in fuse_frames(n):
        vol.integrate(V.z_image(z, cam), cam, T)
    return vol


RAY_N = VOLUME_SIZES[2]
RAY_W, RAY_H = 65, 49
RAY_CAM = dict(fx=50.0, fy=50.0, cx=32.0, cy=24.0, z_min=0.1, z_max=10.0)      # integer cx, cy: d[0] == 0 at u == 32
TURN_Y = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])        # 90 degrees about y, exact: looks along +x


def ray_cases():
    """[(name, T_vol_cam, cam, w, h)] on the 72x24x40 volume (9 x 3 x 5 m; wall at z = 3, box at z = 2 of 1 x 0.8 m)."""
    R = edge_inputs.rigid
    sc = scene_of(RAY_N)
    half_x = 0.5 * RAY_N[0] * VOXEL
    back = R(K.axis_rotation((0.0, 1.0, 0.0), 180.0), (1.2, 0.1, sc["wall"] + 0.6))
    gap = R(K.axis_rotation((0.0, 1.0, 0.0), 75.0), (-1.3, 0.0, 2.55))
    out = [("zero inside", R(t=(0.0625, 0.0625, 0.3)), RAY_CAM),                   # d[0] == 0 and d[1] == 0, o inside the slabs
           ("zero outside x", R(t=(-half_x - 0.5, 0.0, 0.3)), RAY_CAM),            # o outside the x slab: column 32 misses
           ("zero outside y", R(t=(0.0, 1.45, 0.3)), RAY_CAM),                     # between the volume's face and the shrunk one
           ("turned inside", R(TURN_Y, (-1.4, 0.0, 2.6)), RAY_CAM),                # d[2] == 0 at u == 32, o inside the z slab
           ("turned outside z", R(TURN_Y, (-1.4, 0.0, -0.5)), RAY_CAM),            # ... and outside it
           ("inside", R(K.axis_rotation((0.3, 1.0, 0.1), 12.0), (0.2, -0.1, 0.6)), RAY_CAM),
           ("outside", R(t=(0.3, -0.2, -1.5)), RAY_CAM),
           ("behind the wall", back, RAY_CAM),                                     # the back face of the wall
           ("z_max before the surface", R(t=(0.0, 0.0, 0.3)), dict(RAY_CAM, z_max=1.4)),
           ("z_min behind the surface", R(t=(0.0, 0.0, 0.3)), dict(RAY_CAM, z_min=2.8)),
           ("across the gap", gap, RAY_CAM)]                                       # through the box's shadow to the wall
    out = [(name, T, cam, RAY_W, RAY_H) for name, T, cam in out]
    for h, w in ((1, 1), (33, 9), (9, 33), (31, 7)):                               # against the 32 x 8 tile
        f = 0.8 * max(h, w) + 2.0
        cam = dict(fx=f, fy=1.03 * f, cx=0.37 * w + 0.25, cy=0.58 * h - 0.125, z_min=0.1, z_max=10.0)
        out.append(("shape %dx%d" % (h, w), R(K.axis_rotation((0.3, 1.0, 0.1), 12.0), (0.2, -0.1, 0.6)), cam, w, h))
    return out


def small_ray_cases(n):
    """two cameras for the small volumes: outside before the near face, and inside"""
    depth = n[2] * VOXEL
    cam = dict(fx=30.0, fy=31.0, cx=16.3, cy=4.2, z_min=0.1, z_max=10.0)
    return [("outside", edge_inputs.rigid(t=(0.0, 0.0, -0.25 * depth)), cam, 33, 9),
            ("inside", edge_inputs.rigid(K.axis_rotation((0.2, 1.0, 0.0), 10.0), (0.05, 0.0, 0.1 * depth)), cam, 33, 9)]


def special_ray_cases():
    """[(name, n, frames [(z image, cam, T_vol_cam)], T_vol_cam, cam, w, h)]: ray casts that need a volume of their own.
      zero then negative   the 16^3 volume after one 33x33 frame that is exactly SURFACE_Z everywhere, cast from the
                           frame's own pose: the samples t = 0.1 + k / 8 fall into voxels with F = 0.5, 0, -0.5.  A sample
                           F == 0 before a negative one is no crossing (F_prev > 0), and the whole slab of voxels around
                           it is seen, so a rule with F_prev >= 0 would return a hit at the surface where this one misses;
      low sliver           a wall seen from a camera whose centre lies between the volume's y face and the shrunk slab's,
                           above the half voxel from which a trilinear read succeeds; the row v == cy has d[1] == 0 and
                           must miss although everything a hit needs is there;
      inside the band      on the 72x24x40 scene from a camera inside the box's band (F < 0) that looks sideways: its rays
                           leave the band into free space (a back face: the ray ends) with the wall's front still ahead."""
    n = VOLUME_SIZES[0]
    T, cam = integration_poses(n)["centre"], integration_cam(33, 33)
    out = [("zero then negative", n, [(np.full((33, 33), SURFACE_Z, np.float32), cam, T)], T, integration_cam(9, 33), 33, 9)]
    spec = volume_spec(n)
    at = edge_inputs.rigid(t=(0.03, spec["origin"][1] + 0.1, 0.07))
    u, v = np.meshgrid(np.arange(FUSE_W), np.arange(FUSE_H))
    wall = (1.2 + 0.002 * (((u * 7 + v * 13) % 5) - 2)).astype(np.float32)
    out.append(("low sliver", n, [(wall, dict(FUSE_CAM), at)], at, dict(fx=30.0, fy=30.0, cx=16.0, cy=4.0, z_min=0.1, z_max=10.0),
                33, 9))
    side = edge_inputs.rigid(K.axis_rotation((0.0, 1.0, 0.0), 50.0), (0.4, 0.0, 2.12))
    out.append(("inside the band", RAY_N, fuse_frames(RAY_N), side, RAY_CAM, RAY_W, RAY_H))
    return out


def full_cam(cam):
    """a ray-cast camera as the restatement's dict"""
    return dict(cam, depth_scale=1.0)
