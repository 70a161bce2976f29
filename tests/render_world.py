"""The moving-object frames of the render tests: the static planes of tests/camera_ref.py seen by a camera that moves
along camera_ref.trajectory, and one synth object in front of them that moves on its own between the two frames.  The
camera motion between the frames is estimated three ways (raw frames, frames with the object masked out by a render at
its true pose, frames that never held the object); tests/test_render_host.py does that with the restatements and holds
the numbers, tests/test_gpu_render.py does it on the device.  numpy only; seeded."""
import numpy as np

import camera_ref as CR
import render_ref as R
import track_ref as K

F = np.float32
W, H = 160, 120
# the stream camera of tests/track_ref.py at a quarter of its resolution (pixel centres stay where they were)
CAM = dict(fx=K.STREAM_CAM["fx"] / 4, fy=K.STREAM_CAM["fy"] / 4, cx=(K.STREAM_CAM["cx"] + 0.5) / 4 - 0.5,
           cy=(K.STREAM_CAM["cy"] + 0.5) / 4 - 0.5, depth_scale=0.001, z_min=0.3, z_max=10.0)
FCAM = dict(CAM, depth_scale=1.0)           # the same camera over float images in metres
MAX_JUMP = 4 * CR.MAX_JUMP                  # a pixel is four times as wide
SIZE = dict(width=W, height=H, fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"])
OBJECT_MODEL, OBJECT_SCALE = 0, 0.3
OBJECT_AT = (0.1, 0.3, 1.3)                 # metres before the first camera: a fifth of the image's pixels
OBJECT_TURN, OBJECT_STEP = 3.0, (0.05, 0.0, 0.02)      # its own motion between the frames: degrees, metres
# The camera's motion between the frames.  Half of camera_ref.trajectory's default rate: the three planes alone hold
# the sideways translation only through the strip of side wall at the image's left edge, and at 3 degrees a frame that
# strip starts outside the correspondence gate (measured: the planes-only estimate is then 0.25 m off sideways, with
# the object or without it).
CAMERA_DEG, CAMERA_STEP = 1.5, 0.03


def make(synth, oracle):
    """-> dict: cloud (the object's model: points, normals, d_dist), T_obj [2] (model -> camera, float32), frames [2]
    (uint16, with the object), empty [2] (uint16, without it), T_wc [2], truth (camera 0 -> camera 1)."""
    planes = CR.make_world(synth, planes_only=True)
    dense, _ = synth.make_model(OBJECT_MODEL, 150000)
    dense = OBJECT_SCALE * dense.astype(np.float64)
    mp, mn = synth.make_model(OBJECT_MODEL, 20000)
    mp = np.ascontiguousarray(mp * F(OBJECT_SCALE))
    d = synth.d_dist_for(mp, 0.05)
    gp, gn = oracle.voxel_grid(mp, mn, d)
    rng = synth.SplitMix64(4711)
    T0 = np.eye(4)
    T0[:3, :3] = synth.random_rotation(rng)
    T0[:3, 3] = OBJECT_AT
    D = np.eye(4)
    D[:3, :3] = K.axis_rotation((0.2, 1.0, 0.1), OBJECT_TURN)
    c = np.asarray(OBJECT_AT)
    D[:3, 3] = c - D[:3, :3] @ c + np.asarray(OBJECT_STEP)          # turns about its own centre, then steps
    T_wo = [T0, D @ T0]
    T_wc = CR.trajectory(synth, frames=2, deg=CAMERA_DEG, step=CAMERA_STEP)
    frames, empty, T_obj = [], [], []
    for f in range(2):
        obj = dense @ T_wo[f][:3, :3].T + T_wo[f][:3, 3]
        frames.append(CR.render(synth, np.concatenate([planes, obj]), T_wc[f], **SIZE))
        empty.append(CR.render(synth, planes, T_wc[f], **SIZE))
        T_obj.append((np.linalg.inv(T_wc[f]) @ T_wo[f]).astype(np.float32))
    return dict(cloud=(gp, gn, d), T_obj=T_obj, frames=frames, empty=empty, T_wc=T_wc, truth=CR.truth(T_wc[0], T_wc[1]))


def masked_frames(w):
    """the frames with the object removed by the restatement: float32 z images in metres (FCAM), and the mask counters"""
    out, counts = [], []
    for f in range(2):
        r = R.render([w["cloud"]], w["T_obj"][f][None], FCAM, W, H)
        z_o = R.V.view_z(w["frames"][f], CAM["depth_scale"], CAM["z_min"], CAM["z_max"])
        z, cnt = R.mask(z_o, r, R.REMOVE)
        out.append(z)
        counts.append(cnt)
    return out, counts


def cpu_egomotion(img0, img1, cam):
    """camera_ref.egomotion between two frames of one camera: -> T float32 4x4 (camera 0 -> camera 1), result dict"""
    m0, m1 = K.view_maps(img0, cam, MAX_JUMP), K.view_maps(img1, cam, MAX_JUMP)
    return CR.egomotion(m0, m1, cam)


def cpu_three_ways(w):
    """-> {"raw" | "masked" | "empty": (T, result dict)} on the restatements"""
    masked, _ = masked_frames(w)
    return {"raw": cpu_egomotion(w["frames"][0], w["frames"][1], CAM),
            "masked": cpu_egomotion(masked[0], masked[1], FCAM),
            "empty": cpu_egomotion(w["empty"][0], w["empty"][1], CAM)}
