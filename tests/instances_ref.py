"""numpy restatement of the instance selection of include/oslam.h (oslam_align_instances / oslam_select_instances):
candidate order, the same-instance test in float32 with the header's order of operations, greedy suppression with the
score floor and the max_instances cap.  Also the candidates of the default clustering from the host pose stage's
outputs, and the model centroid / extent."""
import math

import numpy as np

F = np.float32
PI_F = F(math.pi)


def centroid(points):
    """mean of the points in double, rounded to float"""
    return np.asarray(points, np.float64).mean(axis=0).astype(np.float32)


def extent(points):
    """largest bounding-box side in float (oslam_d_dist_from_cloud with tau 1)"""
    p = np.asarray(points, np.float32)
    side = p.max(axis=0) - p.min(axis=0)
    return F(max(side[0], side[1], side[2]))


def thresholds(min_separation, max_angle, ext):
    sep = float(F(min_separation)) * float(ext)
    sep2 = F(sep * sep)
    cos_thr = F(1.0 + 2.0 * math.cos(float(F(max_angle))))
    return sep2, cos_thr, bool(F(max_angle) < PI_F)


def transformed_centroid(T, c):
    T = np.asarray(T, np.float32).reshape(16)
    return [F(F(F(T[4 * k] * c[0]) + F(T[4 * k + 1] * c[1])) + F(T[4 * k + 2] * c[2])) + T[4 * k + 3] for k in range(3)]


def rotation_sum(A, B):
    A = np.asarray(A, np.float32).reshape(16)
    B = np.asarray(B, np.float32).reshape(16)
    s = F(0)
    for i in range(3):
        for j in range(3):
            s = F(s + F(A[4 * i + j] * B[4 * i + j]))
    return s


def same_instance(pa, A, pb, B, sep2, cos_thr, rot_on):
    dx, dy, dz = F(pa[0] - pb[0]), F(pa[1] - pb[1]), F(pa[2] - pb[2])
    d2 = F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
    if not d2 < sep2:
        return False
    return (not rot_on) or bool(rotation_sum(A, B) >= cos_thr)


def select(T, scores, c, ext, max_instances=8, min_separation=0.5, max_angle=math.pi, min_score_ratio=0.5):
    """-> accepted candidate indices in acceptance order"""
    T = np.asarray(T, np.float32).reshape(-1, 16)
    scores = np.asarray(scores, np.float32)
    sep2, cos_thr, rot_on = thresholds(min_separation, max_angle, ext)
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    p = [transformed_centroid(T[i], c) for i in range(len(T))]
    acc, floor_v = [], None
    for i in order:
        if len(acc) >= max_instances:
            break
        if acc and scores[i] < floor_v:
            break
        if any(same_instance(p[i], T[i], p[a], T[a], sep2, cos_thr, rot_on) for a in acc):
            continue
        if not acc:
            floor_v = F(F(min_score_ratio) * scores[i])
        acc.append(i)
    return np.array(acc, np.uint32)


def default_candidates(poses, trans):
    """every kept cell's pose with the clustering-stage translation"""
    T = np.array(poses, np.float32).reshape(-1, 4, 4)
    tr = np.asarray(trans, np.float32).reshape(-1, 3)
    T[:, :3, 3] = tr
    return T
