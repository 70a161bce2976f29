"""The clouds of the model-table tests: a table of names -> (points, normals, d_dist), seeded, and their restatements
(tests/model_ref.py), computed once per process and shared.  d_dist is coarse wherever the edge allows it, so that a
model of n points has few keys and the restatement of its n^2 pairs stays at seconds.  tests/test_model_tables_host.py
proves on the CPU oracle that every cloud reaches the edge it is named for; tests/test_gpu_model_tables.py holds the
device to the restatement on the same clouds."""
import time

import numpy as np

import model_ref as R
from test_gpu_wide_keys import mixed_run_case, random_cloud

COARSE = 0.5                           # unit cube [-1, 1]^3: seven distance bins
COUNTS = (2, 3, 1023, 1024, 2046, 2047, 4093)

CLOUDS = {}


def cloud(fn):
    CLOUDS[fn.__name__] = fn
    return fn


def _count_cloud(n):
    def build():
        p, nr = random_cloud(n, 2600 + n)
        return p, nr, COARSE
    build.__name__ = "points_%d" % n
    return cloud(build)


for _n in COUNTS:
    _count_cloud(_n)


@cloud
def markers():
    """test_gpu_wide_keys.mixed_run_case's scene as a model: point 0 at the origin with the normal (1, 0, 0), point 1 on
    that axis (its pair under point 0 has uy = uz = 0: the marker) and point 60, the same point 1e-5 off the axis, whose
    pair shares the key and is clean; then point 5 twice more, once with its normal and once with another (pairs of
    length 0: markers whichever of the three is the reference point)"""
    _, _, sp, sn, d = mixed_run_case()
    p = np.concatenate([sp, sp[5:6], sp[5:6]])
    nr = np.concatenate([sn, sn[5:6], sn[7:8]])
    return p, nr, d


@cloud
def growth():
    """one slice, fine d_dist: more than 32768 distinct keys, so the slice table must grow past 2^16 slots"""
    p, nr = random_cloud(300, 2701)
    return p, nr, float(np.float32(3.5 / 1000))


@cloud
def far_beyond_the_key_map():
    """three points, the third some 3000 distance bins from the other two: beyond the key map's 2048 bins, inside reach"""
    p = np.float32([[0, 0, 0], [0.0012, 0.0003, 0], [1.5, 0.1, -0.2]])
    nr = np.float32([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0]])
    return p, nr, 0.0005


@cloud
def far_beyond_reach():
    """three points, the third some 20000 distance bins away: beyond the 16384 bins of the reach bitset"""
    p = np.float32([[0, 0, 0], [0.0012, 0.0003, 0], [9.5, 3.0, -1.0]])
    nr = np.float32([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0]])
    return p, nr, 0.0005


@cloud
def small():
    """the cloud of the parameter variants, of save and load, and the first member of the group"""
    p, nr = random_cloud(150, 2702)
    return p, nr, COARSE


@cloud
def small_other():
    """the group's second member: another size, partly other keys"""
    p, nr = random_cloud(90, 2703)
    return p * np.float32(1.7), nr, COARSE


_REFS = {}
SECONDS = {}


def reference(name, oracle, ppf):
    """-> (points, normals, d_dist, model_ref.Model, model_ref.Union), computed once"""
    if name not in _REFS:
        p, nr, d = CLOUDS[name]()
        t0 = time.process_time()
        m = R.Model(p, nr, d, oracle, ppf)
        u = R.Union([m], d)
        SECONDS[name] = time.process_time() - t0
        _REFS[name] = (p, nr, d, m, u)
    return _REFS[name]
