"""Python mirror of the reference's registration interface over the C-ABI.

The reference exposes (pcl/alignment/include/): ``ppf_registration(...)``
(ppf.h:9-15), ``class Scene`` (scene.h:10-52) and ``class Model`` (model.h:14-115)
with ``Model::ppf_lookup(Scene*)``.  The same names, argument meaning and result
fields live here, on top of ``liboslam_hip.so`` (include/oslam.h) through ctypes.
Clouds are numpy arrays: points ``[n,3]`` float32 and normals ``[n,3]`` float32,
or one ``[n,12]`` float32 array laid out like ``pcl::PointNormal`` (48 bytes).

There is no CPU fallback: if the shared library is missing, or no HIP device is
present, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OSLAM_LIB", os.path.join(_HERE, "liboslam_hip.so"))   # OSLAM_LIB: A/B builds
_LIB = None

OSLAM_OK, OSLAM_E_INVALID, OSLAM_E_DEVICE, OSLAM_E_NOMEM, OSLAM_E_NO_VOTES, OSLAM_E_LIMIT, OSLAM_E_PEER = range(7)
STAGE_VOTE, STAGE_SELECT, STAGE_GROW = 1, 2, 3       # oslam_comm_inject_failure
VOTE_EXACT, VOTE_FAST = 0, 1
COMM_ID_BYTES = 128


class OslamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("oslam error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("ref_point_df", C.c_uint), ("vote_count_threshold", C.c_float),
                ("cpu_clustering", C.c_int), ("use_l1_norm", C.c_int), ("use_averaged_clusters", C.c_int),
                ("dev", C.c_int), ("vote_mode", C.c_int), ("shard_rank", C.c_int), ("shard_world", C.c_int),
                ("max_cells", C.c_uint), ("pose_gpu_min", C.c_uint), ("no_bucket_spread", C.c_int),
                ("scratch_gib", C.c_uint), ("pose_two_sorts", C.c_int), ("vote_order", C.c_int), ("reserved", C.c_int * 1)]


class Stats(C.Structure):
    _fields_ = [("num_scene_ppfs", C.c_uint64), ("num_hits", C.c_uint64), ("num_votes", C.c_uint64),
                ("num_unique_votes", C.c_uint64), ("num_model_keys", C.c_uint64), ("num_top", C.c_uint64),
                ("max_count", C.c_uint32), ("num_emitted", C.c_uint32), ("ms_vote", C.c_float),
                ("ms_total", C.c_float), ("vote_launches", C.c_uint32), ("ms_vote_kernel", C.c_float),
                ("ms_key_kernel", C.c_float), ("wide_workgroups", C.c_uint32), ("num_pairs_probed", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("num_entries_streamed", C.c_uint64), ("num_items", C.c_uint64)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class RefineParams(C.Structure):
    _fields_ = [("max_iterations", C.c_uint), ("max_corr_dist", C.c_float), ("min_normal_dot", C.c_float),
                ("inlier_dist", C.c_float), ("min_fitness", C.c_float), ("stop_rot", C.c_float), ("stop_trans", C.c_float),
                ("reserved", C.c_int * 4)]


class RefineResult(C.Structure):
    _fields_ = [("fitness_in", C.c_float), ("fitness", C.c_float), ("rmse", C.c_float), ("inliers", C.c_uint32),
                ("correspondences", C.c_uint32), ("iterations", C.c_uint32), ("converged", C.c_int32),
                ("found", C.c_int32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class VerifyParams(C.Structure):
    _fields_ = [("depth_tol", C.c_float), ("window", C.c_uint), ("min_view_fitness", C.c_float),
                ("min_coverage", C.c_float), ("min_supported", C.c_uint), ("reserved", C.c_int * 4)]


class VerifyResult(C.Structure):
    _fields_ = [("back", C.c_uint32), ("out", C.c_uint32), ("supported", C.c_uint32), ("occluded", C.c_uint32),
                ("conflict", C.c_uint32), ("unknown", C.c_uint32), ("view_fitness", C.c_float), ("coverage", C.c_float),
                ("found", C.c_int32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


VERIFY_BACK, VERIFY_OUT, VERIFY_SUPPORTED, VERIFY_OCCLUDED, VERIFY_CONFLICT, VERIFY_UNKNOWN = range(6)


class InstanceParams(C.Structure):
    _fields_ = [("max_instances", C.c_uint), ("min_separation", C.c_float), ("max_angle", C.c_float),
                ("min_score_ratio", C.c_float), ("keep_not_found", C.c_int), ("reserved", C.c_int * 4)]


class Instance(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("T_vote", C.c_float * 16), ("score", C.c_float), ("candidate", C.c_uint32),
                ("refine", RefineResult)]

    def astuple(self):
        """-> (T 4x4, info dict: T_vote 4x4, score, candidate, refine dict)"""
        T = np.array(self.T, np.float32).reshape(4, 4)
        return T, {"T_vote": np.array(self.T_vote, np.float32).reshape(4, 4), "score": float(self.score),
                   "candidate": int(self.candidate), "refine": self.refine.asdict()}


MAX_INSTANCES = 64


class ArbitrateParams(C.Structure):
    _fields_ = [("depth_tol", C.c_float), ("window", C.c_uint), ("tile", C.c_uint), ("tile_spacing", C.c_float),
                ("min_tiles", C.c_uint), ("min_owned_share", C.c_float), ("reserved", C.c_int * 4)]


class ArbitrateResult(C.Structure):
    _fields_ = [("claimed", C.c_uint32), ("owned", C.c_uint32), ("share", C.c_float), ("mean_residual", C.c_float),
                ("kept", C.c_int32), ("suppressed_by", C.c_int32), ("tile", C.c_uint32), ("rounds", C.c_uint32),
                ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class DetectParams(C.Structure):
    _fields_ = [("instances", InstanceParams), ("refine", RefineParams), ("verify", VerifyParams),
                ("arbitrate", ArbitrateParams), ("reserved", C.c_int * 4)]


class Detection(C.Structure):
    _fields_ = [("model", C.c_uint32), ("instance", C.c_uint32), ("T", C.c_float * 16), ("verify", VerifyResult),
                ("arbitrate", ArbitrateResult)]

    def asdict(self):
        return {"model": int(self.model), "instance": int(self.instance), "T": np.array(self.T, np.float32).reshape(4, 4),
                "verify": self.verify.asdict(), "arbitrate": self.arbitrate.asdict()}


class TrackParams(C.Structure):
    _fields_ = [("max_iterations", C.c_uint), ("max_corr_dist", C.c_float), ("min_normal_dot", C.c_float),
                ("stop_rot", C.c_float), ("stop_trans", C.c_float), ("verify", VerifyParams), ("reserved", C.c_int * 4)]


class TrackResult(C.Structure):
    _fields_ = [("verify", VerifyResult), ("iterations", C.c_uint32), ("correspondences", C.c_uint32),
                ("converged", C.c_int32), ("found", C.c_int32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"verify": self.verify.asdict(), "iterations": int(self.iterations),
                "correspondences": int(self.correspondences), "converged": int(self.converged), "found": int(self.found),
                "launches": int(self.launches), "ms_total": float(self.ms_total)}


class TrackerParams(C.Structure):
    _fields_ = [("track", TrackParams), ("detect", DetectParams), ("arbitrate", ArbitrateParams), ("max_misses", C.c_uint),
                ("detect_every", C.c_uint), ("assoc_min_separation", C.c_float), ("assoc_max_angle", C.c_float),
                ("reserved", C.c_int * 4)]


class TrackState(C.Structure):
    _fields_ = [("id", C.c_uint32), ("model", C.c_uint32), ("T", C.c_float * 16), ("age", C.c_uint32), ("hits", C.c_uint32),
                ("misses", C.c_uint32), ("found", C.c_int32), ("track", TrackResult)]

    def asdict(self):
        return {"id": int(self.id), "model": int(self.model), "T": np.array(self.T, np.float32).reshape(4, 4),
                "age": int(self.age), "hits": int(self.hits), "misses": int(self.misses), "found": int(self.found),
                "track": self.track.asdict()}


class EgomotionLevel(C.Structure):
    _fields_ = [("stride", C.c_uint), ("max_iterations", C.c_uint)]


class EgomotionParams(C.Structure):
    _fields_ = [("n_levels", C.c_uint), ("level", EgomotionLevel * 3), ("max_corr_dist", C.c_float),
                ("min_normal_dot", C.c_float), ("stop_rot", C.c_float), ("stop_trans", C.c_float), ("min_overlap", C.c_float),
                ("reserved", C.c_int * 4)]


class EgomotionResult(C.Structure):
    _fields_ = [("iterations", C.c_uint32 * 3), ("correspondences", C.c_uint32), ("rmse", C.c_float), ("overlap", C.c_float),
                ("converged", C.c_int32), ("ok", C.c_int32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"iterations": [int(x) for x in self.iterations], "correspondences": int(self.correspondences),
                "rmse": float(self.rmse), "overlap": float(self.overlap), "converged": int(self.converged), "ok": int(self.ok),
                "launches": int(self.launches), "ms_total": float(self.ms_total)}


class PyramidParams(C.Structure):
    _fields_ = [("n_levels", C.c_uint), ("depth_band", C.c_float), ("reserved", C.c_int * 4)]


class RenderParams(C.Structure):
    _fields_ = [("footprint", C.c_float), ("max_splat", C.c_uint), ("depth_tol", C.c_float), ("keep_back", C.c_int),
                ("reserved", C.c_int * 4)]


class RenderResult(C.Structure):
    _fields_ = [("drawn", C.c_uint32), ("pixels", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class MaskParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("dilate", C.c_uint), ("only", C.c_int32), ("reserved", C.c_int * 4)]


class MaskResult(C.Structure):
    _fields_ = [("valid_in", C.c_uint32), ("object_pixels", C.c_uint32), ("valid_out", C.c_uint32),
                ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


MASK_REMOVE, MASK_KEEP = 0, 1


class PlanesParams(C.Structure):
    _fields_ = [("dist_tol", C.c_float), ("min_normal_dot", C.c_float), ("label_min_dot", C.c_float),
                ("max_planes", C.c_uint), ("min_pixels", C.c_uint), ("reserved", C.c_int * 4)]


class Plane(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("d", C.c_float), ("support", C.c_uint32), ("pixels", C.c_uint32),
                ("candidate", C.c_uint32), ("rms", C.c_float)]

    def asdict(self):
        return dict(normal=tuple(self.normal), d=self.d, support=self.support, pixels=self.pixels,
                    candidate=self.candidate, rms=self.rms)


class PlanesResult(C.Structure):
    _fields_ = [("n_planes", C.c_uint32), ("valid_in", C.c_uint32), ("labelled", C.c_uint32), ("launches", C.c_uint32),
                ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


PLANES_MAX = 8
PLANES_CANDIDATES = 256


class SegmentsParams(C.Structure):
    _fields_ = [("max_step", C.c_float), ("rel_step", C.c_float), ("min_pixels", C.c_uint), ("max_segments", C.c_uint),
                ("reserved", C.c_int * 4)]


class Segment(C.Structure):
    _fields_ = [("pixels", C.c_uint32), ("root", C.c_uint32), ("u0", C.c_uint16), ("v0", C.c_uint16), ("u1", C.c_uint16),
                ("v1", C.c_uint16), ("centroid", C.c_float * 3), ("sides", C.c_uint32)]

    def asdict(self):
        return dict(pixels=self.pixels, root=self.root, box=(self.u0, self.v0, self.u1, self.v1),
                    centroid=tuple(self.centroid), sides=self.sides)


class SegmentsResult(C.Structure):
    _fields_ = [("n_segments", C.c_uint32), ("n_components", C.c_uint32), ("n_candidates", C.c_uint32),
                ("valid_in", C.c_uint32), ("labelled", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


SEGMENTS_MAX = 64
SEGMENTS_CANDIDATES = 4096
SEGMENTS_LAUNCHES = 6


class BilateralParams(C.Structure):
    _fields_ = [("radius", C.c_uint), ("sigma_space", C.c_float), ("sigma_depth", C.c_float), ("reserved", C.c_int * 4)]


class BilateralResult(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("taps", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


BILATERAL_MAX_RADIUS = 8
GAUSS_TABLE_N = 288


class ExplainParams(C.Structure):
    _fields_ = [("footprint", C.c_float), ("max_splat", C.c_uint), ("keep_back", C.c_int), ("depth_tol", C.c_float),
                ("tile", C.c_uint), ("tile_spacing", C.c_float), ("min_tiles", C.c_uint), ("min_owned_share", C.c_float),
                ("reserved", C.c_int * 4)]


class ExplainResult(C.Structure):
    _fields_ = [("drawn", C.c_uint32), ("pixels", C.c_uint32), ("agree", C.c_uint32), ("occluded", C.c_uint32),
                ("through", C.c_uint32), ("unknown", C.c_uint32), ("resid_sum", C.c_uint64), ("explained", C.c_float),
                ("visible", C.c_float), ("mean_residual", C.c_float), ("conflict_q", C.c_uint32), ("claimed", C.c_uint32),
                ("owned", C.c_uint32), ("share", C.c_float), ("kept", C.c_int32), ("suppressed_by", C.c_int32),
                ("tile", C.c_uint32), ("rounds", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class VolumeParams(C.Structure):
    _fields_ = [("nx", C.c_uint), ("ny", C.c_uint), ("nz", C.c_uint), ("voxel", C.c_float), ("origin", C.c_float * 3),
                ("mu", C.c_float), ("max_weight", C.c_uint), ("reserved", C.c_int * 4)]


class IntegrateResult(C.Structure):
    _fields_ = [("updated", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"updated": int(self.updated), "launches": int(self.launches), "ms_total": float(self.ms_total)}


class ColourParams(C.Structure):
    _fields_ = [("max_weight", C.c_uint), ("band", C.c_float), ("reserved", C.c_int * 6)]


class RaycastResult(C.Structure):
    _fields_ = [("hits", C.c_uint32), ("normals", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"hits": int(self.hits), "normals": int(self.normals), "launches": int(self.launches),
                "ms_total": float(self.ms_total)}


class SurfaceParams(C.Structure):
    _fields_ = [("min_weight", C.c_uint), ("reserved", C.c_int * 7)]


class SurfaceResult(C.Structure):
    _fields_ = [("crossings", C.c_uint32), ("points", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"crossings": int(self.crossings), "points": int(self.points), "launches": int(self.launches),
                "ms_total": float(self.ms_total)}


class MeshParams(C.Structure):
    _fields_ = [("min_weight", C.c_uint), ("reserved", C.c_int * 7)]


class MeshResult(C.Structure):
    _fields_ = [("vertices", C.c_uint32), ("triangles", C.c_uint32), ("cubes", C.c_uint32), ("launches", C.c_uint32),
                ("ms_total", C.c_float)]

    def asdict(self):
        return {"vertices": int(self.vertices), "triangles": int(self.triangles), "cubes": int(self.cubes),
                "launches": int(self.launches), "ms_total": float(self.ms_total)}


class ShiftResult(C.Structure):
    _fields_ = [("offset", C.c_int32 * 3), ("kept", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"offset": tuple(int(x) for x in self.offset), "kept": int(self.kept), "launches": int(self.launches),
                "ms_total": float(self.ms_total)}


class FollowParams(C.Structure):
    _fields_ = [("lookahead", C.c_float), ("threshold", C.c_float), ("granule", C.c_int), ("reserved", C.c_int * 5)]


class WorldParams(C.Structure):
    _fields_ = [("voxel", C.c_float), ("origin0", C.c_float * 3), ("max_bytes", C.c_uint64), ("reserved", C.c_int * 4)]

    # oslam_world_params.colour is the first of these four ints (the C structure names it; the layout is one)
    colour = property(lambda self: int(self.reserved[0]), lambda self, v: self.reserved.__setitem__(0, int(v)))


class WorldStats(C.Structure):
    _fields_ = [("voxels", C.c_uint64), ("bricks", C.c_uint64), ("bytes", C.c_uint64), ("lo", C.c_int32 * 3),
                ("hi", C.c_int32 * 3)]

    def asdict(self):
        return {"voxels": int(self.voxels), "bricks": int(self.bricks), "bytes": int(self.bytes),
                "lo": tuple(int(x) for x in self.lo), "hi": tuple(int(x) for x in self.hi)}


class ReloadResult(C.Structure):
    _fields_ = [("offset", C.c_int32 * 3), ("kept", C.c_uint32), ("stored", C.c_uint32), ("reloaded", C.c_uint32),
                ("launches", C.c_uint32), ("ms_total", C.c_float)]

    def asdict(self):
        return {"offset": tuple(int(x) for x in self.offset), "kept": int(self.kept), "stored": int(self.stored),
                "reloaded": int(self.reloaded), "launches": int(self.launches), "ms_total": float(self.ms_total)}


class WorldSurfaceParams(C.Structure):
    _fields_ = [("min_weight", C.c_uint), ("anchor_set", C.c_int), ("anchor", C.c_int32 * 3), ("dev", C.c_int),
                ("reserved", C.c_int * 6)]


class WorldSurfaceResult(C.Structure):
    _fields_ = [("crossings", C.c_uint32), ("points", C.c_uint32), ("bricks", C.c_uint32), ("window_bricks", C.c_uint32),
                ("launches", C.c_uint32), ("anchor", C.c_int32 * 3), ("ms_total", C.c_float)]

    def asdict(self):
        return {"crossings": int(self.crossings), "points": int(self.points), "bricks": int(self.bricks),
                "window_bricks": int(self.window_bricks), "launches": int(self.launches),
                "anchor": tuple(int(x) for x in self.anchor), "ms_total": float(self.ms_total)}


class WorldMeshResult(C.Structure):
    _fields_ = [("vertices", C.c_uint32), ("triangles", C.c_uint32), ("cubes", C.c_uint32), ("bricks", C.c_uint32),
                ("window_bricks", C.c_uint32), ("launches", C.c_uint32), ("anchor", C.c_int32 * 3), ("ms_total", C.c_float)]

    def asdict(self):
        return {"vertices": int(self.vertices), "triangles": int(self.triangles), "cubes": int(self.cubes),
                "bricks": int(self.bricks), "window_bricks": int(self.window_bricks), "launches": int(self.launches),
                "anchor": tuple(int(x) for x in self.anchor), "ms_total": float(self.ms_total)}


class WorldRaycastParams(C.Structure):
    _fields_ = [("anchor_set", C.c_int), ("anchor", C.c_int32 * 3), ("box_set", C.c_int), ("box_lo", C.c_int32 * 3),
                ("box_hi", C.c_int32 * 3), ("mu", C.c_float), ("dev", C.c_int), ("reserved", C.c_int * 6)]


class WorldRaycastResult(C.Structure):
    _fields_ = [("hits", C.c_uint32), ("normals", C.c_uint32), ("bricks", C.c_uint32), ("window_bricks", C.c_uint32),
                ("launches", C.c_uint32), ("anchor", C.c_int32 * 3), ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
                ("ms_total", C.c_float)]

    def asdict(self):
        return {"hits": int(self.hits), "normals": int(self.normals), "bricks": int(self.bricks),
                "window_bricks": int(self.window_bricks), "launches": int(self.launches),
                "anchor": tuple(int(x) for x in self.anchor), "box_lo": tuple(int(x) for x in self.box_lo),
                "box_hi": tuple(int(x) for x in self.box_hi), "ms_total": float(self.ms_total)}


class ModelTables(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("cap", "shift", "n_slices", "ucap", "ushift", "n_entries", "n_ids", "id_bits",
                                          "uinfo_stride", "kmap_bins", "reach_words", "has_pw")] + \
               [("num_model_keys", C.c_uint64), ("reserved", C.c_uint32 * 2)]

    def asdict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_ if f != "reserved"}


class NormalsParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("min_neighbours", C.c_uint), ("viewpoint", C.c_float * 3), ("orient", C.c_int),
                ("line_ratio", C.c_float), ("reserved", C.c_int * 4)]


class NormalsResult(C.Structure):
    _fields_ = [("n_valid", C.c_uint32), ("n_cells", C.c_uint32), ("edge", C.c_float), ("launches", C.c_uint32),
                ("ms_total", C.c_float), ("ms_grid", C.c_float), ("ms_kernel", C.c_float)]

    def asdict(self):
        return {"n_valid": int(self.n_valid), "n_cells": int(self.n_cells), "edge": float(self.edge),
                "launches": int(self.launches), "ms_total": float(self.ms_total), "ms_grid": float(self.ms_grid),
                "ms_kernel": float(self.ms_kernel)}


NORMALS_SWEEPS = 4
ARBITRATE_MAX_HYPOTHESES = 1024
CELL_DTYPE = np.dtype([("code", "<u8"), ("count", "<u4"), ("pad", "<u4")])

# every function include/oslam.h declares: (name, restype, argtypes)
_vp, _sz, _f, _i, _u = C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_uint
_SIGNATURES = {
    "oslam_params_default": (_i, [C.POINTER(Params)]),
    "oslam_d_dist_from_cloud": (_i, [_vp, _sz, _sz, _f, C.POINTER(_f)]),
    "oslam_model_create": (_i, [_vp, _vp, _sz, _sz, _f, C.POINTER(Params), C.POINTER(_vp)]),
    "oslam_model_destroy": (None, [_vp]),
    "oslam_model_set_point_weights": (_i, [_vp, _vp, _sz]),
    "oslam_model_save": (_i, [_vp, C.c_char_p]),
    "oslam_model_load": (_i, [C.c_char_p, C.POINTER(Params), C.POINTER(_vp)]),
    "oslam_model_info": (_i, [_vp, C.POINTER(_sz), C.POINTER(_f), C.POINTER(C.c_uint64)]),
    "oslam_scene_create": (_i, [_vp, _vp, _sz, _sz, _f, _u, C.POINTER(Params), C.POINTER(_vp)]),
    "oslam_scene_destroy": (None, [_vp]),
    "oslam_align": (_i, [_vp, _vp, _vp, C.POINTER(Stats)]),
    "oslam_align_prepare": (_i, [_vp, _vp]),
    "oslam_ppf_registration": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _u, _f, _i, _i, _i, _i, _vp, _vp]),
    "oslam_ht_dist": (_i, [_vp, _vp, _vp]),
    "oslam_ply_read": (_i, [C.c_char_p, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz)]),
    "oslam_ply_write": (_i, [C.c_char_p, _vp, _vp, _sz, _i]),
    "oslam_free": (None, [_vp]),
    "oslam_depth_to_cloud": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_scene_from_depth": (_i, [_vp, _i, _i, _i, _vp, _f, _f, _u, C.POINTER(Params), C.POINTER(_vp), C.POINTER(_sz)]),
    "oslam_voxel_grid": (_i, [_vp, _vp, _sz, _sz, _f, _i, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_build_T_g": (None, [_vp, _vp, _vp]),
    "oslam_sort_cells": (None, [_vp, _sz]),
    "oslam_filter_cells": (_sz, [_vp, _sz, _f, C.c_uint32]),
    "oslam_pose_stage": (_i, [_vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _f, _i, _i, _i, _vp, _vp, _vp]),
    "oslam_align_local": (_i, [_vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint32), C.POINTER(Stats)]),
    "oslam_align_finish": (_i, [_vp, _vp, _vp, _sz, C.c_uint32, _vp, C.POINTER(Stats)]),
    "oslam_local_peaks": (_i, [_vp, C.c_uint32, _vp, _sz, C.POINTER(_sz)]),
    "oslam_last_result": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint32)]),
    "oslam_pose_stage_ex": (_i, [_vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "oslam_comm_unique_id": (_i, [_vp]),
    "oslam_comm_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "oslam_comm_destroy": (None, [_vp]),
    "oslam_align_multi": (_i, [_vp, _vp, _vp, _vp, C.POINTER(Stats)]),
    "oslam_comm_create_loopback": (_i, [_i, _i, C.POINTER(_vp)]),
    "oslam_comm_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "oslam_comm_inject_failure": (_i, [_vp, _i]),
    "oslam_comm_abort": (_i, [_vp]),
    "oslam_db_align_multi": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "oslam_db_destroy_with_models": (None, [_vp]),
    "oslam_release_scratch": (_i, [_i]),
    "oslam_db_create": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "oslam_db_destroy": (None, [_vp]),
    "oslam_db_align": (_i, [_vp, _vp, _vp, _vp]),
    "oslam_db_size": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "oslam_refine_params_default": (_i, [C.POINTER(RefineParams)]),
    "oslam_refine": (_i, [_vp, _vp, _vp, C.POINTER(RefineParams), _vp, C.POINTER(RefineResult)]),
    "oslam_db_refine": (_i, [_vp, _vp, _vp, C.POINTER(RefineParams), _vp, _vp]),
    "oslam_refine_correspondences": (_i, [_vp, _vp, _vp, _f, _f, _vp]),
    "oslam_view_create": (_i, [_vp, _i, _i, _i, _vp, _i, C.POINTER(_vp)]),
    "oslam_view_destroy": (_i, [_vp]),
    "oslam_verify_params_default": (_i, [C.POINTER(VerifyParams)]),
    "oslam_verify": (_i, [_vp, _vp, _vp, C.POINTER(VerifyParams), C.POINTER(VerifyResult)]),
    "oslam_db_verify": (_i, [_vp, _vp, _vp, C.POINTER(VerifyParams), _vp]),
    "oslam_verify_classes": (_i, [_vp, _vp, _vp, C.POINTER(VerifyParams), _vp]),
    "oslam_instance_params_default": (_i, [C.POINTER(InstanceParams)]),
    "oslam_align_instances": (_i, [_vp, _vp, C.POINTER(InstanceParams), C.POINTER(RefineParams), _vp, _sz, C.POINTER(_sz),
                                   _vp]),
    "oslam_db_align_instances": (_i, [_vp, _vp, C.POINTER(InstanceParams), C.POINTER(RefineParams), _vp, _sz, _vp, _vp]),
    "oslam_select_instances": (_i, [_vp, _vp, _sz, _vp, _f, C.POINTER(InstanceParams), _vp, _sz, C.POINTER(_sz)]),
    "oslam_arbitrate_params_default": (_i, [C.POINTER(ArbitrateParams)]),
    "oslam_arbitrate": (_i, [_vp, _vp, _sz, _vp, C.POINTER(ArbitrateParams), _vp]),
    "oslam_db_arbitrate": (_i, [_vp, _vp, _vp, C.POINTER(ArbitrateParams), _vp]),
    "oslam_arbitrate_claims": (_i, [_vp, _vp, _sz, _vp, C.POINTER(ArbitrateParams), _vp, _vp, _sz, C.POINTER(C.c_uint32),
                                    C.POINTER(_sz)]),
    "oslam_arbitrate_table": (_i, [_vp, _vp, _vp, _sz, _sz, C.c_uint, _f, _vp, C.POINTER(C.c_uint32)]),
    "oslam_detect_params_default": (_i, [C.POINTER(DetectParams)]),
    "oslam_db_detect": (_i, [_vp, _vp, _vp, C.POINTER(DetectParams), _vp, _sz, C.POINTER(_sz)]),
    "oslam_track_params_default": (_i, [C.POINTER(TrackParams)]),
    "oslam_track": (_i, [_vp, _vp, _sz, _vp, C.POINTER(TrackParams), _vp, _vp]),
    "oslam_db_track": (_i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(TrackParams), _vp, _vp]),
    "oslam_view_normals": (_i, [_vp, _vp, _vp]),
    "oslam_view_vertices": (_i, [_vp, _vp]),
    "oslam_track_correspondences": (_i, [_vp, _vp, _vp, _f, _f, _vp]),
    "oslam_tracker_params_default": (_i, [C.POINTER(TrackerParams)]),
    "oslam_tracker_create": (_i, [_vp, C.POINTER(TrackerParams), C.POINTER(_vp)]),
    "oslam_tracker_create_shapes": (_i, [_vp, _vp, _sz, C.POINTER(TrackerParams), C.POINTER(_vp)]),
    "oslam_tracker_destroy": (None, [_vp]),
    "oslam_tracker_update": (_i, [_vp, _vp, _sz]),
    "oslam_tracker_tracks": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_tracker_step": (_i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_i)]),
    "oslam_egomotion_params_default": (_i, [C.POINTER(EgomotionParams)]),
    "oslam_view_egomotion": (_i, [_vp, _vp, _vp, C.POINTER(EgomotionParams), _vp, C.POINTER(EgomotionResult)]),
    "oslam_view_egomotion_correspondences": (_i, [_vp, _vp, _vp, C.POINTER(EgomotionParams), _vp]),
    "oslam_tracker_step_cam": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_i)]),
    "oslam_tracker_predict": (_i, [_vp, _vp]),
    "oslam_tracker_camera": (_i, [_vp, _vp]),
    "oslam_volume_params_default": (_i, [C.POINTER(VolumeParams)]),
    "oslam_volume_create": (_i, [C.POINTER(VolumeParams), _i, C.POINTER(_vp)]),
    "oslam_volume_destroy": (_i, [_vp]),
    "oslam_volume_reset": (_i, [_vp]),
    "oslam_volume_integrate": (_i, [_vp, _vp, _vp, C.POINTER(IntegrateResult)]),
    "oslam_volume_raycast": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(_vp), C.POINTER(RaycastResult)]),
    "oslam_volume_track": (_i, [_vp, _vp, _vp, C.POINTER(EgomotionParams), _vp, C.POINTER(EgomotionResult)]),
    "oslam_view_to_cloud": (_i, [_vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_volume_voxels": (_i, [_vp, _vp, _vp]),
    "oslam_view_maps": (_i, [_vp, _vp, _vp]),
    "oslam_pyramid_params_default": (_i, [C.POINTER(PyramidParams)]),
    "oslam_pyramid_create": (_i, [_vp, C.POINTER(PyramidParams), C.POINTER(_vp)]),
    "oslam_pyramid_destroy": (_i, [_vp]),
    "oslam_pyramid_level": (_i, [_vp, _u, C.POINTER(_vp)]),
    "oslam_pyramid_egomotion": (_i, [_vp, _vp, _vp, C.POINTER(EgomotionParams), _vp, C.POINTER(EgomotionResult)]),
    "oslam_volume_track_pyramid": (_i, [_vp, _vp, _vp, C.POINTER(PyramidParams), C.POINTER(EgomotionParams), _vp,
                                        C.POINTER(EgomotionResult)]),
    "oslam_render_params_default": (_i, [C.POINTER(RenderParams)]),
    "oslam_render_create": (_i, [_vp, _vp, _sz, _vp, _i, _i, C.POINTER(RenderParams), C.POINTER(_vp), _vp]),
    "oslam_db_render": (_i, [_vp, _vp, _vp, _sz, _vp, _i, _i, C.POINTER(RenderParams), C.POINTER(_vp), _vp]),
    "oslam_render_view": (_i, [_vp, C.POINTER(_vp)]),
    "oslam_explain_params_default": (_i, [C.POINTER(ExplainParams)]),
    "oslam_explain": (_i, [_vp, _vp, _sz, _vp, C.POINTER(ExplainParams), _vp]),
    "oslam_db_explain": (_i, [_vp, _vp, _vp, C.POINTER(ExplainParams), _vp]),
    "oslam_explain_rect": (_i, [_vp, C.c_double, _vp, _vp, _i, _i, C.c_uint, _vp]),
    "oslam_explain_z": (_i, [_vp, _vp, _sz, _vp, C.POINTER(ExplainParams), _sz, _vp]),
    "oslam_explain_claims": (_i, [_vp, _vp, _sz, _vp, C.POINTER(ExplainParams), _vp, _vp, _sz, C.POINTER(C.c_uint32),
                                  C.POINTER(_sz)]),
    "oslam_render_labels": (_i, [_vp, _vp]),
    "oslam_render_destroy": (_i, [_vp]),
    "oslam_view_info": (_i, [_vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "oslam_mask_params_default": (_i, [C.POINTER(MaskParams)]),
    "oslam_view_mask": (_i, [_vp, _vp, C.POINTER(MaskParams), C.POINTER(_vp), C.POINTER(MaskResult)]),
    "oslam_planes_params_default": (_i, [C.POINTER(PlanesParams)]),
    "oslam_view_planes": (_i, [_vp, C.POINTER(PlanesParams), C.POINTER(_vp), C.POINTER(PlanesResult)]),
    "oslam_planes_get": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_planes_labels": (_i, [_vp, _vp]),
    "oslam_planes_rounds": (_i, [_vp, _vp, _vp]),
    "oslam_view_remove_planes": (_i, [_vp, _vp, _i, C.c_int32, C.POINTER(_vp), C.POINTER(MaskResult)]),
    "oslam_planes_destroy": (_i, [_vp]),
    "oslam_segments_params_default": (_i, [C.POINTER(SegmentsParams)]),
    "oslam_view_segments": (_i, [_vp, _vp, C.POINTER(SegmentsParams), C.POINTER(_vp), C.POINTER(SegmentsResult)]),
    "oslam_segments_get": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_segments_labels": (_i, [_vp, _vp]),
    "oslam_segments_roots": (_i, [_vp, _vp]),
    "oslam_view_select_segments": (_i, [_vp, _vp, _i, C.c_int32, C.POINTER(_vp), C.POINTER(MaskResult)]),
    "oslam_segments_destroy": (_i, [_vp]),
    "oslam_bilateral_params_default": (_i, [C.POINTER(BilateralParams)]),
    "oslam_view_bilateral": (_i, [_vp, C.POINTER(BilateralParams), C.POINTER(_vp), C.POINTER(BilateralResult)]),
    "oslam_gauss_table": (_i, [_u, C.POINTER(_f)]),
    "oslam_surface_params_default": (_i, [C.POINTER(SurfaceParams)]),
    "oslam_volume_surface": (_i, [_vp, C.POINTER(SurfaceParams), _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(SurfaceResult)]),
    "oslam_scene_from_volume": (_i, [_vp, C.POINTER(SurfaceParams), _f, _f, _u, C.POINTER(Params), C.POINTER(_vp),
                                     C.POINTER(_sz)]),
    "oslam_volume_set_voxels": (_i, [_vp, _vp, _vp]),
    "oslam_volume_shift": (_i, [_vp, _vp, C.POINTER(ShiftResult)]),
    "oslam_volume_window": (_i, [_vp, _vp, _vp]),
    "oslam_volume_leaving": (_i, [_vp, _vp, C.POINTER(SurfaceParams), _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(SurfaceResult)]),
    "oslam_follow_params_default": (_i, [_vp, C.POINTER(FollowParams)]),
    "oslam_volume_follow": (_i, [_vp, _vp, C.POINTER(FollowParams), _vp]),
    "oslam_world_params_of": (_i, [_vp, C.POINTER(WorldParams)]),
    "oslam_world_create": (_i, [C.POINTER(WorldParams), C.POINTER(_vp)]),
    "oslam_world_destroy": (_i, [_vp]),
    "oslam_world_clear": (_i, [_vp]),
    "oslam_world_stats_get": (_i, [_vp, C.POINTER(WorldStats)]),
    "oslam_world_put": (_i, [_vp, _vp, _vp, _sz]),
    "oslam_world_box": (_i, [_vp, _vp, _vp, _vp, _i]),
    "oslam_world_has_colour": (_i, [_vp]),
    "oslam_world_put_colour": (_i, [_vp, _vp, _vp, _vp, _sz]),
    "oslam_world_box_colour": (_i, [_vp, _vp, _vp, _vp, _vp, _i]),
    "oslam_world_colours": (_i, [_vp, _vp, C.POINTER(WorldSurfaceParams), _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz)]),
    "oslam_world_surface_params_default": (_i, [C.POINTER(WorldSurfaceParams)]),
    "oslam_world_surface": (_i, [_vp, _vp, C.POINTER(WorldSurfaceParams), _vp, _vp, _vp, _sz, C.POINTER(_sz),
                                 C.POINTER(WorldSurfaceResult)]),
    "oslam_world_mesh": (_i, [_vp, _vp, C.POINTER(WorldSurfaceParams), _vp, _vp, _vp, _sz, _vp, _sz, C.POINTER(_sz),
                              C.POINTER(_sz), C.POINTER(WorldMeshResult)]),
    "oslam_world_bricks": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_world_raycast_params_default": (_i, [C.POINTER(WorldRaycastParams)]),
    "oslam_world_raycast": (_i, [_vp, _vp, C.POINTER(WorldRaycastParams), _vp, _vp, _i, _i, C.POINTER(_vp),
                                 C.POINTER(WorldRaycastResult)]),
    "oslam_world_track": (_i, [_vp, _vp, C.POINTER(WorldRaycastParams), _vp, _vp, C.POINTER(EgomotionParams), _vp,
                               C.POINTER(EgomotionResult)]),
    "oslam_world_paint_view": (_i, [_vp, _vp, C.POINTER(WorldSurfaceParams), _vp, _vp, C.POINTER(C.c_uint32)]),
    "oslam_scene_from_world": (_i, [_vp, _vp, C.POINTER(WorldSurfaceParams), _f, _f, _u, C.POINTER(Params), C.POINTER(_vp),
                                    C.POINTER(_sz)]),
    "oslam_volume_shift_world": (_i, [_vp, _vp, _vp, C.POINTER(ReloadResult)]),
    "oslam_volume_pack": (_i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_volume_pack_colour": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_mesh_params_default": (_i, [C.POINTER(MeshParams)]),
    "oslam_volume_mesh": (_i, [_vp, C.POINTER(MeshParams), _vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz),
                               C.POINTER(MeshResult)]),
    "oslam_ply_write_mesh": (_i, [C.c_char_p, _vp, _vp, _sz, _vp, _sz, _i]),
    "oslam_mc_table_row": (_i, [_u, _vp, C.POINTER(_u)]),
    "oslam_normals_params_default": (_i, [C.POINTER(NormalsParams)]),
    "oslam_cloud_normals": (_i, [_vp, _sz, _sz, C.POINTER(NormalsParams), _i, _vp, _vp, _vp, C.POINTER(NormalsResult)]),
    "oslam_cloud_normal_moments": (_i, [_vp, _sz, _sz, C.POINTER(NormalsParams), _i, _vp]),
    "oslam_mesh_normals": (_i, [_vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "oslam_ply_read_mesh": (_i, [C.c_char_p, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_sz)]),
    "oslam_view_set_colour": (_i, [_vp, _vp, _sz, _vp]),
    "oslam_view_colour": (_i, [_vp, _vp]),
    "oslam_view_has_colour": (_i, [_vp]),
    "oslam_colour_params_default": (_i, [C.POINTER(ColourParams)]),
    "oslam_volume_colour_enable": (_i, [_vp, C.POINTER(ColourParams)]),
    "oslam_volume_colour_words": (_i, [_vp, _vp]),
    "oslam_volume_set_colour_words": (_i, [_vp, _vp]),
    "oslam_volume_integrate_colour": (_i, [_vp, _vp, _vp, _vp, C.POINTER(IntegrateResult), C.POINTER(C.c_uint32)]),
    "oslam_volume_colours": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz)]),
    "oslam_volume_paint_view": (_i, [_vp, _vp, _vp, C.POINTER(C.c_uint32)]),
    "oslam_ply_write_colour": (_i, [C.c_char_p, _vp, _vp, _vp, _sz, _i]),
    "oslam_ply_write_mesh_colour": (_i, [C.c_char_p, _vp, _vp, _vp, _sz, _vp, _sz, _i]),
    "oslam_scene_keys": (_i, [_vp, _sz, _vp]),
    "oslam_model_keys": (_i, [_vp, _sz, _vp]),
    "oslam_model_bucket": (_i, [_vp, C.c_uint32, _vp, _sz, C.POINTER(_sz)]),
    "oslam_model_bucket_words": (_i, [_vp, C.c_uint32, _i, _vp, _sz, C.POINTER(_sz)]),
    "oslam_vote_accumulator": (_i, [_vp, _vp, _sz, _vp]),
    "oslam_vote_hits": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint32)]),
    "oslam_sort_hits_tap": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, C.c_uint32, _i, _vp, _vp, _vp, _vp, _vp]),
    "oslam_bucket_order_tap": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "oslam_model_tables_tap": (_i, [_vp, C.POINTER(ModelTables)] + [_vp] * 12),
    "oslam_model_key_numbers": (_i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_vote_ref_order": (_i, [_vp, _sz, _vp]),
    "oslam_last_cells": (_i, [_vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "oslam_tail_scores": (_i, [_vp, _vp, _vp, _sz, C.c_uint32, _i, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint32), _vp,
                               C.POINTER(_i)]),
    "oslam_set_stream": (_i, [_vp]),
    "oslam_last_error": (C.c_char_p, []),
    "oslam_set_host_threads": (_i, [_i]),
    "oslam_selftest_math": (_i, [_sz, C.c_uint64, C.POINTER(C.c_uint64)]),
}


def lib():
    """Load liboslam_hip.so (built in-tree by __graft_entry__.build()); raise if absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OslamError(OSLAM_E_DEVICE, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                             "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _check(rc):
    if rc != OSLAM_OK:
        raise OslamError(rc, lib().oslam_last_error().decode("utf-8", "replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# Fields every default_params() call starts from, on top of the library's defaults: how tests and tools steer
# library-wide switches (pose_gpu_min, scratch_gib ...) -- through oslam_params, not through the environment.
DEFAULT_OVERRIDES = {}


def default_params(**kw):
    p = Params()
    _check(lib().oslam_params_default(C.byref(p)))
    for k, v in {**DEFAULT_OVERRIDES, **kw}.items():
        if not hasattr(p, k):
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


def vote_ref_order(keep):
    """The order in which the vote grid takes a batch of reference points with the demands `keep` (host only)."""
    keep = np.ascontiguousarray(keep, np.uint32)
    out = np.zeros(len(keep), np.uint32)
    _check(lib().oslam_vote_ref_order(_p(keep), len(keep), _p(out)))
    return out


def sort_hits(numbers, theta, idx, offsets, counts, id_bits, dev=0):
    """k_sort_hits alone on the lists given (oslam_sort_hits_tap): list l owns the slots offsets[l] .. offsets[l + 1] and
    holds min(counts[l], its slots) hits.  -> (numbers, theta, idx, runs [slots, 2], run_counts), every array whole."""
    numbers, theta, idx, offsets, counts = (np.ascontiguousarray(a, np.uint32) for a in (numbers, theta, idx, offsets, counts))
    n_lists = len(counts)
    if len(offsets) != n_lists + 1:
        raise ValueError("offsets holds one word more than counts")
    total = int(offsets[-1])
    if not (len(numbers) == len(theta) == len(idx) == total):
        raise ValueError("numbers, theta and idx hold offsets[-1] words each")
    num_o, th_o, idx_o = (np.zeros(max(total, 1), np.uint32) for _ in range(3))
    runs, rc = np.zeros((max(total, 1), 2), np.uint32), np.zeros(max(n_lists, 1), np.uint32)
    _check(lib().oslam_sort_hits_tap(_p(numbers), _p(theta), _p(idx), _p(offsets), _p(counts), n_lists, int(id_bits), int(dev),
                                     _p(num_o), _p(th_o), _p(idx_o), _p(runs), _p(rc)))
    return num_o[:total], th_o[:total], idx_o[:total], runs[:total], rc[:n_lists]


def bucket_order(lens, e4, uv, mi, keys=None, with_uv=True, spread=True, dev=0):
    """k_bucket_spread and k_bucket_psort alone on the buckets given (oslam_bucket_order_tap): bucket b holds lens[b]
    entries from the running sum of (len + 3) & ~3 on, under the key keys[b] (None: b + 1).  e4 [total] uint32,
    uv [total, 2] float32, mi [total] uint16 with their padding.  -> (e4, uv, mi, pw, puv, pdir [total + 256]), whole."""
    lens = np.ascontiguousarray(lens, np.uint32)
    e4, uv, mi = np.ascontiguousarray(e4, np.uint32), np.ascontiguousarray(uv, np.float32), np.ascontiguousarray(mi, np.uint16)
    total = int((((lens.astype(np.int64) + 3) >> 2) << 2).sum())
    if keys is not None:
        keys = np.ascontiguousarray(keys, np.uint32)
        if len(keys) != len(lens):
            raise ValueError("keys holds one word per bucket")
    if e4.shape != (total,) or uv.shape != (total, 2) or mi.shape != (total,):
        raise ValueError("e4, uv and mi hold the padded lengths' sum of entries each")
    room = max(total, 1)
    e4_o, pw = np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    uv_o, puv = np.zeros((room, 2), np.float32), np.zeros((room, 2), np.float32)
    mi_o, pdir = np.zeros(room, np.uint16), np.zeros(total + 256, np.uint16)
    _check(lib().oslam_bucket_order_tap(_p(lens), None if keys is None else _p(keys), len(lens), _p(e4), _p(uv), _p(mi),
                                        int(bool(with_uv)), int(bool(spread)), int(dev), _p(e4_o), _p(uv_o), _p(mi_o),
                                        _p(pw), _p(puv), _p(pdir)))
    return e4_o[:total], uv_o[:total], mi_o[:total], pw[:total], puv[:total], pdir


def default_refine_params(**kw):
    """oslam_refine_params_default, then the fields given as keywords."""
    p = RefineParams()
    _check(lib().oslam_refine_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown refine parameter %r" % k)
        setattr(p, k, v)
    return p


def default_verify_params(**kw):
    """oslam_verify_params_default, then the fields given as keywords."""
    p = VerifyParams()
    _check(lib().oslam_verify_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown verify parameter %r" % k)
        setattr(p, k, v)
    return p


def default_instance_params(**kw):
    """oslam_instance_params_default, then the fields given as keywords."""
    p = InstanceParams()
    _check(lib().oslam_instance_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown instance parameter %r" % k)
        setattr(p, k, v)
    return p


def default_arbitrate_params(**kw):
    """oslam_arbitrate_params_default, then the fields given as keywords."""
    p = ArbitrateParams()
    _check(lib().oslam_arbitrate_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown arbitrate parameter %r" % k)
        setattr(p, k, v)
    return p


def default_detect_params():
    """oslam_detect_params_default: the defaults of every stage, as .instances / .refine / .verify / .arbitrate."""
    p = DetectParams()
    _check(lib().oslam_detect_params_default(C.byref(p)))
    return p


def default_track_params(**kw):
    """oslam_track_params_default, then the fields given as keywords (verify: a VerifyParams)."""
    p = TrackParams()
    _check(lib().oslam_track_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown track parameter %r" % k)
        setattr(p, k, v)
    return p


def default_tracker_params(**kw):
    """oslam_tracker_params_default, then the fields given as keywords (track / detect / arbitrate: their structures)."""
    p = TrackerParams()
    _check(lib().oslam_tracker_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown tracker parameter %r" % k)
        setattr(p, k, v)
    return p


def default_egomotion_params(**kw):
    """oslam_egomotion_params_default, then the fields given as keywords; levels=[(stride, max_iterations), ...] sets
    n_levels and level together."""
    p = EgomotionParams()
    _check(lib().oslam_egomotion_params_default(C.byref(p)))
    levels = kw.pop("levels", None)
    if levels is not None:
        levels = list(levels)
        if len(levels) > 3:
            raise ValueError("at most 3 levels")
        p.n_levels = len(levels)
        for k in range(3):
            p.level[k].stride, p.level[k].max_iterations = levels[k] if k < len(levels) else (0, 0)
    for k, v in kw.items():
        if not hasattr(p, k) or k in ("reserved", "level"):
            raise TypeError("unknown egomotion parameter %r" % k)
        setattr(p, k, v)
    return p


def egomotion(src_view, dst_view, T_init=None, params=None):
    """The camera's motion between two depth views by dense projective ICP (oslam_view_egomotion): -> (T float32 4x4,
    source camera coordinates -> destination camera coordinates; result dict).  T_init None: the identity."""
    p = params if params is not None else default_egomotion_params()
    To = np.zeros(16, np.float32)
    res = EgomotionResult()
    Ti = _pose16(T_init) if T_init is not None else None
    _check(lib().oslam_view_egomotion(src_view._h, dst_view._h, _p(Ti) if Ti is not None else None, C.byref(p), _p(To),
                                      C.byref(res)))
    return To.reshape(4, 4), res.asdict()


def egomotion_correspondences(src_view, dst_view, T, params=None):
    """Pixel v * width + u in dst of every source pixel's correspondence under T at stride 1, -1 = none
    (oslam_view_egomotion_correspondences: the rule of oslam_view_egomotion, as a test tap).  -> int32 [h, w] of src."""
    p = params if params is not None else default_egomotion_params()
    out = np.zeros(src_view.width * src_view.height, np.int32)
    _check(lib().oslam_view_egomotion_correspondences(src_view._h, dst_view._h, _p(_pose16(T)), C.byref(p), _p(out)))
    return out.reshape(src_view.height, src_view.width)


def _hypotheses(models, T):
    """-> (array of model handles, T [H,16] float32, H)"""
    models = list(models)
    H = len(models)
    Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(H, 16))
    return (C.c_void_p * max(H, 1))(*[m._h for m in models]), Ti, H


def arbitrate(models, view, T, params=None):
    """Arbitration between the hypotheses (models[h], T[h]) that claim the same pixels of the view's depth image
    (oslam_arbitrate); an all-zero T[h] is skipped.  -> (list of result dicts, kept bool [H])."""
    arr, Ti, H = _hypotheses(models, T)
    res = (ArbitrateResult * max(H, 1))()
    p = params if params is not None else default_arbitrate_params()
    _check(lib().oslam_arbitrate(arr, _p(Ti), H, view._h, C.byref(p), res))
    out = [res[h].asdict() for h in range(H)]
    return out, np.array([bool(r["kept"]) for r in out], dtype=bool)


def default_explain_params(**kw):
    """oslam_explain_params_default, then the fields given as keywords."""
    p = ExplainParams()
    _check(lib().oslam_explain_params_default(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(ExplainParams._fields_) or k == "reserved":
            raise TypeError("unknown explain parameter %r" % k)
        setattr(p, k, v)
    return p


def explain(models, view, T, params=None):
    """Every hypothesis (models[h], T[h]) judged against its own z-buffer in the view's camera and arbitrated by its
    conflict rate (oslam_explain); an all-zero T[h] is skipped.  -> list of result dicts."""
    arr, Ti, H = _hypotheses(models, T)
    res = (ExplainResult * max(H, 1))()
    p = params if params is not None else default_explain_params()
    _check(lib().oslam_explain(arr, _p(Ti), H, view._h, C.byref(p), res))
    return [res[h].asdict() for h in range(H)]


def explain_z(models, view, T, h, params=None):
    """The solo z image of hypothesis h as a test tap (oslam_explain_z): -> float32 [height, width], 0 = nothing drawn."""
    arr, Ti, H = _hypotheses(models, T)
    p = params if params is not None else default_explain_params()
    out = np.zeros((view.height, view.width), np.float32)
    _check(lib().oslam_explain_z(arr, _p(Ti), H, view._h, C.byref(p), int(h), _p(out)))
    return out


def explain_claims(models, view, T, params=None):
    """The claims table after k_explain_claims as a test tap (oslam_explain_claims): -> (cnt uint32 [H, n_tiles], sum
    uint64 [H, n_tiles], tile in pixels)."""
    arr, Ti, H = _hypotheses(models, T)
    p = params if params is not None else default_explain_params()
    n_tiles = ((view.width + 3) // 4) * ((view.height + 3) // 4)       # the smallest tile: the largest table
    cnt = np.zeros(max(H * n_tiles, 1), np.uint32)
    sm = np.zeros(max(H * n_tiles, 1), np.uint64)
    tile, nt = C.c_uint32(0), C.c_size_t(0)
    _check(lib().oslam_explain_claims(arr, _p(Ti), H, view._h, C.byref(p), _p(cnt), _p(sm), len(cnt), C.byref(tile),
                                      C.byref(nt)))
    n = H * nt.value
    return cnt[:n].reshape(H, nt.value).copy(), sm[:n].reshape(H, nt.value).copy(), int(tile.value)


def explain_rect(centre, radius, T, camera, width, height, max_splat=8):
    """The rectangle of the image that holds whatever a hypothesis can draw, on the host (oslam_explain_rect): centre
    [3] and radius of the model's bounding sphere in the model frame, T 4x4, camera a Camera.  -> (x0, y0, w, h)."""
    c = np.ascontiguousarray(centre, np.float64).reshape(3)
    Ti = _pose16(T)
    out = np.zeros(4, np.int32)
    _check(lib().oslam_explain_rect(_p(c), float(radius), _p(Ti), C.byref(camera), int(width), int(height), int(max_splat),
                                    _p(out)))
    return tuple(int(x) for x in out)


def _track_out(To, res, H):
    out = [res[h].asdict() for h in range(H)]
    return To.reshape(H, 4, 4), out, np.array([bool(r["found"]) for r in out], dtype=bool)


def track(models, view, T, params=None):
    """The hypotheses (models[h], T[h]) followed into the view's depth image by projective ICP and judged there
    (oslam_track); an all-zero T[h] is skipped.  -> (T [H,4,4], list of result dicts, found bool [H])."""
    arr, Ti, H = _hypotheses(models, T)
    To = np.zeros((max(H, 1), 16), np.float32)
    res = (TrackResult * max(H, 1))()
    p = params if params is not None else default_track_params()
    _check(lib().oslam_track(arr, _p(Ti), H, view._h, C.byref(p), _p(To), res))
    return _track_out(To[:H], res, H)


def track_correspondences(model, view, T, max_corr_dist=2.0, min_normal_dot=0.8):
    """Pixel v * width + u of every model point's correspondence under T, -1 = none (oslam_track_correspondences: the
    rule of oslam_track, as a test tap)."""
    out = np.zeros(model.n, np.int32)
    _check(lib().oslam_track_correspondences(model._h, view._h, _p(_pose16(T)), float(max_corr_dist), float(min_normal_dot),
                                             _p(out)))
    return out


def view_normals(view):
    """The view's vertex and normal maps as a test tap (oslam_view_vertices / oslam_view_normals): -> (vertices [h,w,3],
    normals [h,w,3], has_normal bool [h,w])."""
    n = view.width * view.height
    vtx, nrm, has = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    _check(lib().oslam_view_normals(view._h, _p(nrm), _p(has)))
    _check(lib().oslam_view_vertices(view._h, _p(vtx)))
    shape = (view.height, view.width)
    return vtx.reshape(shape + (3,)), nrm.reshape(shape + (3,)), has.reshape(shape).astype(bool)


class Tracker:
    """Identity across depth frames (oslam_tracker): Tracker(db, params).step(view, scene=None) follows every live track
    into the frame and, when a scene is given and a search is due, runs db.detect and folds its detections in;
    .update(detections) is that last step alone (host only).  Tracker.from_shapes(centroids, extents) makes one without
    a database, for update() on a machine without a device."""

    def __init__(self, db, params=None, _shapes=None):
        self._h = C.c_void_p(0)
        self.db = db
        self.params = params if params is not None else default_tracker_params()
        if _shapes is None:
            _check(lib().oslam_tracker_create(db._h, C.byref(self.params), C.byref(self._h)))
        else:
            c, e = _shapes
            _check(lib().oslam_tracker_create_shapes(_p(c), _p(e), len(e), C.byref(self.params), C.byref(self._h)))

    @classmethod
    def from_shapes(cls, centroids, extents, params=None):
        c = np.ascontiguousarray(np.asarray(centroids, np.float32).reshape(-1, 3))
        e = np.ascontiguousarray(extents, np.float32).reshape(-1)
        if len(c) != len(e):
            raise ValueError("centroids and extents differ in length")
        return cls(None, params, _shapes=(c, e))

    def tracks(self):
        """The live tracks ordered by id, as dicts (id, model, T 4x4, age, hits, misses, found, track)."""
        n = C.c_size_t(0)
        rc = lib().oslam_tracker_tracks(self._h, None, 0, C.byref(n))
        if rc not in (OSLAM_OK, OSLAM_E_LIMIT):
            _check(rc)
        out = (TrackState * max(n.value, 1))()
        _check(lib().oslam_tracker_tracks(self._h, out, max(n.value, 1), C.byref(n)))
        return [out[k].asdict() for k in range(n.value)]

    def update(self, detections):
        """Fold a detection list (dicts with model and T, as Database.detect returns them) into the tracks."""
        det = (Detection * max(len(detections), 1))()
        for k, d in enumerate(detections):
            det[k].model = int(d["model"])
            det[k].instance = int(d.get("instance", 0))
            det[k].T[:] = [float(x) for x in np.asarray(d["T"], np.float32).reshape(16)]
        _check(lib().oslam_tracker_update(self._h, det, len(detections)))
        return self.tracks()

    def step(self, view, scene=None, T_cam=None):
        """One frame.  T_cam: the camera's motion from the previous frame to this one (egomotion(previous, view)), moved
        into every live track before it is followed; None: none.  -> (live tracks as dicts, searched bool)."""
        cap = ARBITRATE_MAX_HYPOTHESES + max(1, len(self.db.models)) * MAX_INSTANCES
        out = (TrackState * cap)()
        n, searched = C.c_size_t(0), C.c_int(0)
        sc = scene._h if scene is not None else None
        if T_cam is None:
            _check(lib().oslam_tracker_step(self._h, sc, view._h, out, cap, C.byref(n), C.byref(searched)))
        else:
            _check(lib().oslam_tracker_step_cam(self._h, sc, view._h, _p(_pose16(T_cam)), out, cap, C.byref(n),
                                                C.byref(searched)))
        return [out[k].asdict() for k in range(n.value)], bool(searched.value)

    def render(self, view, found_only=True, params=None):
        """The live tracks rendered into view's camera (render: hypothesis k is the k-th track taken, in id order).
        found_only: only the tracks the last step found.  -> a Render, or None when there is no such track."""
        if self.db is None:
            raise ValueError("a tracker made from shapes has no models to render")
        live = [t for t in self.tracks() if t["found"] or not found_only]
        if not live:
            return None
        return self.db.render(view, [t["model"] for t in live], np.stack([t["T"] for t in live]), params)

    def predict(self, T_cam):
        """Step 0 of step(T_cam=...) alone, on the host (oslam_tracker_predict).  -> the live tracks."""
        _check(lib().oslam_tracker_predict(self._h, _p(_pose16(T_cam))))
        return self.tracks()

    def camera(self):
        """The camera's accumulated pose in the frame of the first step's camera (oslam_tracker_camera), float32 4x4."""
        T = np.zeros(16, np.float32)
        _check(lib().oslam_tracker_camera(self._h, _p(T)))
        return T.reshape(4, 4)

    def close(self):
        if self._h:
            lib().oslam_tracker_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def arbitrate_claims(models, view, T, params=None):
    """The claims table after k_claim as a test tap (oslam_arbitrate_claims): -> (cnt uint32 [H, n_tiles], sum uint64
    [H, n_tiles], tile in pixels)."""
    arr, Ti, H = _hypotheses(models, T)
    p = params if params is not None else default_arbitrate_params()
    n_tiles = ((view.width + 3) // 4) * ((view.height + 3) // 4)       # the smallest tile: the largest table
    cnt = np.zeros(max(H * n_tiles, 1), np.uint32)
    sm = np.zeros(max(H * n_tiles, 1), np.uint64)
    tile, nt = C.c_uint32(0), C.c_size_t(0)
    _check(lib().oslam_arbitrate_claims(arr, _p(Ti), H, view._h, C.byref(p), _p(cnt), _p(sm), len(cnt), C.byref(tile),
                                        C.byref(nt)))
    n = H * nt.value
    return cnt[:n].reshape(H, nt.value).copy(), sm[:n].reshape(H, nt.value).copy(), int(tile.value)


def arbitrate_table(cnt, sm, skipped=None, min_tiles=4, min_owned_share=0.52):
    """The elimination alone over a given claims table as a test tap (oslam_arbitrate_table): cnt [H, n_tiles] (below
    2^24), sm [H, n_tiles] (below 2^40), skipped bool [H].  -> (list of result dicts, rounds)."""
    c = np.ascontiguousarray(cnt, np.uint32)
    s = np.ascontiguousarray(sm, np.uint64)
    if c.ndim != 2 or s.shape != c.shape:
        raise ValueError("cnt and sm must both be [H, n_tiles]")
    H, n_tiles = c.shape
    k = np.zeros(max(H, 1), np.uint8) if skipped is None else np.ascontiguousarray(np.asarray(skipped, bool), np.uint8)
    if skipped is not None and k.shape != (H,):
        raise ValueError("skipped must be [H]")
    res = (ArbitrateResult * max(H, 1))()
    rounds = C.c_uint32(0)
    _check(lib().oslam_arbitrate_table(_p(c) if c.size else None, _p(s) if s.size else None, _p(k), H, n_tiles, int(min_tiles),
                                       float(min_owned_share), res, C.byref(rounds)))
    return [res[h].asdict() for h in range(H)], int(rounds.value)


def _instance_args(refine, params, refine_params):
    ip = params if params is not None else default_instance_params()
    rp = None
    if refine:
        rp = refine_params if refine_params is not None else default_refine_params()
    return ip, rp


def select_instances(T, scores, centroid, extent, params=None, cap=None):
    """The host selection rule alone (oslam_select_instances, no GPU): T [n,4,4] and scores [n] indexed by candidate;
    -> accepted candidate indices in acceptance order (uint32 array).  Raises OslamError on invalid arguments."""
    ip = params if params is not None else default_instance_params()
    Ta = np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1, 16))
    sc = np.ascontiguousarray(scores, np.float32).reshape(-1)
    if len(sc) != len(Ta):
        raise ValueError("T and scores differ in length")
    c = np.ascontiguousarray(centroid, np.float32).reshape(3)
    cap = int(ip.max_instances) if cap is None else int(cap)
    idx = np.zeros(max(cap, 1), np.uint32)
    n = C.c_size_t(0)
    rc = lib().oslam_select_instances(_p(Ta) if len(Ta) else None, _p(sc) if len(sc) else None, len(sc), _p(c),
                                      float(extent), C.byref(ip), _p(idx), cap, C.byref(n))
    if rc != OSLAM_OK:
        raise OslamError(rc, "instance selection rejected its arguments" if rc == OSLAM_E_INVALID else "instance selection failed")
    return idx[: n.value].copy()


def _pose16(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))


def _cloud_args(points, normals=None):
    """-> (xyz pointer holder, nrm pointer, n, stride, keepalive array(s))"""
    pts = np.asarray(points)
    if normals is None:
        a = np.ascontiguousarray(pts, np.float32)
        if a.ndim != 2 or a.shape[1] != 12:
            raise ValueError("a single cloud array must be [n,12] float32 (pcl::PointNormal layout)")
        base = a.ctypes.data
        return C.c_void_p(base), C.c_void_p(base + 16), len(a), 48, (a,)
    p = np.ascontiguousarray(pts, np.float32)
    n = np.ascontiguousarray(normals, np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or n.shape != p.shape:
        raise ValueError("points and normals must both be [n,3]")
    return _p(p), _p(n), len(p), 12, (p, n)


def d_dist_from_cloud(points, tau_d):
    """d_dist = tau_d * max bbox extent (alignment.cpp:246-253)."""
    p = np.ascontiguousarray(points, np.float32)
    out = C.c_float(0)
    _check(lib().oslam_d_dist_from_cloud(_p(p), len(p), p.strides[0], float(tau_d), C.byref(out)))
    return out.value


def default_normals_params(**kw):
    """oslam_normals_params_default, then the fields given as keywords (viewpoint: three numbers)."""
    p = NormalsParams()
    _check(lib().oslam_normals_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown normals parameter %r" % k)
        setattr(p, k, (C.c_float * 3)(*[float(x) for x in v]) if k == "viewpoint" else v)
    return p


def _normals_cloud(points):
    """-> (array kept alive, n, stride): a packed [n,3] float32 array, or [n,12] (pcl::PointNormal) with stride 48"""
    a = np.ascontiguousarray(points, np.float32)
    if a.ndim != 2 or a.shape[1] not in (3, 12):
        raise ValueError("points must be [n,3] or [n,12] float32")
    return a, len(a), a.strides[0]


def estimate_normals(points, radius, viewpoint=(0, 0, 0), dev=0, want=("curvature", "valid"), result=None, **fields):
    """Normals of a cloud seen from `viewpoint`, from the principal axes of the neighbours within `radius`
    (oslam_cloud_normals) -> (normals [n,3] f32, curvature [n] f32, valid [n] bool).  fields: min_neighbours, orient,
    line_ratio.  want: which of the optional outputs the library is asked for (the others come back as None); result: a
    dict that receives oslam_normals_result."""
    a, n, stride = _normals_cloud(points)
    p = default_normals_params(radius=float(radius), viewpoint=viewpoint, **fields)
    nrm = np.zeros((n, 3), np.float32)
    curv = np.zeros(n, np.float32) if "curvature" in want else None
    valid = np.zeros(n, np.uint8) if "valid" in want else None
    res = NormalsResult()
    _check(lib().oslam_cloud_normals(_p(a), n, stride, C.byref(p), int(dev), _p(nrm), None if curv is None else _p(curv),
                                     None if valid is None else _p(valid), C.byref(res)))
    if result is not None:
        result.update(res.asdict())
    return nrm, curv, None if valid is None else valid.astype(bool)


def normal_moments(points, radius, dev=0, **fields):
    """The ten int64 moments per point that estimate_normals forms its covariance from (test tap) -> [n,10]."""
    a, n, stride = _normals_cloud(points)
    p = default_normals_params(radius=float(radius), **fields)
    out = np.zeros((n, 10), np.int64)
    _check(lib().oslam_cloud_normal_moments(_p(a), n, stride, C.byref(p), int(dev), _p(out)))
    return out


def mesh_normals(points, triangles):
    """Area-weighted vertex normals of a triangle mesh (oslam_mesh_normals, host) -> (normals [nv,3] f32, valid [nv] bool)."""
    a, n, stride = _normals_cloud(points)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    nrm, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    _check(lib().oslam_mesh_normals(_p(a), n, stride, _p(t), len(t), _p(nrm), _p(valid)))
    return nrm, valid.astype(bool)


class Scene:
    """Scene(cloud, d_dist, ref_point_downsample_factor=1)  (scene.h:15-16)."""

    @classmethod
    def from_points(cls, points, radius, viewpoint=(0, 0, 0), d_dist=None, ref_point_downsample_factor=1, params=None,
                    dev=0, **fields):
        """A scene from points alone: estimate_normals, drop the points without a valid normal, then Scene(...)."""
        pts = np.ascontiguousarray(points, np.float32)
        nrm, _, valid = estimate_normals(pts, radius, viewpoint, dev=dev, want=("valid",), **fields)
        return cls(pts[valid], nrm[valid], d_dist=d_dist, ref_point_downsample_factor=ref_point_downsample_factor,
                   params=params)

    def __init__(self, points, normals=None, d_dist=None, ref_point_downsample_factor=1, params=None):
        if d_dist is None:
            raise TypeError("d_dist is required")
        self._h = C.c_void_p(0)
        xyz, nrm, n, stride, keep = _cloud_args(points, normals)
        self.params = params if params is not None else default_params()
        self.d_dist = float(d_dist)
        self.df = int(ref_point_downsample_factor)
        self.n = n
        _check(lib().oslam_scene_create(xyz, nrm, n, stride, self.d_dist, self.df, C.byref(self.params), C.byref(self._h)))

    @classmethod
    def from_depth(cls, depth, fx, fy, cx, cy, leaf, d_dist=0.0, ref_point_downsample_factor=1, depth_scale=0.001,
                   z_min=0.1, z_max=10.0, max_jump=0.05, params=None):
        """Depth frame -> points + normals -> voxel grid -> Scene in one call, the full-resolution cloud
        staying in HBM (oslam_scene_from_depth)."""
        d = np.ascontiguousarray(depth)
        if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
            raise ValueError("depth must be a 2-D uint16 or float32 image")
        self = cls.__new__(cls)
        self._h = C.c_void_p(0)
        self.params = params if params is not None else default_params()
        self.d_dist, self.df = float(d_dist), int(ref_point_downsample_factor)
        cam = Camera(fx, fy, cx, cy, depth_scale, z_min, z_max, max_jump)
        n = C.c_size_t(0)
        _check(lib().oslam_scene_from_depth(_p(d), int(d.dtype == np.uint16), d.shape[1], d.shape[0], C.byref(cam),
                                            float(leaf), self.d_dist, self.df, C.byref(self.params), C.byref(self._h),
                                            C.byref(n)))
        self.n = n.value
        return self

    @classmethod
    def from_volume(cls, vol, leaf, d_dist=0.0, ref_point_downsample_factor=1, min_weight=1, params=None):
        """The fused surface of a Volume -> voxel grid (leaf > 0) -> Scene in one call, the extracted cloud staying in
        HBM (oslam_scene_from_volume).  The scene is in the volume frame and on the volume's device."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(0)
        self.params = params if params is not None else default_params()
        self.d_dist, self.df = float(d_dist), int(ref_point_downsample_factor)
        sp = default_surface_params(min_weight=min_weight)
        n = C.c_size_t(0)
        _check(lib().oslam_scene_from_volume(vol._h, C.byref(sp), float(leaf), self.d_dist, self.df, C.byref(self.params),
                                             C.byref(self._h), C.byref(n)))
        self.n = n.value
        return self

    @classmethod
    def from_world(cls, world, vol=None, leaf=0.0, d_dist=0.0, ref_point_downsample_factor=1, min_weight=1, anchor=None, dev=0,
                   params=None):
        """The surface of the whole map, the voxel store `world` plus the window of `vol` (None: the store alone, on
        device dev) -> voxel grid (leaf > 0) -> Scene in one call, the extracted cloud staying in HBM
        (oslam_scene_from_world).  The scene is in the volume frame."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(0)
        self.params = params if params is not None else default_params()
        self.d_dist, self.df = float(d_dist), int(ref_point_downsample_factor)
        sp = _world_surface_params(min_weight, anchor, dev)
        n = C.c_size_t(0)
        _check(lib().oslam_scene_from_world(world._h, vol._h if vol is not None else None, C.byref(sp), float(leaf), self.d_dist,
                                            self.df, C.byref(self.params), C.byref(self._h), C.byref(n)))
        self.n = n.value
        return self

    @classmethod
    def from_view(cls, view, planes=None, leaf=None, d_dist=None, ref_point_downsample_factor=1, params=None, dev=0,
                  segments=None, only=-1):
        """The view's pixels that have a normal as a scene: remove_planes (planes: a Planes of this view, None = keep
        everything), view_to_cloud, a voxel_grid when leaf is given, then Scene(...).  With segments (a Segments of this
        view) the scene is that of select_segments(view, segments, "keep", only); the planes then went into
        find_segments, and giving both is a TypeError."""
        if segments is not None and planes is not None:
            raise TypeError("give planes or segments, not both: the planes went into find_segments")
        if segments is not None:
            reduced = select_segments(view, segments, "keep", only)
        else:
            reduced = remove_planes(view, planes) if planes is not None else None
        try:
            pts, nrm = view_to_cloud(reduced if reduced is not None else view)
        finally:
            if reduced is not None:
                reduced.close()
        if leaf:
            pts, nrm = voxel_grid(pts, nrm, leaf=leaf, dev=dev)
        return cls(pts, nrm, d_dist=d_dist, ref_point_downsample_factor=ref_point_downsample_factor, params=params)

    def numPoints(self):
        return self.n

    def getHashKeys(self, ref_index):
        """Row `ref_index` of the reference's N x N hashKeys array (scene.cu:49-54)."""
        out = np.zeros(self.n, np.uint32)
        _check(lib().oslam_scene_keys(self._h, int(ref_index), _p(out)))
        return out

    def close(self):
        if self._h:
            lib().oslam_scene_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """Model(cloud, d_dist, vote_count_threshold, cpu_clustering, use_l1_norm,
    use_averaged_clusters)  (model.h:17-19); results appear in the same fields
    after ppf_lookup: transformations, vote_counts, max_idx / best_T."""

    def __init__(self, points, normals=None, d_dist=None, vote_count_threshold=0.4, cpu_clustering=False,
                 use_l1_norm=False, use_averaged_clusters=False, params=None):
        if d_dist is None:
            raise TypeError("d_dist is required")
        self._h = C.c_void_p(0)
        xyz, nrm, n, stride, keep = _cloud_args(points, normals)
        self.params = params if params is not None else default_params()
        self.params.vote_count_threshold = float(vote_count_threshold)
        self.params.cpu_clustering = int(cpu_clustering)
        self.params.use_l1_norm = int(use_l1_norm)
        self.params.use_averaged_clusters = int(use_averaged_clusters)
        self.d_dist = float(d_dist)
        self.n = n
        self.best_T = None
        self.stats = None
        _check(lib().oslam_model_create(xyz, nrm, n, stride, self.d_dist, C.byref(self.params), C.byref(self._h)))

    @classmethod
    def from_mesh(cls, points, triangles, d_dist=None, **kw):
        """A model from a triangle mesh: mesh_normals, drop the vertices without a normal, then Model(...)."""
        pts = np.ascontiguousarray(points, np.float32)
        nrm, valid = mesh_normals(pts, triangles)
        return cls(pts[valid], nrm[valid], d_dist=d_dist, **kw)

    def numPoints(self):
        return self.n

    # -- persistent model database (ppf.cu:64-66 asks for it; the reference rebuilds per pair) --
    def save(self, path):
        """Write the built table to `path` (oslam_model_save)."""
        _check(lib().oslam_model_save(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, path, params=None):
        """A model whose table comes from a file written by save(): nothing is recomputed."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(0)
        self.params = params if params is not None else default_params()
        self.best_T = None
        self.stats = None
        _check(lib().oslam_model_load(os.fsencode(path), C.byref(self.params) if params is not None else None,
                                      C.byref(self._h)))
        n, d = C.c_size_t(0), C.c_float(0)
        _check(lib().oslam_model_info(self._h, C.byref(n), C.byref(d), None))
        self.n, self.d_dist = n.value, d.value
        return self

    def table_bytes(self):
        b = C.c_uint64(0)
        _check(lib().oslam_model_info(self._h, None, None, C.byref(b)))
        return int(b.value)

    def SetModelPointVoteWeights(self, weights):
        w = np.ascontiguousarray(weights, np.float32)
        _check(lib().oslam_model_set_point_weights(self._h, _p(w), len(w)))

    def prepare(self, scene):
        """Allocate what the first ppf_lookup of this pair would (device scratch pool, pose-tail tables)."""
        _check(lib().oslam_align_prepare(self._h, scene._h))

    def ppf_lookup(self, scene, allow_no_votes=False):
        """Model::ppf_lookup (model.cu:269-306) + extraction (ppf.cu:74-93)."""
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = lib().oslam_align(self._h, scene._h, _p(T), C.byref(st))
        if not (allow_no_votes and rc == OSLAM_E_NO_VOTES):
            _check(rc)
        self.best_T = T.reshape(4, 4)
        self.stats = st.asdict()
        return self.best_T

    def refine(self, scene, T=None, params=None):
        """Point-to-plane ICP of the pose T (default: best_T of the last ppf_lookup) against the scene, and its presence
        score (oslam_refine).  -> (refined T 4x4, result dict: fitness_in, fitness, rmse, inliers, iterations, found ...)."""
        if T is None:
            T = self.best_T
        if T is None:
            raise ValueError("no pose: run ppf_lookup first or pass T")
        Ti = _pose16(T)
        To = np.zeros(16, np.float32)
        r = RefineResult()
        p = params if params is not None else default_refine_params()
        _check(lib().oslam_refine(self._h, scene._h, _p(Ti), C.byref(p), _p(To), C.byref(r)))
        return To.reshape(4, 4), r.asdict()

    def verify(self, view, T, params=None):
        """The pose T checked against the depth image of `view` (oslam_verify): -> result dict (the six class counts,
        view_fitness, coverage, found, launches, ms_total)."""
        r = VerifyResult()
        p = params if params is not None else default_verify_params()
        _check(lib().oslam_verify(self._h, view._h, _p(_pose16(T)), C.byref(p), C.byref(r)))
        return r.asdict()

    def find_instances(self, scene, refine=True, params=None, refine_params=None):
        """Every instance of the model in the scene (oslam_align_instances): -> list of (T 4x4, info dict) in
        acceptance order; info: T_vote, score, candidate, refine (zeros without refinement).  Instance 0's T_vote is
        the pose ppf_lookup returns; an empty list when nothing matched."""
        ip, rp = _instance_args(refine, params, refine_params)
        cap = int(ip.max_instances)
        out = (Instance * max(cap, 1))()
        n = C.c_size_t(0)
        st = Stats()
        rc = lib().oslam_align_instances(self._h, scene._h, C.byref(ip), C.byref(rp) if rp is not None else None, out,
                                         cap, C.byref(n), C.byref(st))
        if rc != OSLAM_E_NO_VOTES:
            _check(rc)
        self.stats = st.asdict()
        return [out[k].astuple() for k in range(n.value)]

    def align_local(self, scene, cap=None):
        """This rank's votes.  cap=None: returns (number of peaks above the LOCAL threshold, local maximum) and
        leaves the records with the model for local_peaks(); with a cap: (records, local maximum), and
        OSLAM_E_LIMIT is raised when they do not fit (nothing is cut silently)."""
        n = C.c_size_t(0)
        lmax = C.c_uint32(0)
        st = Stats()
        if cap is None:
            _check(lib().oslam_align_local(self._h, scene._h, None, 0, C.byref(n), C.byref(lmax), C.byref(st)))
            self.stats = st.asdict()
            return int(n.value), int(lmax.value)
        cells = np.zeros(cap, CELL_DTYPE)
        _check(lib().oslam_align_local(self._h, scene._h, _p(cells), cap, C.byref(n), C.byref(lmax), C.byref(st)))
        self.stats = st.asdict()
        return cells[: n.value].copy(), int(lmax.value)

    def local_peaks(self, global_max):
        """Records of the last align_local above threshold * global_max (oslam_local_peaks)."""
        n = C.c_size_t(0)
        rc = lib().oslam_local_peaks(self._h, int(global_max), None, 0, C.byref(n))
        if rc not in (OSLAM_OK, OSLAM_E_LIMIT):
            _check(rc)
        cells = np.zeros(max(n.value, 1), CELL_DTYPE)
        _check(lib().oslam_local_peaks(self._h, int(global_max), _p(cells), len(cells), C.byref(n)))
        return cells[: n.value].copy()

    def align_multi(self, scene, comm, allow_no_votes=False):
        """One call per rank: votes of this rank's shard, RCCL exchange, pose tail on the union (oslam_align_multi)."""
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = lib().oslam_align_multi(self._h, scene._h, comm._h, _p(T), C.byref(st))
        if not (allow_no_votes and rc == OSLAM_E_NO_VOTES):
            _check(rc)
        self.best_T = T.reshape(4, 4)
        self.stats = st.asdict()
        return self.best_T

    def align_finish(self, scene, cells, global_max, allow_no_votes=False):
        cells = np.ascontiguousarray(cells, CELL_DTYPE)
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = lib().oslam_align_finish(self._h, scene._h, _p(cells), len(cells), int(global_max), _p(T), C.byref(st))
        if not (allow_no_votes and rc == OSLAM_E_NO_VOTES):
            _check(rc)
        self.best_T = T.reshape(4, 4)
        if self.stats is not None:                      # the local counters stay; the union's tail adds its own
            self.stats["num_top"], self.stats["max_count"] = st.num_top, st.max_count
        return self.best_T

    # -- result fields of the reference's Model (model.h:92-113) --
    def last_cells(self):
        n = C.c_size_t(0)
        _check(lib().oslam_last_cells(self._h, None, None, 0, C.byref(n)))
        cells = np.zeros(n.value, CELL_DTYPE)
        poses = np.zeros((n.value, 16), np.float32)
        if n.value:
            _check(lib().oslam_last_cells(self._h, _p(cells), _p(poses), n.value, C.byref(n)))
        return cells, poses

    @property
    def transformations(self):
        return self.last_cells()[1]

    def last_result(self, scene):
        """(transformation_trans [n,3], transformation_rots [n,4] wxyz, vote_counts_out [n], max_idx) of the last
        ppf_lookup against `scene` (model.h:100-113)."""
        n = C.c_size_t(0)
        _check(lib().oslam_last_cells(self._h, None, None, 0, C.byref(n)))
        k = max(n.value, 1)
        tr, ro, sc = np.zeros((k, 3), np.float32), np.zeros((k, 4), np.float32), np.zeros(k, np.float32)
        best = C.c_uint32(0)
        _check(lib().oslam_last_result(self._h, scene._h, _p(tr), _p(ro), _p(sc), k, C.byref(n), C.byref(best)))
        return tr[: n.value], ro[: n.value], sc[: n.value], int(best.value)

    def tail_scores(self, scene, cells, global_max, path):
        """The peak records through a named pose tail (oslam_tail_scores; path 0: host loop, 1: host tail with the scores
        from the device kernel, 2: device tail): -> (kept cells in order, the score of each as that tail computed it,
        the winner's index, its T 4x4, the tail that really ran)."""
        cells = np.ascontiguousarray(cells, CELL_DTYPE)
        k = max(len(cells), 1)
        kept, sc, T = np.zeros(k, CELL_DTYPE), np.zeros(k, np.float32), np.zeros(16, np.float32)
        n, best, ran = C.c_size_t(0), C.c_uint32(0), C.c_int(-1)
        _check(lib().oslam_tail_scores(self._h, scene._h, _p(cells), len(cells), int(global_max), int(path), _p(kept), _p(sc), k,
                                       C.byref(n), C.byref(best), _p(T), C.byref(ran)))
        return kept[: n.value].copy(), sc[: n.value].copy(), int(best.value), T.reshape(4, 4), int(ran.value)

    def getHashKeys(self, ref_index):
        out = np.zeros(self.n, np.uint32)
        _check(lib().oslam_model_keys(self._h, int(ref_index), _p(out)))
        return out

    def bucket(self, key, cap=1 << 20):
        """Flat pair indices m_r*M + m_i stored under `key` (ParallelHashArray lookup)."""
        out = np.zeros(cap, np.uint32)
        n = C.c_size_t(0)
        _check(lib().oslam_model_bucket(self._h, int(key), _p(out), cap, C.byref(n)))
        return out[: min(n.value, cap)].copy(), n.value

    def bucket_words(self, key, slice_index=0, cap=1 << 20):
        """Stored entry words of `key`'s bucket in one slice, in storage order."""
        out = np.zeros(cap, np.uint32)
        n = C.c_size_t(0)
        _check(lib().oslam_model_bucket_words(self._h, int(key), int(slice_index), _p(out), cap, C.byref(n)))
        return out[: min(n.value, cap)].copy()

    def key_numbers(self):
        """(keys, numbers, weights) of every key of the model's table (its group's inside a database), by ascending key:
        the number the hit lists carry for the key, and the entries in its buckets that the number is ranked by."""
        n = C.c_size_t(0)
        _check(lib().oslam_model_key_numbers(self._h, None, None, None, 0, C.byref(n)))
        keys, nums, w = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().oslam_model_key_numbers(self._h, _p(keys), _p(nums), _p(w), n.value, C.byref(n)))
        return keys, nums, w

    def tables(self):
        """The model's tables as they lie in device memory (oslam_model_tables_tap): a dict of the scalars and of slots
        [n_slices, cap, 4], ukeys, uids, weights [ucap], reach [512], kmap [kmap_bins, 4913], uinfo [n_slices, stride, 2],
        e4 [n_entries + 256], mi [n_entries] and, when has_pw, pw, puv [n_entries, 2] (float32), pdir [n_entries + 256]."""
        info = ModelTables()
        _check(lib().oslam_model_tables_tap(self._h, C.byref(info), *([None] * 12)))
        t = info.asdict()
        ne = t["n_entries"]
        a = dict(slots=np.zeros((t["n_slices"], t["cap"], 4), np.uint32), ukeys=np.zeros(t["ucap"], np.uint32),
                 uids=np.zeros(t["ucap"], np.uint32), weights=np.zeros(t["ucap"], np.uint64), reach=np.zeros(512, np.uint32),
                 kmap=np.zeros((t["kmap_bins"], 4913), np.uint32), uinfo=np.zeros((t["n_slices"], t["uinfo_stride"], 2), np.uint32),
                 e4=np.zeros(ne + 256, np.uint32), mi=np.zeros(ne, np.uint16))
        if t["has_pw"]:
            a.update(pw=np.zeros(ne, np.uint32), puv=np.zeros((ne, 2), np.float32), pdir=np.zeros(ne + 256, np.uint16))
        order = ("slots", "ukeys", "uids", "weights", "reach", "kmap", "uinfo", "e4", "mi", "pw", "puv", "pdir")
        _check(lib().oslam_model_tables_tap(self._h, C.byref(info), *[_p(a[k]) if k in a and a[k].size else None for k in order]))
        t.update(a)
        return t

    def vote_accumulator(self, scene, ref_index):
        acc = np.zeros((self.n, 32), np.uint32)
        _check(lib().oslam_vote_accumulator(self._h, scene._h, int(ref_index), _p(acc)))
        return acc

    def vote_hits(self, scene, ref_index):
        """(numbers, theta_v, scene indices, keep) of one scene reference point: its hit list as the votes read it,
        sorted by key number (segment by segment above 16384 hits, or 8192 from 2^18 key numbers on), and the places the
        list was given (the pairs whose distance bin is within reach)."""
        n, keep = C.c_size_t(0), C.c_uint32(0)
        _check(lib().oslam_vote_hits(self._h, scene._h, int(ref_index), None, None, None, 0, C.byref(n), C.byref(keep)))
        num, th, idx = (np.zeros(n.value, np.uint32) for _ in range(3))
        if n.value:
            _check(lib().oslam_vote_hits(self._h, scene._h, int(ref_index), _p(num), _p(th), _p(idx), n.value, C.byref(n), C.byref(keep)))
        return num, th, idx, int(keep.value)

    def close(self):
        if getattr(self, "_db", None) is not None:
            self._db.close()
        if self._h:
            lib().oslam_model_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Database:
    """Resident model database (oslam_db): models with one d_dist share the scene pass of every frame."""

    def __init__(self, models):
        self.models = list(models)
        self._h = C.c_void_p(0)
        arr = (C.c_void_p * len(self.models))(*[m._h for m in self.models])
        _check(lib().oslam_db_create(arr, len(self.models), C.byref(self._h)))
        n, g = C.c_size_t(0), C.c_size_t(0)
        _check(lib().oslam_db_size(self._h, C.byref(n), C.byref(g)))
        self.n_groups = g.value
        for m in self.models:              # the database borrows its models: it goes first
            m._db = self

    def align(self, scene):
        """-> (poses [n,4,4], list of per-model counters)."""
        n = len(self.models)
        T = np.zeros((n, 4, 4), np.float32)
        st = (Stats * n)()
        _check(lib().oslam_db_align(self._h, scene._h, _p(T), st))
        stats = [s.asdict() for s in st]
        for m, t, d in zip(self.models, T, stats):
            m.best_T, m.stats = t, d
        return T, stats

    def refine(self, scene, T, params=None):
        """Every member's pose T[j] refined against the scene in one set of launches (oslam_db_refine); members whose
        T[j] is all zeros are skipped.  -> (T [n,4,4], list of result dicts, found bool [n])."""
        n = len(self.models)
        Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(n, 16))
        To = np.zeros((n, 4, 4), np.float32)
        res = (RefineResult * n)()
        p = params if params is not None else default_refine_params()
        _check(lib().oslam_db_refine(self._h, scene._h, _p(Ti), C.byref(p), _p(To), res))
        out = [r.asdict() for r in res]
        return To, out, np.array([bool(r["found"]) for r in out])

    def verify(self, view, T, params=None):
        """Every member's pose T[j] checked against the depth image of `view` in one set of launches (oslam_db_verify);
        members whose T[j] is all zeros are skipped.  -> (list of result dicts, found bool [n])."""
        n = len(self.models)
        Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(n, 16))
        res = (VerifyResult * max(n, 1))()
        p = params if params is not None else default_verify_params()
        _check(lib().oslam_db_verify(self._h, view._h, _p(Ti), C.byref(p), res))
        out = [res[j].asdict() for j in range(n)]
        return out, np.array([bool(r["found"]) for r in out], dtype=bool)

    def arbitrate(self, view, T, params=None):
        """Arbitration between the members' poses T[j] (oslam_db_arbitrate; all-zero = skipped, e.g. the members that
        verify did not find).  -> (list of result dicts, kept bool [n])."""
        n = len(self.models)
        Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(n, 16))
        res = (ArbitrateResult * max(n, 1))()
        p = params if params is not None else default_arbitrate_params()
        _check(lib().oslam_db_arbitrate(self._h, view._h, _p(Ti), C.byref(p), res))
        out = [res[j].asdict() for j in range(n)]
        return out, np.array([bool(r["kept"]) for r in out], dtype=bool)

    def explain(self, view, T, params=None):
        """explain() with hypothesis j = member j and T[j] (oslam_db_explain; all-zero = skipped, e.g. the members that
        verify did not find).  -> list of result dicts."""
        n = len(self.models)
        Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(n, 16))
        res = (ExplainResult * max(n, 1))()
        p = params if params is not None else default_explain_params()
        _check(lib().oslam_db_explain(self._h, view._h, _p(Ti), C.byref(p), res))
        return [res[j].asdict() for j in range(n)]

    def detect(self, scene, view, params=None):
        """The whole chain for one frame (oslam_db_detect): every instance of every member, refined, verified against
        the view and arbitrated.  -> list of dicts (model, instance, T 4x4, verify, arbitrate) ordered by (model,
        instance).  params: a DetectParams (default_detect_params())."""
        p = params if params is not None else default_detect_params()
        cap = max(1, len(self.models) * int(p.instances.max_instances))
        out = (Detection * cap)()
        n = C.c_size_t(0)
        _check(lib().oslam_db_detect(self._h, scene._h, view._h, C.byref(p), out, cap, C.byref(n)))
        return [out[k].asdict() for k in range(n.value)]

    def track(self, view, members, T, params=None):
        """The hypotheses (member members[h], T[h]) followed into the view's depth image (oslam_db_track; all-zero =
        skipped).  -> (T [H,4,4], list of result dicts, found bool [H])."""
        mem = np.ascontiguousarray(members, np.uint32).reshape(-1)
        H = len(mem)
        Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(H, 16))
        To = np.zeros((max(H, 1), 16), np.float32)
        res = (TrackResult * max(H, 1))()
        p = params if params is not None else default_track_params()
        _check(lib().oslam_db_track(self._h, _p(mem), _p(Ti), H, view._h, C.byref(p), _p(To), res))
        return _track_out(To[:H], res, H)

    def render(self, view_or_camera, members, T, params=None):
        """render() with models[h] = the database's member members[h] (oslam_db_render).  -> a Render."""
        return Render._make(None, view_or_camera, T, params, db=self, members=members)

    def find_instances(self, scene, refine=True, params=None, refine_params=None):
        """Every instance of every member in one frame (oslam_db_align_instances): -> one list per member, as
        Model.find_instances returns it."""
        ip, rp = _instance_args(refine, params, refine_params)
        n = len(self.models)
        cap = int(ip.max_instances)
        out = (Instance * max(n * cap, 1))()
        n_out = np.zeros(max(n, 1), np.uintp)
        st = (Stats * max(n, 1))()
        _check(lib().oslam_db_align_instances(self._h, scene._h, C.byref(ip), C.byref(rp) if rp is not None else None,
                                              out, cap, _p(n_out), st))
        for m, d in zip(self.models, st):
            m.stats = d.asdict()
        return [[out[j * cap + k].astuple() for k in range(int(n_out[j]))] for j in range(n)]

    def align_multi(self, scene, comm, n_total):
        """This rank's models (j = rank, rank + world, ... of n_total) against the whole scene, then every pose to
        every rank through the communicator (oslam_db_align_multi).  -> (poses [n_total,4,4], found [n_total])."""
        return db_align_multi(self, scene, comm, n_total)

    def close(self):
        if self._h:
            lib().oslam_db_destroy(self._h)
            self._h = C.c_void_p(0)
            for m in self.models:
                m._db = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def db_align_multi(db, scene, comm, n_total):
    """oslam_db_align_multi; db may be None on a rank that holds no model."""
    T = np.zeros((int(n_total), 4, 4), np.float32)
    found = np.zeros(int(n_total), np.int32)
    n_mine = len(db.models) if db is not None else 0
    st = (Stats * max(1, n_mine))()
    _check(lib().oslam_db_align_multi(db._h if db is not None else None, scene._h, comm._h, int(n_total), _p(T), _p(found), st))
    if db is not None:
        for m, d in zip(db.models, st):
            m.stats = d.asdict()
    return T, found


class Comm:
    """Communicator of the multi-GPU path (oslam_comm).  RCCL: rank 0 makes the id, everybody gets its bytes
    (here: through torch.distributed, any backend) and creates its end.  Comm.loopback(world): `world` emulated
    ranks on one device inside this process, one thread per rank -- the same exchange code, for tests."""

    def __init__(self, id_bytes, rank, world, dev, _handle=None):
        self._h = C.c_void_p(0)
        self.rank, self.world = rank, world
        if _handle is not None:
            self._h = C.c_void_p(_handle)
            return
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        _check(lib().oslam_comm_create(buf, int(rank), int(world), int(dev), C.byref(self._h)))

    @classmethod
    def loopback(cls, world, dev=0):
        arr = (C.c_void_p * int(world))()
        _check(lib().oslam_comm_create_loopback(int(world), int(dev), arr))
        return [cls(None, r, int(world), dev, _handle=arr[r]) for r in range(int(world))]

    def abort(self):
        _check(lib().oslam_comm_abort(self._h))

    def inject_failure(self, stage):
        _check(lib().oslam_comm_inject_failure(self._h, int(stage)))

    @property
    def broken(self):
        b = C.c_int(0)
        _check(lib().oslam_comm_info(self._h, None, None, C.byref(b)))
        return bool(b.value)

    @staticmethod
    def unique_id():
        buf = (C.c_char * COMM_ID_BYTES)()
        _check(lib().oslam_comm_unique_id(buf))
        return bytes(buf)

    def close(self):
        if self._h:
            lib().oslam_comm_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def refine_correspondences(model, scene, T, radius, min_normal_dot):
    """Scene index of every model point's correspondence under T at `radius` (scene units), -1 = none
    (oslam_refine_correspondences: the rule of oslam_refine, as a test tap)."""
    out = np.zeros(model.n, np.int32)
    _check(lib().oslam_refine_correspondences(model._h, scene._h, _p(_pose16(T)), float(radius), float(min_normal_dot),
                                              _p(out)))
    return out


def verify_classes(model, view, T, params=None):
    """Class of every model point under T against the view (uint8 [M], VERIFY_BACK .. VERIFY_UNKNOWN): the rule of
    oslam_verify as a test tap (oslam_verify_classes)."""
    out = np.zeros(model.n, np.uint8)
    p = params if params is not None else default_verify_params()
    _check(lib().oslam_verify_classes(model._h, view._h, _p(_pose16(T)), C.byref(p), _p(out)))
    return out


def kernel_source_hash():
    """One hash over every file the device code is built from (kernels, their headers, the Makefile with its
    flags).  bench.py quotes PMC passes on file only for exactly this source; tools/make_pmc_traffic.py records it."""
    import hashlib
    d = os.path.join(_HERE, "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".inc")) or name == "Makefile":
            with open(os.path.join(d, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def release_scratch(dev=0):
    _check(lib().oslam_release_scratch(int(dev)))


def ppf_registration(scene_clouds, model_clouds, model_d_dists, ref_point_downsample_factor=1,
                     vote_count_threshold=0.4, cpu_clustering=False, use_l1_norm=False,
                     use_averaged_clusters=False, devUse=0, model_weights=None):
    """ppf_registration (ppf.h:9-15): clouds are (points, normals) tuples.
    Returns results[i][j] = 4x4 pose of model j in scene i."""
    L = lib()
    keep = []

    def pack(clouds):
        xs, ns, cnt = [], [], []
        for pts, nrm in clouds:
            p = np.ascontiguousarray(pts, np.float32)
            q = np.ascontiguousarray(nrm, np.float32)
            keep.extend([p, q])
            xs.append(p.ctypes.data)
            ns.append(q.ctypes.data)
            cnt.append(len(p))
        return ((C.c_void_p * len(xs))(*xs), (C.c_void_p * len(ns))(*ns), (C.c_size_t * len(cnt))(*cnt))

    sx, sn, sc = pack(scene_clouds)
    mx, mn, mc = pack(model_clouds)
    dd = np.ascontiguousarray(model_d_dists, np.float32)
    out = np.zeros((len(scene_clouds), len(model_clouds), 4, 4), np.float32)
    _check(L.oslam_ppf_registration(sx, sn, sc, len(scene_clouds), mx, mn, mc, len(model_clouds), 12, _p(dd),
                                    int(ref_point_downsample_factor), float(vote_count_threshold),
                                    int(cpu_clustering), int(use_l1_norm), int(use_averaged_clusters),
                                    int(devUse), None, _p(out)))
    return out


def ply_read(path):
    """(points [n,3], normals [n,3]) of a PLY file (pcl::io::loadPLYFile<PointNormal>)."""
    L = lib()
    px, pn, n = C.c_void_p(0), C.c_void_p(0), C.c_size_t(0)
    rc = L.oslam_ply_read(os.fsencode(path), C.byref(px), C.byref(pn), C.byref(n))
    if rc != OSLAM_OK:
        raise OslamError(rc, "cannot read PLY file %s" % path)
    try:
        shape = (n.value, 3)
        pts = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_float)), shape=shape).copy() if n.value else np.zeros(shape, np.float32)
        nrm = np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_float)), shape=shape).copy() if n.value else np.zeros(shape, np.float32)
    finally:
        L.oslam_free(px)
        L.oslam_free(pn)
    return pts, nrm


def ply_read_mesh(path):
    """(points [nv,3], normals [nv,3] or None, triangles [nt,3] uint32) of a PLY file with or without normals and faces
    (oslam_ply_read_mesh)."""
    L = lib()
    px, pn, pt, nv, nt = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
    rc = L.oslam_ply_read_mesh(os.fsencode(path), C.byref(px), C.byref(pn), C.byref(pt), C.byref(nv), C.byref(nt))
    if rc != OSLAM_OK:
        raise OslamError(rc, "cannot read PLY file %s" % path)
    try:
        def take(ptr, n, ctype, dtype):
            if not ptr or not n:
                return np.zeros((n, 3), dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n, 3)).copy()
        pts = take(px, nv.value, C.c_float, np.float32)
        nrm = take(pn, nv.value, C.c_float, np.float32) if pn else None
        tri = take(pt, nt.value, C.c_uint32, np.uint32)
    finally:
        L.oslam_free(px)
        L.oslam_free(pn)
        L.oslam_free(pt)
    return pts, nrm, tri


def _rgb_rows(rgb, n):
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    if len(c) != n:
        raise ValueError("rgb must be [n,3] like the points")
    return c


def ply_write(path, points, normals, binary=True, rgb=None):
    """rgb: uint8 [n,3]; the vertices then carry red, green, blue (oslam_ply_write_colour)."""
    p = np.ascontiguousarray(points, np.float32)
    q = np.ascontiguousarray(normals, np.float32)
    if rgb is not None:
        c = _rgb_rows(rgb, len(p))
        rc = lib().oslam_ply_write_colour(os.fsencode(path), _p(p), _p(q), _p(c), len(p), int(binary))
    else:
        rc = lib().oslam_ply_write(os.fsencode(path), _p(p), _p(q), len(p), int(binary))
    if rc != OSLAM_OK:
        raise OslamError(rc, "cannot write PLY file %s" % path)


def ply_write_mesh(path, points, normals, triangles, binary=True, rgb=None):
    """A triangle mesh as a PLY file (oslam_ply_write_mesh): points [nv,3], normals [nv,3] or None (zeros are written),
    triangles [nt,3] vertex indices.  rgb: uint8 [nv,3]; the vertices then carry red, green, blue
    (oslam_ply_write_mesh_colour)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    q = np.zeros_like(p) if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    if q.shape != p.shape:
        raise ValueError("points and normals must have the same shape")
    if rgb is not None:
        c = _rgb_rows(rgb, len(p))
        rc = lib().oslam_ply_write_mesh_colour(os.fsencode(path), _p(p), _p(q), _p(c), len(p), _p(t), len(t), int(binary))
    else:
        rc = lib().oslam_ply_write_mesh(os.fsencode(path), _p(p), _p(q), len(p), _p(t), len(t), int(binary))
    if rc != OSLAM_OK:
        raise OslamError(rc, "cannot write PLY file %s" % path)


def mc_table_row(case):
    """Row `case` of the library's marching-cubes table (oslam_mc_table_row): a list of (e0, e1, e2) cube-edge numbers."""
    edges, n = np.zeros(15, np.uint8), C.c_uint(0)
    _check(lib().oslam_mc_table_row(int(case), _p(edges), C.byref(n)))
    return [tuple(int(e) for e in edges[3 * t:3 * t + 3]) for t in range(n.value)]


def voxel_grid(points, normals=None, leaf=None, dev=0):
    """voxelGridDownsample (alignment.cpp:79-87): (points, normals) of the occupied voxels."""
    xyz, nrm, n, stride, keep = _cloud_args(points, normals)
    po, no = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    k = C.c_size_t(0)
    _check(lib().oslam_voxel_grid(xyz, nrm, n, stride, float(leaf), int(dev), _p(po), _p(no), n, C.byref(k)))
    return po[: k.value].copy(), no[: k.value].copy()


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("depth_scale", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("max_jump", C.c_float)]


def depth_to_cloud(depth, fx, fy, cx, cy, depth_scale=0.001, z_min=0.1, z_max=10.0, max_jump=0.05, dev=0):
    """Depth image (uint16 or float32, [h,w]) -> (points, normals) in camera coordinates
    (oslam_depth_to_cloud; specification: oracle/oracle_depth.c)."""
    d = np.ascontiguousarray(depth)
    if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
        raise ValueError("depth must be a 2-D uint16 or float32 image")
    cam = Camera(fx, fy, cx, cy, depth_scale, z_min, z_max, max_jump)
    n = d.size
    po, no = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    k = C.c_size_t(0)
    _check(lib().oslam_depth_to_cloud(_p(d), int(d.dtype == np.uint16), d.shape[1], d.shape[0], C.byref(cam), int(dev),
                                      _p(po), _p(no), n, C.byref(k)))
    return po[: k.value].copy(), no[: k.value].copy()


class View:
    """A depth image on the device as float z, for verification (oslam_view): the camera and depth conventions of
    depth_to_cloud (z = raw * depth_scale, valid in [z_min, z_max]; max_jump limits the normal map of the tracking stage)."""

    def __init__(self, depth, fx, fy, cx, cy, depth_scale=0.001, z_min=0.1, z_max=10.0, max_jump=0.05, dev=0):
        self._h = C.c_void_p(0)
        d = np.ascontiguousarray(depth)
        if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
            raise ValueError("depth must be a 2-D uint16 or float32 image")
        cam = Camera(fx, fy, cx, cy, depth_scale, z_min, z_max, max_jump)
        self.width, self.height = d.shape[1], d.shape[0]
        _check(lib().oslam_view_create(_p(d), int(d.dtype == np.uint16), self.width, self.height, C.byref(cam), int(dev),
                                       C.byref(self._h)))

    def set_colour(self, rgb, valid=None):
        """The colour image registered with the depth image (oslam_view_set_colour): rgb uint8 [h,w,3]; valid [h,w],
        0 = the pixel has no colour, None = every pixel has one.  A second call replaces the image."""
        c = np.ascontiguousarray(rgb, np.uint8)
        if c.shape != (self.height, self.width, 3):
            raise ValueError("rgb must be [h,w,3] = %r" % ((self.height, self.width, 3),))
        m = None
        if valid is not None:
            m = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
            if m.shape != (self.height, self.width):
                raise ValueError("valid must be [h,w]")
        _check(lib().oslam_view_set_colour(self._h, _p(c), 0, _p(m) if m is not None else None))

    def colour(self):
        """The view's colour image as a test tap (oslam_view_colour): uint32 [h,w], r | g << 8 | b << 16 | a << 24."""
        out = np.zeros((self.height, self.width), np.uint32)
        _check(lib().oslam_view_colour(self._h, _p(out)))
        return out

    def has_colour(self):
        return bool(lib().oslam_view_has_colour(self._h))

    def close(self):
        if self._h:
            lib().oslam_view_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def view_to_cloud(view):
    """The pixels of a view that have a normal, in row-major order (oslam_view_to_cloud): -> (points, normals) in the
    view's camera coordinates.  For a depth view what depth_to_cloud returns for its image, for a ray-cast view the fused
    surface seen from its pose."""
    n = view.width * view.height
    po, no = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    k = C.c_size_t(0)
    _check(lib().oslam_view_to_cloud(view._h, _p(po), _p(no), n, C.byref(k)))
    return po[: k.value].copy(), no[: k.value].copy()


def view_maps(view):
    """The view's maps and z image as a test tap (oslam_view_maps): -> (maps float32 [h,w,8]: x y z has | nx ny nz 0,
    z float32 [h,w])."""
    n = view.width * view.height
    maps, z = np.zeros((n, 8), np.float32), np.zeros(n, np.float32)
    _check(lib().oslam_view_maps(view._h, _p(maps), _p(z)))
    return maps.reshape(view.height, view.width, 8), z.reshape(view.height, view.width)


def default_pyramid_params(**kw):
    """oslam_pyramid_params_default, then the fields given as keywords."""
    p = PyramidParams()
    _check(lib().oslam_pyramid_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown pyramid parameter %r" % k)
        setattr(p, k, v)
    return p


class Pyramid:
    """Up to three views of one depth image, each at half the resolution of the one before (oslam_pyramid): level 0 is
    `view` itself, which the pyramid keeps alive.  level(k) is a View that does not own its handle."""

    def __init__(self, view, levels=3, depth_band=0.09):
        self._h = C.c_void_p(0)
        self.base = view
        self.params = default_pyramid_params(n_levels=levels, depth_band=depth_band)
        _check(lib().oslam_pyramid_create(view._h, C.byref(self.params), C.byref(self._h)))
        self.levels = int(levels)

    def level(self, k):
        h = C.c_void_p(0)
        _check(lib().oslam_pyramid_level(self._h, int(k), C.byref(h)))
        v = _BorrowedView.__new__(_BorrowedView)
        v._h, v._owner = h, self                # the pyramid, and through it the base, live as long as the level does
        v.width, v.height = self.base.width, self.base.height
        for _ in range(int(k)):
            v.width, v.height = (v.width + 1) // 2, (v.height + 1) // 2
        return v

    def close(self):
        if self._h:
            lib().oslam_pyramid_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedView(View):
    """A View whose handle belongs to something else: closing it gives nothing back."""

    def close(self):
        self._h = C.c_void_p(0)


def view_camera(view):
    """The camera and size of any view (oslam_view_info): -> (Camera with depth_scale 1, width, height)."""
    cam = Camera()
    w, h = C.c_int(0), C.c_int(0)
    _check(lib().oslam_view_info(view._h, C.byref(cam), C.byref(w), C.byref(h)))
    return cam, w.value, h.value


def default_render_params(**kw):
    """oslam_render_params_default, then the fields given as keywords."""
    p = RenderParams()
    _check(lib().oslam_render_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown render parameter %r" % k)
        setattr(p, k, v)
    return p


class Render:
    """Hypotheses rendered into a labelled depth view (oslam_render): .view is the z image as a View that does not own
    its handle, .labels() the int32 [h, w] label image (-1 = nothing drawn), .results one dict per hypothesis (drawn,
    pixels, launches, ms_total).  Made by render(), Database.render() and Tracker.render()."""

    @classmethod
    def _make(cls, models, view_or_camera, T, params, db=None, members=None):
        r = cls.__new__(cls)
        r._h = C.c_void_p(0)
        if isinstance(view_or_camera, View):
            cam, w, h = view_camera(view_or_camera)
        else:
            cam, w, h = view_or_camera              # (Camera, width, height)
        p = params if params is not None else default_render_params()
        if db is None:
            r._keep = list(models)                  # the models live as long as the render's caller needs them
            arr, Ti, H = _hypotheses(r._keep, T)
            res = (RenderResult * max(H, 1))()
            _check(lib().oslam_render_create(arr, _p(Ti), H, C.byref(cam), int(w), int(h), C.byref(p), C.byref(r._h), res))
        else:
            r._keep = db
            mem = np.ascontiguousarray(members, np.uint32).reshape(-1)
            H = len(mem)
            Ti = np.ascontiguousarray(np.asarray(T, np.float32).reshape(H, 16))
            res = (RenderResult * max(H, 1))()
            _check(lib().oslam_db_render(db._h, _p(mem), _p(Ti), H, C.byref(cam), int(w), int(h), C.byref(p),
                                         C.byref(r._h), res))
        r.results = [res[k].asdict() for k in range(H)]
        r.width, r.height = int(w), int(h)
        return r

    @property
    def view(self):
        hv = C.c_void_p(0)
        _check(lib().oslam_render_view(self._h, C.byref(hv)))
        v = _BorrowedView.__new__(_BorrowedView)
        v._h, v._owner = hv, self                   # the render lives as long as a view of it does
        v.width, v.height = self.width, self.height
        return v

    def labels(self):
        out = np.zeros(self.width * self.height, np.int32)
        _check(lib().oslam_render_labels(self._h, _p(out)))
        return out.reshape(self.height, self.width)

    def close(self):
        if self._h:
            lib().oslam_render_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render(models, T, view_or_camera, params=None):
    """The image the hypotheses (models[h], T[h]) would produce (oslam_render_create); an all-zero T[h] is skipped.
    view_or_camera: a View, whose camera and size are taken, or (Camera, width, height).  -> a Render."""
    return Render._make(models, view_or_camera, T, params)


def mask_view(view, render, mode="remove", dilate=2, only=-1):
    """The view without (mode "remove") or with only (mode "keep") the pixels that show the rendered objects
    (oslam_view_mask).  -> (View owned by the caller, result dict: valid_in, object_pixels, valid_out, launches, ms_total)."""
    modes = {"remove": MASK_REMOVE, "keep": MASK_KEEP, MASK_REMOVE: MASK_REMOVE, MASK_KEEP: MASK_KEEP}
    if mode not in modes:
        raise ValueError("mode must be 'remove' or 'keep'")
    p = MaskParams()
    _check(lib().oslam_mask_params_default(C.byref(p)))
    p.mode, p.dilate, p.only = modes[mode], int(dilate), int(only)
    res = MaskResult()
    v = View.__new__(View)
    v._h = C.c_void_p(0)
    v.width, v.height = view.width, view.height
    _check(lib().oslam_view_mask(view._h, render._h, C.byref(p), C.byref(v._h), C.byref(res)))
    return v, res.asdict()


def default_planes_params(**kw):
    """oslam_planes_params_default, then the fields given as keywords."""
    p = PlanesParams()
    _check(lib().oslam_planes_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown planes parameter %r" % k)
        setattr(p, k, v)
    return p


class Planes:
    """The dominant planes of a view (oslam_planes): .planes is a list of dicts (normal, d, support, pixels, candidate,
    rms), .labels() the int32 [h, w] label image (-1 = no plane), .rounds() the test tap (counts uint32 [max_planes, 256],
    moments int64 [max_planes, 10]), .result a dict (n_planes, valid_in, labelled, launches, ms_total).  Made by
    find_planes()."""

    def __init__(self, view, params):
        self._h = C.c_void_p(0)
        res = PlanesResult()
        _check(lib().oslam_view_planes(view._h, C.byref(params), C.byref(self._h), C.byref(res)))
        self.width, self.height, self.max_planes = view.width, view.height, int(params.max_planes)
        self.result = res.asdict()
        rec, n = (Plane * PLANES_MAX)(), C.c_size_t(0)
        _check(lib().oslam_planes_get(self._h, rec, PLANES_MAX, C.byref(n)))
        self.planes = [rec[k].asdict() for k in range(n.value)]
        self.records = np.frombuffer(bytes(rec), np.uint32).reshape(PLANES_MAX, 8)[: n.value].copy()   # the records' words

    def labels(self):
        out = np.zeros(self.width * self.height, np.int32)
        _check(lib().oslam_planes_labels(self._h, _p(out)))
        return out.reshape(self.height, self.width)

    def rounds(self):
        counts = np.zeros((self.max_planes, PLANES_CANDIDATES), np.uint32)
        moments = np.zeros((self.max_planes, 10), np.int64)
        _check(lib().oslam_planes_rounds(self._h, _p(counts), _p(moments)))
        return counts, moments

    def close(self):
        if self._h:
            lib().oslam_planes_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def find_planes(view, params=None, **fields):
    """Up to 8 dominant planes of the view and the label of every pixel (oslam_view_planes).  params: a PlanesParams;
    otherwise the defaults with the fields given as keywords.  -> a Planes."""
    if params is not None and fields:
        raise TypeError("give params or fields, not both")
    return Planes(view, params if params is not None else default_planes_params(**fields))


def remove_planes(view, planes, mode="remove", only=-1):
    """The view without (mode "remove") or with only (mode "keep") the pixels of the planes, or of plane `only` alone
    (oslam_view_remove_planes).  -> a View owned by the caller; its .mask_result is the dict of mask_view (valid_in,
    object_pixels = the plane pixels, valid_out, launches, ms_total)."""
    modes = {"remove": MASK_REMOVE, "keep": MASK_KEEP, MASK_REMOVE: MASK_REMOVE, MASK_KEEP: MASK_KEEP}
    if mode not in modes:
        raise ValueError("mode must be 'remove' or 'keep'")
    res = MaskResult()
    v = View.__new__(View)
    v._h = C.c_void_p(0)
    v.width, v.height = view.width, view.height
    _check(lib().oslam_view_remove_planes(view._h, planes._h, modes[mode], int(only), C.byref(v._h), C.byref(res)))
    v.mask_result = res.asdict()
    return v


def default_segments_params(**kw):
    """oslam_segments_params_default, then the fields given as keywords."""
    p = SegmentsParams()
    _check(lib().oslam_segments_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown segments parameter %r" % k)
        setattr(p, k, v)
    return p


class Segments:
    """The connected regions of a view (oslam_segments): .segments is a list of dicts (pixels, root, box = (u0, v0, u1,
    v1), centroid, sides), .records the records' words uint32 [n_segments, 8], .labels() the int32 [h, w] label image (a
    segment's rank or -1), .roots() the test tap (int32 [h, w], the component's root or -1), .result a dict (n_segments,
    n_components, n_candidates, valid_in, labelled, launches, ms_total).  Made by find_segments()."""

    def __init__(self, view, planes, params):
        self._h = C.c_void_p(0)
        res = SegmentsResult()
        _check(lib().oslam_view_segments(view._h, planes._h if planes is not None else None, C.byref(params), C.byref(self._h),
                                         C.byref(res)))
        self.width, self.height = view.width, view.height
        self.result = res.asdict()
        rec, n = (Segment * SEGMENTS_MAX)(), C.c_size_t(0)
        _check(lib().oslam_segments_get(self._h, rec, SEGMENTS_MAX, C.byref(n)))
        self.segments = [rec[k].asdict() for k in range(n.value)]
        self.records = np.frombuffer(bytes(rec), np.uint32).reshape(SEGMENTS_MAX, 8)[: n.value].copy()

    def labels(self):
        out = np.zeros(self.width * self.height, np.int32)
        _check(lib().oslam_segments_labels(self._h, _p(out)))
        return out.reshape(self.height, self.width)

    def roots(self):
        out = np.zeros(self.width * self.height, np.int32)
        _check(lib().oslam_segments_roots(self._h, _p(out)))
        return out.reshape(self.height, self.width)

    def close(self):
        if self._h:
            lib().oslam_segments_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def find_segments(view, planes=None, params=None, **fields):
    """The connected regions of the view's pixels, without the pixels of `planes` (a Planes of this view) when given, and
    the label of every pixel (oslam_view_segments).  params: a SegmentsParams; otherwise the defaults with the fields given
    as keywords.  More than 4096 components of min_pixels or more raise OslamError (OSLAM_E_LIMIT) with both counts in the
    message.  -> a Segments."""
    if params is not None and fields:
        raise TypeError("give params or fields, not both")
    return Segments(view, planes, params if params is not None else default_segments_params(**fields))


def select_segments(view, segs, mode="keep", only=-1):
    """The view with only (mode "keep") or without (mode "remove") the pixels of the segments, or of segment `only` alone
    (oslam_view_select_segments).  -> a View owned by the caller; its .mask_result is the dict of mask_view (valid_in,
    object_pixels = the segment pixels, valid_out, launches, ms_total)."""
    modes = {"remove": MASK_REMOVE, "keep": MASK_KEEP, MASK_REMOVE: MASK_REMOVE, MASK_KEEP: MASK_KEEP}
    if mode not in modes:
        raise ValueError("mode must be 'remove' or 'keep'")
    res = MaskResult()
    v = View.__new__(View)
    v._h = C.c_void_p(0)
    v.width, v.height = view.width, view.height
    _check(lib().oslam_view_select_segments(view._h, segs._h, modes[mode], int(only), C.byref(v._h), C.byref(res)))
    v.mask_result = res.asdict()
    return v


def default_bilateral_params(**kw):
    """oslam_bilateral_params_default, then the fields given as keywords."""
    p = BilateralParams()
    _check(lib().oslam_bilateral_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown bilateral parameter %r" % k)
        setattr(p, k, v)
    return p


def bilateral_view(view, radius=6, sigma_space=4.5, sigma_depth=0.03, params=None):
    """The view with its depth image smoothed by a bilateral filter (oslam_view_bilateral): within a surface the noise
    goes, depth steps above about 3 sigma_depth stay.  params: a BilateralParams, which then replaces the three keywords.
    -> (View owned by the caller, result dict: valid, taps, launches, ms_total)."""
    p = params if params is not None else default_bilateral_params(radius=int(radius), sigma_space=sigma_space,
                                                                   sigma_depth=sigma_depth)
    res = BilateralResult()
    v = View.__new__(View)
    v._h = C.c_void_p(0)
    v.width, v.height = view.width, view.height
    _check(lib().oslam_view_bilateral(view._h, C.byref(p), C.byref(v._h), C.byref(res)))
    return v, res.asdict()


def gauss_table():
    """The library's compiled-in weight table of the bilateral filter (oslam_gauss_table): float32 [288]."""
    out, w = np.zeros(GAUSS_TABLE_N, np.float32), C.c_float(0)
    for i in range(GAUSS_TABLE_N):
        _check(lib().oslam_gauss_table(i, C.byref(w)))
        out[i] = w.value
    return out


def egomotion_pyramid(src_pyr, dst_pyr, T_init=None, params=None, **fields):
    """Coarse-to-fine camera motion over two pyramids (oslam_pyramid_egomotion): stride 1, 2, 4 of a schedule level names
    pyramid level 0, 1, 2.  params: an EgomotionParams, or none and the fields of default_egomotion_params as keywords.
    -> what egomotion returns."""
    if params is not None and fields:
        raise TypeError("give params or keyword fields, not both")
    p = params if params is not None else default_egomotion_params(**fields)
    To = np.zeros(16, np.float32)
    res = EgomotionResult()
    Ti = _pose16(T_init) if T_init is not None else None
    _check(lib().oslam_pyramid_egomotion(src_pyr._h, dst_pyr._h, _p(Ti) if Ti is not None else None, C.byref(p), _p(To),
                                         C.byref(res)))
    return To.reshape(4, 4), res.asdict()


def default_volume_params(**kw):
    """oslam_volume_params_default, then the fields given as keywords (origin: three floats)."""
    p = VolumeParams()
    _check(lib().oslam_volume_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown volume parameter %r" % k)
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_colour_params(**kw):
    """oslam_colour_params_default, then the fields given as keywords."""
    p = ColourParams()
    _check(lib().oslam_colour_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown colour parameter %r" % k)
        setattr(p, k, v)
    return p


def default_surface_params(**kw):
    """oslam_surface_params_default, then the fields given as keywords."""
    p = SurfaceParams()
    _check(lib().oslam_surface_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown surface parameter %r" % k)
        setattr(p, k, v)
    return p


def default_world_surface_params(**fields):
    """oslam_world_surface_params_default, then the fields given as keywords (anchor: three ints)."""
    p = WorldSurfaceParams()
    _check(lib().oslam_world_surface_params_default(C.byref(p)))
    for k, v in fields.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown world surface parameter %r" % k)
        if k == "anchor":
            p.anchor[:] = [int(x) for x in _shift3(v)]
        else:
            setattr(p, k, v)
    return p


def _world_surface_params(min_weight, anchor, dev):
    if anchor is None:
        return default_world_surface_params(min_weight=min_weight, dev=int(dev))
    return default_world_surface_params(min_weight=min_weight, dev=int(dev), anchor_set=1, anchor=anchor)


def default_mesh_params(**kw):
    """oslam_mesh_params_default, then the fields given as keywords."""
    p = MeshParams()
    _check(lib().oslam_mesh_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown mesh parameter %r" % k)
        setattr(p, k, v)
    return p


def default_follow_params(vol, **kw):
    """oslam_follow_params_default for the volume, then the fields given as keywords."""
    p = FollowParams()
    _check(lib().oslam_follow_params_default(vol._h, C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k) or k == "reserved":
            raise TypeError("unknown follow parameter %r" % k)
        setattr(p, k, v)
    return p


def _shift3(s):
    s = np.ascontiguousarray(s, np.int32)
    if s.shape != (3,):
        raise ValueError("a shift is three integers")
    return s


class World:
    """The voxel store (oslam_world): a host-side map from global voxel coordinates g = window index + window offset to
    TSDF words, which keeps what leaves a volume's shifting window (Volume.shift(s, world=...)) and gives it back when
    the window returns.  vol_or_params: a Volume, whose voxel size and created origin the store takes, or a
    WorldParams.  max_bytes bounds the store's memory, 0 = 1 GiB.  colour=True makes a colour store: every voxel keeps
    its colour word next to its TSDF word, so a coloured volume's voxels leave and come back with their colour (a brick
    then takes 4112 bytes instead of 2064; the volume needs enable_colour()).  Needs no device."""

    def __init__(self, vol_or_params, max_bytes=0, colour=False):
        self._h = C.c_void_p(0)
        if isinstance(vol_or_params, WorldParams):
            p = WorldParams.from_buffer_copy(vol_or_params)
        else:
            p = WorldParams()
            _check(lib().oslam_world_params_of(vol_or_params._h, C.byref(p)))
        if max_bytes:
            p.max_bytes = int(max_bytes)
        if colour:
            p.colour = 1
        self.params = p
        _check(lib().oslam_world_create(C.byref(p), C.byref(self._h)))

    def has_colour(self):
        """Whether this is a colour store (oslam_world_has_colour)."""
        return bool(lib().oslam_world_has_colour(self._h))

    def put(self, g, words, colours=None):
        """Stores words uint32 [n] under g int32 [n,3]; unseen words (w == 0) are skipped, a later record wins.
        colours: uint32 [n], the colour word of each record, on a colour store only (oslam_world_put_colour); without
        them a colour store keeps colour 0 for these records."""
        g = np.ascontiguousarray(g, np.int32).reshape(-1, 3)
        words = np.ascontiguousarray(words, np.uint32).ravel()
        if len(g) != len(words):
            raise ValueError("g must be [n,3] and words [n]")
        if colours is None:
            _check(lib().oslam_world_put(self._h, _p(g), _p(words), len(words)))
            return
        colours = np.ascontiguousarray(colours, np.uint32).ravel()
        if len(colours) != len(words):
            raise ValueError("colours must be [n]")
        _check(lib().oslam_world_put_colour(self._h, _p(g), _p(words), _p(colours), len(words)))

    def box(self, lo, hi, take=False, colours=False):
        """The words with lo <= g < hi as uint32 [hz-lz, hy-ly, hx-lx], 0 where nothing is stored; take=True also
        removes them from the store.  colours=True, on a colour store: -> (words, colours), the colour words laid out
        alike (oslam_world_box_colour)."""
        lo, hi = _shift3(lo), _shift3(hi)
        out = np.zeros(tuple(max(int(hi[a]) - int(lo[a]), 0) for a in (2, 1, 0)), np.uint32)
        if colours:
            col = np.zeros_like(out)
            _check(lib().oslam_world_box_colour(self._h, _p(lo), _p(hi), _p(out), _p(col), int(bool(take))))
            return out, col
        _check(lib().oslam_world_box(self._h, _p(lo), _p(hi), _p(out), int(bool(take))))
        return out

    def bricks(self):
        """The keys floor(g / 8) of the store's 8 x 8 x 8 bricks, int32 [n,3], ascending by (bz, by, bx)
        (oslam_world_bricks)."""
        n = C.c_size_t(0)
        _check(lib().oslam_world_bricks(self._h, None, 0, C.byref(n)))
        keys = np.zeros((n.value, 3), np.int32)
        if n.value:
            _check(lib().oslam_world_bricks(self._h, _p(keys), n.value, C.byref(n)))
        return keys

    def colours(self, points, vol=None, anchor=None, dev=0):
        """The fused colour of the whole map, this colour store plus the window of the coloured Volume vol (None: the
        store alone, on device dev), at volume-frame points [n,3] (oslam_world_colours): -> (rgb uint8 [n,3], valid bool
        [n]).  Volume.colours' rule against the map; anchor as in surface(): the points of surface() and the vertices of
        mesh() are to be coloured with the anchor they were made with."""
        sp = _world_surface_params(1, anchor, dev)
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        rgb, valid, n = np.zeros((len(p), 3), np.uint8), np.zeros(len(p), np.uint8), C.c_size_t(0)
        _check(lib().oslam_world_colours(self._h, vol._h if vol is not None else None, C.byref(sp), _p(p), len(p), 0, _p(rgb),
                                         _p(valid), C.byref(n)))
        assert n.value == int(valid.sum())
        return rgb, valid.astype(bool)

    def surface(self, vol=None, min_weight=1, anchor=None, keys=False, dev=0, colour=False):
        """Every zero crossing of the whole map, this store plus the window of the Volume vol (None: the store alone, on
        device dev), as a point with its outward normal in the volume frame (oslam_world_surface): -> (points [n,3],
        normals [n,3]) and with keys=True also int32 [n,4], (g_x, g_y, g_z, axis) of every point.  Bricks ascend by
        (bz, by, bx), a brick's points by voxel and axis; anchor (three ints, default the window's offset, or 0) picks the
        frame the floats are formed in.  With colour=True rgb uint8 [n,3] and valid bool [n], colours() of the points,
        follow (ply_write(..., rgb=) takes them).  The result dict of the call is kept as self.last_surface."""
        sp = _world_surface_params(min_weight, anchor, dev)
        vh = vol._h if vol is not None else None
        n, res = C.c_size_t(0), WorldSurfaceResult()
        _check(lib().oslam_world_surface(self._h, vh, C.byref(sp), None, None, None, 0, C.byref(n), C.byref(res)))
        po, no = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 3), np.float32)
        ko = np.zeros((n.value, 4), np.int32)
        if n.value:
            _check(lib().oslam_world_surface(self._h, vh, C.byref(sp), _p(po), _p(no), _p(ko) if keys else None, n.value,
                                             C.byref(n), C.byref(res)))
        self.last_surface = res.asdict()
        out = (po, no, ko) if keys else (po, no)
        return out + self.colours(po, vol, anchor, dev) if colour else out

    def mesh(self, vol=None, min_weight=1, normals=True, anchor=None, keys=False, dev=0):
        """The marching-cubes mesh of the whole map, this store plus the window of the Volume vol (None: the store alone,
        on device dev) (oslam_world_mesh): -> (vertices [nv,3], normals [nv,3] or None, triangles uint32 [nt,3], result
        dict) and with keys=True also int32 [nv,4], (g_x, g_y, g_z, axis) of every vertex.  The vertices are every
        crossing of World.surface's rule in its order, (0, 0, 0) as the normal where there is none; normals=False skips
        the trilinear reads.  ply_write_mesh takes the output as it is.  The result dict is kept as self.last_mesh.
        mesh_colour() is this call with the vertices' colours."""
        sp = _world_surface_params(min_weight, anchor, dev)
        vh = vol._h if vol is not None else None
        nv, nt, res = C.c_size_t(0), C.c_size_t(0), WorldMeshResult()
        _check(lib().oslam_world_mesh(self._h, vh, C.byref(sp), None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), C.byref(res)))
        xyz = np.zeros((nv.value, 3), np.float32)
        nrm = np.zeros((nv.value, 3), np.float32) if normals else None
        ko = np.zeros((nv.value, 4), np.int32)
        tri = np.zeros((nt.value, 3), np.uint32)
        if nv.value:
            _check(lib().oslam_world_mesh(self._h, vh, C.byref(sp), _p(xyz), _p(nrm) if normals else None, _p(ko) if keys else None,
                                          nv.value, _p(tri), nt.value, C.byref(nv), C.byref(nt), C.byref(res)))
        self.last_mesh = res.asdict()
        return (xyz, nrm, tri, self.last_mesh, ko) if keys else (xyz, nrm, tri, self.last_mesh)

    def mesh_colour(self, vol=None, min_weight=1, normals=True, anchor=None, keys=False, dev=0):
        """mesh() with the colour of every vertex: its outputs, then rgb uint8 [nv,3] and valid bool [nv], colours() of
        the vertices with the same volume and anchor, as Volume.mesh(colour=True) appends them; ply_write_mesh(..., rgb=)
        takes them.  (A method of its own: mesh()'s parameter list is pinned by tests/test_world_mesh_host.py.)"""
        out = self.mesh(vol, min_weight, normals, anchor, keys, dev)
        return out + self.colours(out[0], vol, anchor, dev)

    @staticmethod
    def _raycast_params(anchor, box, mu, dev):
        p = WorldRaycastParams()
        _check(lib().oslam_world_raycast_params_default(C.byref(p)))
        if anchor is not None:
            p.anchor_set, p.anchor[:] = 1, [int(x) for x in _shift3(anchor)]
        if box is not None:
            p.box_set = 1
            p.box_lo[:], p.box_hi[:] = [int(x) for x in _shift3(box[0])], [int(x) for x in _shift3(box[1])]
        p.mu, p.dev = float(mu), int(dev)
        return p

    def raycast(self, T_vol_cam, fx, fy, cx, cy, width, height, vol=None, anchor=None, box=None, mu=0.0, z_min=0.1, z_max=10.0,
                max_jump=0.05, dev=0):
        """The whole map, this store plus the window of the Volume vol (None: the store alone, on device dev), seen from
        T_vol_cam (oslam_world_raycast): -> (View, result dict), as Volume.raycast.  Volume.raycast's rule against the
        map.  anchor (three ints, default the window's offset, or 0) picks the frame the floats are formed in; box =
        (lo, hi) in global voxels, hi exclusive, bounds the march (default: the bounding box of the map's bricks, which
        the result names as box_lo and box_hi); mu 0.0 = the volume's, and is needed without one."""
        cam = Camera(fx, fy, cx, cy, 1.0, z_min, z_max, max_jump)
        rp, res = self._raycast_params(anchor, box, mu, dev), WorldRaycastResult()
        v = View.__new__(View)
        v._h = C.c_void_p(0)
        v.width, v.height = int(width), int(height)
        _check(lib().oslam_world_raycast(self._h, vol._h if vol is not None else None, C.byref(rp), _p(_pose16(T_vol_cam)),
                                         C.byref(cam), int(width), int(height), C.byref(v._h), C.byref(res)))
        return v, res.asdict()

    def track(self, view, T_prev, vol=None, params=None, anchor=None, box=None, mu=0.0):
        """Frame-to-model camera tracking against the whole map (oslam_world_track): Volume.track with raycast() at its
        head, on the view's device.  -> (T_vol_cam float32 4x4, egomotion result dict).  It integrates nothing."""
        p = params if params is not None else default_egomotion_params()
        rp = self._raycast_params(anchor, box, mu, 0)
        To = np.zeros(16, np.float32)
        res = EgomotionResult()
        _check(lib().oslam_world_track(self._h, vol._h if vol is not None else None, C.byref(rp), view._h, _p(_pose16(T_prev)),
                                       C.byref(p), _p(To), C.byref(res)))
        return To.reshape(4, 4), res.asdict()

    def paint(self, view, T_vol_cam, vol=None, anchor=None):
        """The colour of the whole map, this colour store plus the window of the coloured Volume vol, at every pixel of
        view seen from T_vol_cam, into the view's colour image (oslam_world_paint_view; View.colour() reads it): -> the
        number of pixels painted.  Volume.paint with colours()' read; anchor as in raycast()."""
        sp = _world_surface_params(1, anchor, 0)
        n = C.c_uint32(0)
        _check(lib().oslam_world_paint_view(self._h, vol._h if vol is not None else None, C.byref(sp), _p(_pose16(T_vol_cam)),
                                            view._h, C.byref(n)))
        return int(n.value)

    def stats(self):
        s = WorldStats()
        _check(lib().oslam_world_stats_get(self._h, C.byref(s)))
        return s.asdict()

    def clear(self):
        _check(lib().oslam_world_clear(self._h))

    def close(self):
        if self._h:
            lib().oslam_world_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Volume:
    """A TSDF volume on the device (oslam_volume): integrate(view, T_vol_cam) fuses a depth view, raycast(...) returns
    the fused surface as a View, track(view, T_prev) follows the camera against it.  T_vol_cam: the camera's pose in the
    volume frame, float32 4x4.  mu None: 4 voxels."""

    def __init__(self, nx, ny, nz, voxel, origin, mu=None, max_weight=128, dev=0):
        self._h = C.c_void_p(0)
        p = default_volume_params(nx=nx, ny=ny, nz=nz, voxel=voxel, origin=origin,
                                  mu=float(np.float32(4.0) * np.float32(voxel)) if mu is None else mu, max_weight=max_weight)
        self.params = p
        self.T, self._started = np.eye(4, dtype=np.float32), False      # the pose step() keeps
        self.world = []                 # what step(..., follow=...) shifted out: (points, normals) in the volume frame
        self.last_integrate = None      # the integrate result of the last step() that integrated
        _check(lib().oslam_volume_create(C.byref(p), int(dev), C.byref(self._h)))

    def integrate(self, view, T_vol_cam, colour=None):
        """colour: the View that carries the frame's colour image (view itself, or the raw view of a masked or filtered
        one); the volume needs enable_colour().  The result then has "coloured" too (oslam_volume_integrate_colour)."""
        res = IntegrateResult()
        if colour is not None:
            n = C.c_uint32(0)
            _check(lib().oslam_volume_integrate_colour(self._h, view._h, colour._h, _p(_pose16(T_vol_cam)), C.byref(res),
                                                       C.byref(n)))
            return dict(res.asdict(), coloured=int(n.value))
        _check(lib().oslam_volume_integrate(self._h, view._h, _p(_pose16(T_vol_cam)), C.byref(res)))
        return res.asdict()

    def enable_colour(self, **fields):
        """A colour per voxel next to the TSDF (oslam_volume_colour_enable); fields: default_colour_params'."""
        p = default_colour_params(**fields)
        _check(lib().oslam_volume_colour_enable(self._h, C.byref(p)))
        self.colour_params = p

    def colour_words(self):
        """The colour buffer as a test tap: uint32 [nz,ny,nx], r | g << 8 | b << 16 | wc << 24."""
        out = np.zeros((self.params.nz, self.params.ny, self.params.nx), np.uint32)
        _check(lib().oslam_volume_colour_words(self._h, _p(out)))
        return out

    def set_colour_words(self, words):
        w = np.ascontiguousarray(words, np.uint32)
        if w.shape != (self.params.nz, self.params.ny, self.params.nx):
            raise ValueError("words must be [nz,ny,nx]")
        _check(lib().oslam_volume_set_colour_words(self._h, _p(w)))

    def colours(self, points):
        """The fused colour at volume-frame points [n,3] (oslam_volume_colours): -> (rgb uint8 [n,3], valid bool [n])."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        rgb, valid, n = np.zeros((len(p), 3), np.uint8), np.zeros(len(p), np.uint8), C.c_size_t(0)
        _check(lib().oslam_volume_colours(self._h, _p(p), len(p), 0, _p(rgb), _p(valid), C.byref(n)))
        assert n.value == int(valid.sum())
        return rgb, valid.astype(bool)

    def paint(self, view, T_vol_cam):
        """The fused colour at every pixel of view seen from T_vol_cam, into the view's colour image
        (oslam_volume_paint_view; View.colour() reads it): -> the number of pixels painted."""
        n = C.c_uint32(0)
        _check(lib().oslam_volume_paint_view(self._h, _p(_pose16(T_vol_cam)), view._h, C.byref(n)))
        return int(n.value)

    def raycast(self, T_vol_cam, fx, fy, cx, cy, width, height, z_min=0.1, z_max=10.0, max_jump=0.05):
        """-> (View, result dict)"""
        cam = Camera(fx, fy, cx, cy, 1.0, z_min, z_max, max_jump)
        res = RaycastResult()
        v = View.__new__(View)
        v._h = C.c_void_p(0)
        v.width, v.height = int(width), int(height)
        _check(lib().oslam_volume_raycast(self._h, _p(_pose16(T_vol_cam)), C.byref(cam), int(width), int(height),
                                          C.byref(v._h), C.byref(res)))
        return v, res.asdict()

    def track(self, view, T_prev, params=None):
        """Frame-to-model camera tracking (oslam_volume_track): -> (T_vol_cam float32 4x4, egomotion result dict)."""
        p = params if params is not None else default_egomotion_params()
        To = np.zeros(16, np.float32)
        res = EgomotionResult()
        _check(lib().oslam_volume_track(self._h, view._h, _p(_pose16(T_prev)), C.byref(p), _p(To), C.byref(res)))
        return To.reshape(4, 4), res.asdict()

    def track_pyramid(self, pyr, T_prev, params=None, levels=3, depth_band=0.09):
        """Frame-to-model camera tracking over pyramids (oslam_volume_track_pyramid): the volume is ray-cast at T_prev
        and down-sampled with (levels, depth_band).  -> (T_vol_cam float32 4x4, egomotion result dict)."""
        p = params if params is not None else default_egomotion_params()
        pp = default_pyramid_params(n_levels=levels, depth_band=depth_band)
        To = np.zeros(16, np.float32)
        res = EgomotionResult()
        _check(lib().oslam_volume_track_pyramid(self._h, pyr._h, _p(_pose16(T_prev)), C.byref(pp), C.byref(p), _p(To),
                                                C.byref(res)))
        return To.reshape(4, 4), res.asdict()

    def step(self, view, params=None, follow=None, world=None, static=None, smooth=None, colour=None):
        """One frame with the pose kept here: the first call integrates at the initial pose (the identity: the
        volume frame is the first camera's);
        a later call tracks from the kept pose and integrates when the result is ok.  -> (T_vol_cam, egomotion result
        dict, None on the first call).
        follow: follow parameters (default_follow_params).  After a frame was followed and integrated the window then
        moves as follow(T) says; what leaves it is appended to self.world first.
        world: a World.  With follow, the shift then goes through the store (shift(s, world)) and nothing is appended to
        self.world: the store is the map, and a surface handed over now would be handed over again on the next visit.
        static: a Render of the objects that move.  The view is masked with it (mask_view, mode "remove") before it is
        tracked and integrated, the first frame too, and the mask's counters come back as result["mask"] (on the first
        call the result is {"mask": ...} instead of None).
        smooth: a BilateralParams (default_bilateral_params).  KinFu's order: the frame is tracked on the filtered view
        (bilateral_view) and integrated from the raw one, so the map keeps the sensor's detail and the tracker sees
        smooth normals.  The first frame is only integrated, raw, and not filtered.  With static the mask comes first and
        the filter sees the masked view.  The filter's counters come back as result["smooth"]; the filtered view is
        closed before returning.
        colour: the View that carries the frame's colour image, usually view itself.  Every integration of the step then
        fuses it too (integrate(..., colour=)); with static and smooth the z comes from the masked view and the colour
        from this raw one.  With a world made with colour=True the voxels leave and come back with their colour; a
        plain world keeps none, and what it reloads comes back without colour.
        self.last_integrate keeps the result dict of the frame's integration."""
        if static is not None:
            masked, mres = mask_view(view, static, "remove")
            try:
                T, res = self.step(masked, params, follow, world, smooth=smooth, colour=colour)
            finally:
                masked.close()
            res = dict(res) if res is not None else {}
            res["mask"] = mres
            return T, res
        if not self._started:
            self.last_integrate = self.integrate(view, self.T, colour)
            self._started = True
            return self.T.copy(), None
        if smooth is not None:
            filtered, sres = bilateral_view(view, params=smooth)
            try:
                T, res = self.track(filtered, self.T, params)
            finally:
                filtered.close()
            res["smooth"] = sres
        else:
            T, res = self.track(view, self.T, params)
        if res["ok"]:
            self.T = T
            self.last_integrate = self.integrate(view, T, colour)
            if follow is not None:
                s = self.follow(T, follow)
                if any(s) and world is not None:
                    self.shift(s, world)
                elif any(s):
                    po, no, _ = self.leaving(s)
                    self.world.append((po, no))
                    self.shift(s)
        return self.T.copy(), res

    def shift(self, s, world=None):
        """Moves the window of voxels by s = (sx, sy, sz) whole voxels (oslam_volume_shift): -> result dict.
        world: a World.  The seen voxels that leave go into it and those it holds for the entering region come back
        (oslam_volume_shift_world); the result also has "stored" and "reloaded".  A colour store (World(colour=True))
        carries the voxels' colour words along both ways."""
        if world is not None:
            res = ReloadResult()
            _check(lib().oslam_volume_shift_world(self._h, world._h, _p(_shift3(s)), C.byref(res)))
            return res.asdict()
        res = ShiftResult()
        _check(lib().oslam_volume_shift(self._h, _p(_shift3(s)), C.byref(res)))
        return res.asdict()

    def packed(self, s, colours=False):
        """The records the device makes of the seen voxels that shift(s) would move out, as a test tap
        (oslam_volume_pack): -> (lin uint32 [n], ascending linear indices (k * ny + j) * nx + i; words uint32 [n]).
        colours=True, on a volume with colour: -> (lin, words, colours uint32 [n]), the colour word of each record as a
        colour store gets it (oslam_volume_pack_colour)."""
        s = _shift3(s)
        n = C.c_size_t(0)
        if colours:
            _check(lib().oslam_volume_pack_colour(self._h, _p(s), None, None, None, 0, C.byref(n)))
            lin, words, col = (np.zeros(n.value, np.uint32) for _ in range(3))
            if n.value:
                _check(lib().oslam_volume_pack_colour(self._h, _p(s), _p(lin), _p(words), _p(col), n.value, C.byref(n)))
            return lin, words, col
        _check(lib().oslam_volume_pack(self._h, _p(s), None, None, 0, C.byref(n)))
        lin, words = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        if n.value:
            _check(lib().oslam_volume_pack(self._h, _p(s), _p(lin), _p(words), n.value, C.byref(n)))
        return lin, words

    def window(self):
        """-> (offset, three ints in voxels; origin float32 [3]) of the window (oslam_volume_window)."""
        off, org = np.zeros(3, np.int32), np.zeros(3, np.float32)
        _check(lib().oslam_volume_window(self._h, _p(off), _p(org)))
        return tuple(int(x) for x in off), org

    def leaving(self, s, min_weight=1):
        """The part of surface(min_weight) that shift(s) would lose, in its order (oslam_volume_leaving): -> (points
        [n,3], normals [n,3], result dict).  The volume does not change."""
        s = _shift3(s)
        return self._points(lib().oslam_volume_leaving, (self._h, _p(s)), min_weight)

    def follow(self, T_vol_cam, params=None):
        """The shift that keeps the window before the camera at T_vol_cam (oslam_volume_follow; host arithmetic): ->
        (sx, sy, sz), zeros while the camera's look-ahead point is within the threshold of the window's centre."""
        s = np.zeros(3, np.int32)
        _check(lib().oslam_volume_follow(self._h, _p(_pose16(T_vol_cam)), C.byref(params) if params is not None else None, _p(s)))
        return tuple(int(x) for x in s)

    def voxels(self):
        """The whole volume as a test tap: -> (q int16 [nz,ny,nx], w uint16 [nz,ny,nx])."""
        shape = (self.params.nz, self.params.ny, self.params.nx)
        q, w = np.zeros(shape, np.int16), np.zeros(shape, np.uint16)
        _check(lib().oslam_volume_voxels(self._h, _p(q), _p(w)))
        return q, w

    def set_voxels(self, q, w):
        """The inverse of voxels(): q int16 and w uint16, [nz,ny,nx] each (oslam_volume_set_voxels)."""
        shape = (self.params.nz, self.params.ny, self.params.nx)
        q, w = np.ascontiguousarray(q, np.int16), np.ascontiguousarray(w, np.uint16)
        if q.shape != shape or w.shape != shape:
            raise ValueError("q and w must both be [nz,ny,nx] = %r" % (shape,))
        _check(lib().oslam_volume_set_voxels(self._h, _p(q), _p(w)))

    def surface(self, min_weight=1, colour=False):
        """Every zero crossing of the fused TSDF along a voxel edge as a point with its outward normal, in the volume
        frame and in voxel order (oslam_volume_surface): -> (points [n,3], normals [n,3], result dict); with colour=True
        -> (points, normals, result dict, rgb uint8 [n,3], valid bool [n]) with colours() of the points."""
        out = self._points(lib().oslam_volume_surface, (self._h,), min_weight)
        return out + self.colours(out[0]) if colour else out

    @staticmethod
    def _points(call, head, min_weight):
        """The protocol of oslam_volume_surface and oslam_volume_leaving: call(*head, params, outputs...) once without
        outputs for the number of points, then with arrays of that size: -> (points [n,3], normals [n,3], result dict)."""
        sp = default_surface_params(min_weight=min_weight)
        n, res = C.c_size_t(0), SurfaceResult()
        _check(call(*head, C.byref(sp), None, None, 0, C.byref(n), C.byref(res)))
        po, no = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 3), np.float32)
        if n.value:
            _check(call(*head, C.byref(sp), _p(po), _p(no), n.value, C.byref(n), C.byref(res)))
        return po, no, res.asdict()

    def mesh(self, min_weight=1, normals=True, colour=False):
        """The fused surface as a triangle mesh by marching cubes, in the volume frame (oslam_volume_mesh): -> (vertices
        [nv,3], normals [nv,3] with (0, 0, 0) where a vertex has none, or None with normals=False, triangles uint32
        [nt,3], result dict).  The vertices are surface()'s crossings, in its order.  With colour=True rgb uint8 [nv,3] and
        valid bool [nv], colours() of the vertices, follow the result dict."""
        mp = default_mesh_params(min_weight=min_weight)
        nv, nt, res = C.c_size_t(0), C.c_size_t(0), MeshResult()
        _check(lib().oslam_volume_mesh(self._h, C.byref(mp), None, None, 0, None, 0, C.byref(nv), C.byref(nt), C.byref(res)))
        xyz, tri = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.uint32)
        nrm = np.zeros((nv.value, 3), np.float32) if normals else None
        if nv.value:
            _check(lib().oslam_volume_mesh(self._h, C.byref(mp), _p(xyz), _p(nrm) if normals else None, nv.value, _p(tri),
                                           nt.value, C.byref(nv), C.byref(nt), C.byref(res)))
        out = (xyz, nrm, tri, res.asdict())
        return out + self.colours(xyz) if colour else out

    def reset(self):
        _check(lib().oslam_volume_reset(self._h))
        self.T, self._started = np.eye(4, dtype=np.float32), False
        self.world = []

    def close(self):
        if self._h:
            lib().oslam_volume_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ht_dist(A, B):
    """ht_dist (linalg.cu:9-20): (|dt|, |rotation angle|)."""
    a = np.ascontiguousarray(A, np.float32).reshape(16)
    b = np.ascontiguousarray(B, np.float32).reshape(16)
    out = np.zeros(2, np.float32)
    _check(lib().oslam_ht_dist(_p(a), _p(b), _p(out)))
    return float(out[0]), float(out[1])


def pose_stage(cells, m_pts, m_nrm, s_pts, s_nrm, d_dist, cpu_clustering=False, use_l1_norm=False,
               use_averaged_clusters=False, weights=None, allow_no_votes=False):
    """Host stage only (no GPU): filtered+sorted cells -> (best T, all poses)."""
    cells = np.ascontiguousarray(cells, CELL_DTYPE)
    mp, mn = np.ascontiguousarray(m_pts, np.float32), np.ascontiguousarray(m_nrm, np.float32)
    sp, sn = np.ascontiguousarray(s_pts, np.float32), np.ascontiguousarray(s_nrm, np.float32)
    T = np.zeros(16, np.float32)
    poses = np.zeros((len(cells), 16), np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    rc = lib().oslam_pose_stage(_p(cells), len(cells), _p(mp), _p(mn), len(mp), _p(sp), _p(sn), len(sp),
                                float(d_dist), int(cpu_clustering), int(use_l1_norm), int(use_averaged_clusters),
                                _p(w) if w is not None else None, _p(T), _p(poses))
    if not (allow_no_votes and rc == OSLAM_E_NO_VOTES):
        if rc != OSLAM_OK:
            raise OslamError(rc, "pose stage failed")
    return T.reshape(4, 4), poses


def selftest_math(n=1 << 20, seed=1):
    bad = C.c_uint64(0)
    _check(lib().oslam_selftest_math(int(n), int(seed), C.byref(bad)))
    return int(bad.value)


def set_host_threads(n):
    _check(lib().oslam_set_host_threads(int(n)))


def set_stream(stream_ptr):
    _check(lib().oslam_set_stream(C.c_void_p(stream_ptr or 0)))
