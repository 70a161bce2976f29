"""A plain statement of the pose tail's clustering scores (rot_clustering_kernel, kernel.cu:702-763, without the
in-place averaging) in numpy: float32, one pose after the other, every sum in the reference's order.

Input is reference-side data only (cluster_inputs.reference_side): translations, quaternions (w, x, y, z), weighted
votes, translation cells and their hashes, in pose order.  A pose visits its 26 neighbour cells in (dx, dy, dz) order,
skips its own cell and every neighbour whose hash is 0, takes the poses that carry the neighbour's HASH (cells that
share a hash are one list) in ascending pose index, and adds the weighted votes of those that pass the rotation test
and -- unless use_l1 -- the distance test, to a float32 sum that starts at 1.  The winner is the first maximum."""
import numpy as np

F = np.float32
D_ANGLE = F(F(2.0) * F(3.141592654)) / F(30.0)                   # kernel.h:16
ROT_THRESH_SQ = F(F(2) * D_ANGLE) * F(F(2) * D_ANGLE)           # kernel.h:17, squared as kernel.cu:716 does
FNV_BASIS, FNV_PRIME = 2166136261, 16777619


def fnv_cells(cells):
    """kernel.cu:23-30 over the 12 bytes of int32 cells [n, 3]: FNV-1a through a signed char pointer."""
    c = np.ascontiguousarray(cells, np.int32).reshape(-1, 3)
    by = c.view(np.int8).reshape(len(c), 12).astype(np.int64) & 0xFFFFFFFF          # sign-extended to 32 bits
    h = np.full(len(c), FNV_BASIS, np.uint64)
    for k in range(12):
        h = ((h ^ by[:, k].astype(np.uint64)) * np.uint64(FNV_PRIME)) & np.uint64(0xFFFFFFFF)
    return h.astype(np.uint32)


def trans_cells(trans, d_dist):
    """kernel.cu:102-107,674-680: (int)((t - fmodf(t, d)) / d), truncating toward zero."""
    t = np.ascontiguousarray(trans, F)
    d = F(d_dist)
    return ((t - np.fmod(t, d)) / d).astype(np.int32)


NEIGHBOURS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]       # lane c = index here


def hash_lists(hashes):
    """hash -> ascending pose indices"""
    out = {}
    for i, h in enumerate(np.asarray(hashes).tolist()):
        out.setdefault(h, []).append(i)
    return {h: np.asarray(v, np.int64) for h, v in out.items()}


def neighbour_hashes(cell):
    """the 27 hashes around one cell in lane order; lane 13 (the pose's own cell) is reported as 0: never searched"""
    nb = np.asarray(cell, np.int64)[None, :] + np.asarray(NEIGHBOURS, np.int64)
    h = fnv_cells(nb.astype(np.int32))
    h[13] = 0
    return h


def candidates(ref, i, lists=None, cache=None):
    """Pose i's candidate list: (pose indices in visiting order, the 27 list lengths per lane)."""
    lists = ref["lists"] if lists is None else lists
    key = tuple(int(v) for v in ref["cell"][i])
    nh = cache.get(key) if cache is not None else None
    if nh is None:
        nh = neighbour_hashes(ref["cell"][i])
        if cache is not None:
            cache[key] = nh
    empty = np.zeros(0, np.int64)
    parts = [lists.get(int(h), empty) if h != 0 else empty for h in nh.tolist()]
    lens = np.asarray([len(p) for p in parts], np.int64)
    return (np.concatenate(parts) if lens.sum() else empty), lens


def compatible(ref, i, cand, d_dist, use_l1):
    """the reference's two tests of pose i against the poses `cand`, in float32 with its order of operations"""
    q, qo = ref["quat"][i], ref["quat"][cand]
    dot = q[0] * qo[:, 0]
    for k in (1, 2, 3):
        dot = dot + q[k] * qo[:, k]
    ok = np.abs(F(8) * (F(1) - dot)) < ROT_THRESH_SQ
    if not use_l1:
        e = ref["trans"][i][None, :] - ref["trans"][cand]
        d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        d2 = d2 + e[:, 2] * e[:, 2]
        ok &= np.sqrt(d2) < F(d_dist)                  # a real float32 root (IEEE: correctly rounded), then the comparison
    return ok


def seq_sum(start, values):
    """float32 sum in the given order"""
    if len(values) == 0:
        return F(start)
    return np.cumsum(np.concatenate([[F(start)], np.asarray(values, F)]), dtype=F)[-1]


def scores(ref, d_dist, use_l1=False):
    """-> (scores [n] float32, index of the first maximum)"""
    n = len(ref["trans"])
    out = np.ones(n, F)                                      # kernel.cu:722: a pose with no candidate keeps the 1
    # the candidate list is the same for every pose of a cell: the neighbour hashes of all distinct cells at once, then
    # one pose after the other
    ucell, inv = np.unique(ref["cell"], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    nbh = fnv_cells((ucell[:, None, :].astype(np.int64) + np.asarray(NEIGHBOURS, np.int64)[None]).astype(np.int32).reshape(-1, 3))
    nbh = nbh.reshape(-1, 27)
    nbh[:, 13] = 0
    lists = ref["lists"]
    present = np.isin(nbh, np.fromiter(lists.keys(), np.uint32, len(lists))) & (nbh != 0)
    cand_of = {}
    for u in np.nonzero(present.any(axis=1))[0]:
        cand_of[int(u)] = np.concatenate([lists[int(h)] for h in nbh[u][present[u]]])
    for i in np.nonzero(np.isin(inv, np.fromiter(cand_of.keys(), np.int64, len(cand_of))))[0]:
        cand = cand_of[int(inv[i])]
        ok = compatible(ref, int(i), cand, d_dist, use_l1)
        out[i] = seq_sum(1, ref["wv"][cand[ok]])
    return out, int(np.argmax(out))
