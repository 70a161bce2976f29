"""The rule of oslam_view_segments and oslam_view_select_segments (include/oslam.h) restated in numpy: the yardstick of
the device path.

Every float32 step of the gate is a separate numpy float32 operation with the header's grouping, components come from
repeated neighbour-minimum with root hooking and pointer jumping (the definition, not the kernels' schedule), every sum is
a whole number and the centroid is made from Python ints in IEEE doubles, so roots, labels, record words and counts equal
the device's byte for byte.  A trace counts which branches of the rule a call took.  numpy only.
"""
import numpy as np

import planes_ref as PR
import view_ref

F = np.float32
SEGMENTS_MAX = 64
CANDIDATES = 4096
LAUNCHES = 6
TILE = 32                       # of k_seg_tile: the trace tells seams from tile interiors
SCALE = F(8192.0)
BOUND = F(1073741824.0)         # 2^30

SEGMENT_DTYPE = np.dtype([("pixels", "<u4"), ("root", "<u4"), ("u0", "<u2"), ("v0", "<u2"), ("u1", "<u2"), ("v1", "<u2"),
                          ("centroid", "<f4", 3), ("sides", "<u4")])

TRACE_KEYS = ("seam_x_joined", "seam_x_cut", "seam_y_joined", "seam_y_cut", "inner_joined", "inner_cut", "rank_tie",
              "capped", "limit", "below_min_pixels", "centroid_out_of_range", "plane_pixels", "holes", "diagonal_only")


def default_params():
    """oslam_segments_params_default."""
    return dict(max_step=0.0, rel_step=0.0, min_pixels=0, max_segments=16)


def new_trace():
    return {k: 0 for k in TRACE_KEYS}


def gate(za, zb, max_step, rel_step):
    """fabsf(za - zb) <= max_step + rel_step * fminf(za, zb), float32 operation by operation."""
    za, zb = np.asarray(za, np.float32), np.asarray(zb, np.float32)
    prod = F(rel_step) * np.minimum(za, zb)
    lim = F(max_step) + prod
    assert prod.dtype == np.float32 and lim.dtype == np.float32
    return np.abs(za - zb) <= lim


def edge_list(z, inn, max_step, rel_step, trace=None):
    """The joined pairs (a, b) of linear pixel indices, b = a + 1 (first) or a + w."""
    h, w = z.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    tr = trace if trace is not None else new_trace()
    both = inn[:, :-1] & inn[:, 1:]
    jx = both & gate(z[:, :-1], z[:, 1:], max_step, rel_step)
    seam = np.zeros_like(both)
    seam[:, TILE - 1::TILE] = True
    tr["seam_x_joined"] += int((jx & seam).sum())
    tr["seam_x_cut"] += int((both & ~jx & seam).sum())
    tr["inner_joined"] += int((jx & ~seam).sum())
    tr["inner_cut"] += int((both & ~jx & ~seam).sum())
    both = inn[:-1, :] & inn[1:, :]
    jy = both & gate(z[:-1, :], z[1:, :], max_step, rel_step)
    seam = np.zeros_like(both)
    seam[TILE - 1::TILE, :] = True
    tr["seam_y_joined"] += int((jy & seam).sum())
    tr["seam_y_cut"] += int((both & ~jy & seam).sum())
    tr["inner_joined"] += int((jy & ~seam).sum())
    tr["inner_cut"] += int((both & ~jy & ~seam).sum())
    a = np.concatenate([idx[:, :-1][jx], idx[:-1, :][jy]])
    b = np.concatenate([idx[:, 1:][jx], idx[1:, :][jy]])
    return a, b


def components(n, a, b):
    """The smallest index of every node's component under the edges (a, b): neighbour minimum, hooking of the roots and
    pointer jumping until nothing moves -> int64 [n]."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[a], lab[b])
        if (m == lab[a]).all() and (m == lab[b]).all():
            return lab
        np.minimum.at(lab, lab[a], m)
        np.minimum.at(lab, lab[b], m)
        np.minimum.at(lab, a, m)
        np.minimum.at(lab, b, m)
        while True:
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt


def segments(z, cam, max_jump, plane_labels=None, max_step=0.0, rel_step=0.0, min_pixels=0, max_segments=16, trace=None):
    """oslam_view_segments on the z image [h, w] -> dict(roots int32 [h, w], labels int32 [h, w] or None, records
    SEGMENT_DTYPE [n_segments] or None, n_segments, n_components, n_candidates, valid_in, labelled, limit).  limit True is
    the OSLAM_E_LIMIT outcome: only n_components and n_candidates are set."""
    assert 1 <= max_segments <= SEGMENTS_MAX
    tr = trace if trace is not None else new_trace()
    z = np.ascontiguousarray(z, np.float32)
    h, w = z.shape
    step = F(max_step) if max_step else F(max_jump)
    assert step > 0
    minpix = int(min_pixels) if min_pixels else max(1, (w * h) // 1000)
    inn = z > 0
    tr["holes"] += int((~inn).sum())
    if plane_labels is not None:
        tr["plane_pixels"] += int((inn & (plane_labels >= 0)).sum())
        inn = inn & (plane_labels < 0)
    a, b = edge_list(z, inn, step, rel_step, tr)
    comp = components(h * w, a, b)
    roots = np.where(inn.ravel(), comp, -1).astype(np.int32).reshape(h, w)
    # pixels that meet only at a corner and lie in different components
    d1 = inn[:-1, :-1] & inn[1:, 1:] & (roots[:-1, :-1] != roots[1:, 1:])
    d2 = inn[:-1, 1:] & inn[1:, :-1] & (roots[:-1, 1:] != roots[1:, :-1])
    tr["diagonal_only"] += int(d1.sum() + d2.sum())
    ids, counts = np.unique(roots[inn], return_counts=True)
    cand = counts >= minpix
    tr["below_min_pixels"] += int((~cand).sum())
    out = dict(roots=roots, labels=None, records=None, n_segments=0, n_components=len(ids), n_candidates=int(cand.sum()),
               valid_in=int(inn.sum()), labelled=0, limit=False)
    if out["n_candidates"] > CANDIDATES:
        tr["limit"] += 1
        out["limit"] = True
        return out
    ids, counts = ids[cand].astype(np.int64), counts[cand].astype(np.int64)
    order = np.lexsort((ids, -counts))              # pixels descending, then root ascending
    tr["rank_tie"] += int(len(counts) - len(np.unique(counts)))
    tr["capped"] += int(len(order) > max_segments)
    order = order[:max_segments]
    labels = np.full((h, w), -1, np.int32)
    rec = np.zeros(len(order), SEGMENT_DTYPE)
    P = PR.points(z, cam)
    f = P * SCALE
    assert f.dtype == np.float32
    with np.errstate(all="ignore"):
        inb = (np.abs(f) <= BOUND).all(axis=2)
        q = np.where(inb[..., None], np.rint(f), F(0)).astype(np.int64)
    for k, o in enumerate(order):
        m = roots == ids[o]
        labels[m] = k
        vv, uu = np.nonzero(m)
        ok = m & inb
        tr["centroid_out_of_range"] += int((m & ~inb).sum())
        n = int(ok.sum())
        r = rec[k]
        r["pixels"], r["root"] = int(counts[o]), int(ids[o])
        r["u0"], r["v0"], r["u1"], r["v1"] = uu.min(), vv.min(), uu.max(), vv.max()
        for c in range(3):
            s = int(q[..., c][ok].sum())
            r["centroid"][c] = F((float(s) / float(n)) / 8192.0) if n else F(0)
        r["sides"] = (int(uu.min() == 0) | int(vv.min() == 0) << 1 | int(uu.max() == w - 1) << 2 | int(vv.max() == h - 1) << 3)
    out.update(labels=labels, records=rec, n_segments=len(order), labelled=int(rec["pixels"].sum()))
    return out


def find_in_depth(depth, cam, max_jump, plane_labels=None, **kw):
    """segments() on a raw depth image (uint16 or float32) under cam (a dict with depth_scale, z_min, z_max) ->
    (result, z)."""
    z = view_ref.view_z(depth, cam["depth_scale"], cam["z_min"], cam["z_max"])
    return segments(z, cam, max_jump, plane_labels, **kw), z


def select(z, labels, mode="keep", only=-1):
    """oslam_view_select_segments -> (z image, (valid_in, object_pixels, valid_out)): planes_ref.remove on the label
    image."""
    return PR.remove(z, labels, mode, only)
