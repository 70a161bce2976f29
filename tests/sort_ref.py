"""The hit sort's result restated (k_sort_hits, csrc/oslam_sort.hip; the contract is DESIGN.md's at the hit sort).
numpy and integers only.

A list owns `slots` places and holds n = min(count, slots) hits.  The hits are taken in segments of SEG (16384 while
id_bits + 14 <= 32: key number and place share one 32-bit word; 8192 above that).  Inside a segment the hits are ordered
by key number, hits of one key in arrival order, and cut into runs: a run starts at every multiple of 64 places of the
segment and wherever the key changes, and ends at the next start or with the segment.  A run is marked iff one of its
hits has theta == MARKER."""
import numpy as np

MARKER = 0xFFFFFFFF
RUN_SHIFT = 26
IDX_BITS = 14
GROUP = 64
SENTINEL = 0xA5A5A5A5
FLAG = 0x80000000


def seg_of(id_bits):
    return 1 << IDX_BITS if id_bits + IDX_BITS <= 32 else 1 << (IDX_BITS - 1)


def sort_list(numbers, theta, idx, count, id_bits):
    """One list: numbers / theta / idx [slots] in arrival order -> dict of numbers, theta, idx [slots], runs [slots, 2],
    run_count, and `detail`: per run (segment start, place in the segment, hits, key, marked) for the tests of the cases."""
    numbers, theta, idx = (np.asarray(a, np.uint32) for a in (numbers, theta, idx))
    slots = len(numbers)
    n = min(int(count), slots)
    seg_max = seg_of(id_bits)
    out_n = numbers.copy()                                                # past n: the input
    out_t = np.full(slots, SENTINEL, np.uint32)
    out_i = np.full(slots, SENTINEL, np.uint32)
    runs = np.full((slots, 2), SENTINEL, np.uint32)
    detail = []
    r = 0
    for seg in range(0, n, seg_max):
        m = min(seg_max, n - seg)
        order = np.argsort(numbers[seg:seg + m], kind="stable")
        k = numbers[seg:seg + m][order].astype(np.int64)
        t = theta[seg:seg + m][order]
        out_t[seg:seg + m] = t
        out_i[seg:seg + m] = idx[seg:seg + m][order]
        place = np.arange(m)
        head = place % GROUP == 0
        head[1:] |= k[1:] != k[:-1]
        starts = np.nonzero(head)[0]
        ends = np.append(starts[1:], m)
        marked_hit = t == np.uint32(MARKER)
        for s, e in zip(starts.tolist(), ends.tolist()):
            marked = bool(marked_hit[s:e].any())
            key = int(k[s])
            runs[r, 0] = key | ((e - s - 1) << RUN_SHIFT)
            runs[r, 1] = (seg + s) | (FLAG if marked else 0)
            out_n[seg + s:seg + e] = key | (FLAG if marked else 0)
            detail.append((seg, s, e - s, key, marked))
            r += 1
    return dict(numbers=out_n, theta=out_t, idx=out_i, runs=runs, run_count=r, detail=detail)


def sort_lists(numbers, theta, idx, offsets, counts, id_bits):
    """Several lists side by side, as one launch takes them -> (numbers, theta, idx, runs, run_counts, details)."""
    numbers, theta, idx = (np.asarray(a, np.uint32) for a in (numbers, theta, idx))
    total = int(offsets[-1])
    out_n = numbers.copy()
    out_t = np.full(total, SENTINEL, np.uint32)
    out_i = np.full(total, SENTINEL, np.uint32)
    runs = np.full((total, 2), SENTINEL, np.uint32)
    rc = np.zeros(len(counts), np.uint32)
    details = []
    for l, c in enumerate(counts):
        a, b = int(offsets[l]), int(offsets[l + 1])
        one = sort_list(numbers[a:b], theta[a:b], idx[a:b], c, id_bits)
        out_n[a:b], out_t[a:b], out_i[a:b], runs[a:b] = one["numbers"], one["theta"], one["idx"], one["runs"]
        rc[l] = one["run_count"]
        details.append(one["detail"])
    return out_n, out_t, out_i, runs, rc, details
