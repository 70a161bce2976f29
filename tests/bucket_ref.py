"""The two orders inside a model's buckets restated (k_bucket_spread and k_bucket_psort, csrc/oslam_model.hip; the
contract is oslamk_entries' in csrc/oslam_kernels.h and DESIGN.md's at the model build).  numpy and integers only;
written from the comments, not from the kernel's rank expression.

A bucket of `len` entries starts on a multiple of 4 entries (start = the running sum of (len + 3) & ~3) and is worked on
in segments of SEG = 4096 positions.  A slot with key 0 is skipped by both kernels.

Spread (buckets of 2 entries and more): the n entries of a segment are sorted ascending by (spread_key(word), arrival
index) and dealt out: position p = 256 c + 4 lane + j of the segment, h = lane & 31, g = lane >> 5; the positions p < n,
listed in ascending (h, c, j, g), take the sorted entries one after the other.  e4, uv and mi move together (the
fast-mode build, with_uv = 0, has no uv: the array given comes back as it is).

Second order (every bucket of 1 entry and more, on what the spread left): the segment sorted ascending by
(P(word), position), P = word * 30 mod 2^32, gives pw and puv; the directory of a segment at bucket offset b has
K = cells(n) cells of equal width in P, and pdir[b + k], k = 0 .. K, is the first sorted position whose cell
(P * K) >> 32 is >= k.

Everything else -- padding positions, buckets the kernels skip, directory places K + 1 .. of a segment -- comes back as
it went in (e4, uv, mi) or as the 0xA5 bytes the tap filled it with (pw, puv, pdir)."""
import numpy as np

SEG = 4096
CHUNK = 256
PDIR_TAIL = 256                    # directory places behind the entries, as oslam_model_create allocates
ROW_BITS = 11
ROW10_MASK = 0x3FF
ROW_SINK = 1023
ACC_STRIDE = 31
A5_32 = 0xA5A5A5A5
A5_16 = 0xA5A5
M32 = 0xFFFFFFFF


def cells(n):
    """OSLAMK_PDIR_CELLS(n): the largest power of two below n (1 for n <= 2), at most 4096"""
    n = int(n)
    raw = 1 if n <= 1 else 1 << ((n - 1).bit_length() - 1)
    return min(raw, 4096)


def spread_key(words):
    w = np.asarray(words, np.uint32).astype(np.uint64)
    u = (((w >> np.uint64(ROW_BITS)) * np.uint64(30)) & np.uint64(M32)) >> np.uint64(5)
    rows = (((w & np.uint64(ROW10_MASK)) * np.uint64(ACC_STRIDE)) << np.uint64(16)) & np.uint64(M32)
    return (((u + np.uint64(1 << 32) - rows) & np.uint64(M32)) & np.uint64((1 << 21) - 1)).astype(np.uint32)


def p_of(words):
    return ((np.asarray(words, np.uint32).astype(np.uint64) * np.uint64(30)) & np.uint64(M32)).astype(np.uint64)


def cell_of(p, K):
    return (np.asarray(p, np.uint64) * np.uint64(K)) >> np.uint64(32)


def starts_of(lens):
    """-> (start of every bucket, padded total): what k_table_scan gives"""
    padded = (np.asarray(lens, np.int64) + 3) & ~3
    ends = np.cumsum(padded)
    return (ends - padded), int(ends[-1]) if len(ends) else 0


def deal_positions(n):
    """the positions 0 .. n-1 of a segment in the order they are dealt: ascending (h, c, j, g)"""
    p = np.arange(n)
    lane = (p % CHUNK) >> 2
    return np.lexsort((lane >> 5, p & 3, p // CHUNK, lane & 31))


def spread_segment(words):
    """-> src[n]: position p of the segment takes the entry that arrived at src[p]"""
    n = len(words)
    by_key = np.argsort(spread_key(words), kind="stable")
    src = np.empty(n, np.int64)
    src[deal_positions(n)] = by_key
    return src


def psort_segment(words):
    """-> (order[n], dir[K + 1]) of a segment as the spread left it"""
    n = len(words)
    p = p_of(words)
    order = np.argsort(p, kind="stable")
    K = cells(n)
    directory = np.searchsorted(cell_of(p[order], K), np.arange(K + 1), side="left")
    return order, directory


def order_buckets(lens, keys, e4, uv, mi, with_uv=True, spread=True):
    """One launch.  lens / keys [n_buckets]; e4 [total] uint32, uv [total, 2] uint32 (the floats' bits), mi [total]
    uint16, in arrival order with their padding.  -> (e4, uv, mi, pw [total], puv [total, 2], pdir [total + 256])"""
    lens = np.asarray(lens, np.int64)
    keys = np.asarray(keys, np.uint32)
    e4, uv, mi = np.array(e4, np.uint32), np.array(uv, np.uint32), np.array(mi, np.uint16)
    starts, total = starts_of(lens)
    assert e4.shape == (total,) and uv.shape == (total, 2) and mi.shape == (total,)
    pw = np.full(total, A5_32, np.uint32)
    puv = np.full((total, 2), A5_32, np.uint32)
    pdir = np.full(total + PDIR_TAIL, A5_16, np.uint16)
    for b, n_b in enumerate(lens.tolist()):
        if keys[b] == 0:
            continue
        for seg in range(0, n_b, SEG):
            a = int(starts[b]) + seg
            n = min(SEG, n_b - seg)
            if spread and n_b >= 2:
                src = spread_segment(e4[a:a + n])
                e4[a:a + n], mi[a:a + n] = e4[a:a + n][src], mi[a:a + n][src]
                if with_uv:                                               # the fast-mode build has no uv to move
                    uv[a:a + n] = uv[a:a + n][src]
            if with_uv:
                order, directory = psort_segment(e4[a:a + n])
                pw[a:a + n], puv[a:a + n] = e4[a:a + n][order], uv[a:a + n][order]
                pdir[a:a + len(directory)] = directory
    return e4, uv, mi, pw, puv, pdir
