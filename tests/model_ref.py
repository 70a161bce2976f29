"""A model's tables restated from its cloud and parameters alone (oslam_model_create, oslam_model_load, oslam_db_create:
csrc/oslam_model.c, csrc/oslam_db.c and the build kernels of csrc/oslam_model.hip; the layout is csrc/oslam_kernels.h's).

Where the values come from:
  * the key of every ordered pair: the CPU oracle (oracle.ppf_all_pairs), which shares no code with the library;
  * the entry word and uv of a pair: the host statements -- rows y and z of oslam_build_T_g (host code with libm, no
    device) and pc_row_dot, pc_angle_t22, pc_entry_word, pc_row11 of ppf_core.h through tests/native/model_ref_helper.c,
    built with gcc -ffp-contract=off; the same helper evaluates pc_key_of_bins over every distance bin for `reach`/`kmap`;
  * everything structural: numpy, here.

WHAT IS NOT DETERMINED.  The count pass claims table slots by atomic compare-and-swap and the fill pass appends by atomic
cursor, so which slot of its probe run a key sits in, the arrival order inside a bucket and, with it, which entries of a
bucket above 4096 share a segment differ from build to build.  hold() therefore asks of the device only what every
correct build gives: sets and multisets per bucket, probe reachability, the scan, and the two orders as functions of
the device's OWN segments (tests/bucket_ref.py).  Places of pw, puv and pdir that the build does not own are
uninitialised memory and are not looked at.

simulate() builds tables the same way in numpy with a seeded arrival order: the CPU tests hold it to hold(), and
show that hold() refuses tables that are wrong in one place."""
import ctypes as C
import os
import subprocess

import numpy as np

import bucket_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objective-slam_amd", "csrc")
BUILD = os.path.join(ROOT, "build")

SLICE = 2046
HALF = 1023
COMBOS = 17 * 17 * 17
REACH_BINS = 16384
KMAP_MAX_BINS = 2048
KMAP_NONE = 0xFFFFFFFF
GOLD = 2654435761
SINK = B.ROW_SINK
MARK = 0x80000000

_HELPER = None


def helper():
    global _HELPER
    if _HELPER is None:
        os.makedirs(BUILD, exist_ok=True)
        out = os.path.join(BUILD, "libmodel_ref_helper.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "model_ref_helper.c"), "-o", out, "-lm"], check=True)
        L = C.CDLL(out)
        vp = C.c_void_p
        L.mrh_entries.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
        L.mrh_entries.restype = None
        L.mrh_bins.argtypes = [C.c_float, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp]
        L.mrh_bins.restype = C.c_int
        _HELPER = L
    return _HELPER


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def log2_exact(x):
    assert x > 0 and x & (x - 1) == 0, x
    return x.bit_length() - 1


def home_of(keys, shift):
    return ((np.asarray(keys, np.uint64) * np.uint64(GOLD)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


def union_cap(distinct):
    """oslam_build_union / oslam_db_create: at most a quarter full, 2^16 .. 2^26 slots"""
    lg = 16
    while (1 << lg) < 4 * distinct and lg < 26:
        lg += 1
    return 1 << lg


def id_bits_of(n_ids):
    b = 1
    while b < 32 and (1 << b) < n_ids:
        b += 1
    return b


def stride_of(n_ids):
    return ((n_ids + 63) & ~63) or 64


class Model:
    """the pairs of one model, sorted by (slice, key, reference point, second point), and its buckets"""

    def __init__(self, points, normals, d_dist, oracle, ppf):
        self.p = np.ascontiguousarray(points, np.float32)
        self.n = np.ascontiguousarray(normals, np.float32)
        self.d = float(np.float32(d_dist))
        M = self.M = len(self.p)
        self.n_slices = (M + SLICE - 1) // SLICE
        keys = oracle.ppf_all_pairs(self.p, self.n, 1, self.d, want_ppf=False)[1]
        np.fill_diagonal(keys, 0)
        r, i = np.nonzero(keys)                                              # row-major: ascending (r, i)
        k = keys[keys != 0]
        del keys
        rows8 = np.zeros((M, 8), np.float32)
        T = np.zeros(16, np.float32)
        for j in range(M):                                                   # rows y, z of T_m_g: the library's host code
            ppf.lib().oslam_build_T_g(_p(self.p[j]), _p(self.n[j]), _p(T))
            rows8[j] = T[4:12]
        r32, i32 = r.astype(np.uint32), i.astype(np.uint32)
        word, uv, force = np.zeros(len(r), np.uint32), np.zeros((len(r), 2), np.float32), np.zeros(len(r), np.uint8)
        helper().mrh_entries(_p(rows8), _p(self.p), _p(r32), _p(i32), len(r), _p(word), _p(uv), _p(force))
        sl = r // SLICE
        code = (sl.astype(np.uint64) << np.uint64(32)) | k
        order = np.argsort(code, kind="stable")                               # (slice, key), then (r, i) as they came
        code = code[order]
        self.slice, self.key, self.r, self.mi = sl[order], k[order], r32[order], i32[order].astype(np.uint16)
        self.word, self.uv, self.force = word[order], uv[order].view(np.uint32), force[order].astype(bool)
        first = np.flatnonzero(np.concatenate([[True], code[1:] != code[:-1]])) if len(code) else np.zeros(0, np.int64)
        length = np.diff(np.append(first, len(code)))
        self.b_first, self.b_len = first, length
        self.b_slice, self.b_key = self.slice[first], self.key[first]
        self.b_of = np.repeat(np.arange(len(first)), length)                  # bucket of every sorted pair
        self.b_force = np.add.reduceat(self.force.astype(np.int64), first) > 0 if len(first) else np.zeros(0, bool)
        self.b_clean = np.add.reduceat((~self.force).astype(np.int64), first) > 0 if len(first) else np.zeros(0, bool)
        self.n_unique = np.bincount(self.b_slice, minlength=self.n_slices)
        cap = 1 << 16
        while self.n_unique.max(initial=0) > cap // 2:
            cap <<= 1
        self.cap, self.shift = cap, 32 - log2_exact(cap)
        self.n_entries = int(((length + 3) & ~3).sum())
        self.ukeys, inv = np.unique(self.b_key, return_inverse=True)
        self.uweights = np.bincount(inv, weights=length.astype(np.float64), minlength=len(self.ukeys)).astype(np.int64)
        self.num_model_keys = len(self.ukeys) + 1


class Union:
    """the union table of one model or of a group: keys, weights, numbers, reach and the key map"""

    def __init__(self, members, d_dist):
        self.d = float(np.float32(d_dist))
        allk = np.concatenate([m.ukeys for m in members])
        allw = np.concatenate([m.uweights for m in members])
        self.keys, inv = np.unique(allk, return_inverse=True)
        self.weights = np.bincount(inv, weights=allw.astype(np.float64), minlength=len(self.keys)).astype(np.uint64)
        if len(members) == 1:
            self.ucap = union_cap(int(members[0].n_unique.sum()))           # the sum of the slices' distinct counts
        else:
            self.ucap = union_cap(sum(m.num_model_keys for m in members))
        self.ushift = 32 - log2_exact(self.ucap)
        self.n_ids = len(self.keys)
        self.id_bits, self.stride = id_bits_of(self.n_ids), stride_of(self.n_ids)
        rank_order = np.lexsort((self.keys, -self.weights.astype(np.int64)))   # weight descending, key ascending
        self.rank = np.empty(self.n_ids, np.uint32)
        self.rank[rank_order] = np.arange(self.n_ids, dtype=np.uint32)
        found = np.zeros(REACH_BINS, np.uint8)
        assert helper().mrh_bins(self.d, _p(self.keys), len(self.keys), 0, REACH_BINS, None, _p(found)) == 0
        self.reach = np.packbits(found.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()
        at = np.nonzero(found)[0]
        self.top = int(at[-1]) + 1 if len(at) else 0
        self.reach_words = (self.top + 31) // 32
        self.kmap_bins = min(self.top, KMAP_MAX_BINS)
        self.kmap_index = np.zeros((self.kmap_bins, COMBOS), np.int32)
        if self.kmap_bins:
            assert helper().mrh_bins(self.d, _p(self.keys), len(self.keys), 0, self.kmap_bins, _p(self.kmap_index),
                                     _p(np.zeros(self.kmap_bins, np.uint8))) == 0


# ---------------------------------------------------------------- what every correct build gives
def reachable(keys, shift):
    """every key of an open-addressing table is found from its home slot by linear probing over occupied slots"""
    keys = np.asarray(keys, np.uint32)
    cap = len(keys)
    occ = np.nonzero(keys)[0]
    empty = np.nonzero(keys == 0)[0]
    if len(empty) == 0:
        return False
    home = home_of(keys[occ], shift).astype(np.int64)
    last_empty = empty[np.searchsorted(empty, occ) - 1]                       # the empty slot before (cyclic: index -1 = the last)
    run = (occ - last_empty) % cap - 1                                        # occupied slots right before this one
    return bool(np.all((occ - home) % cap <= run))


def owned_places(starts, lens):
    """the places start .. start + len of every bucket, and the bucket of each"""
    lens = np.asarray(lens, np.int64)
    b = np.repeat(np.arange(len(lens)), lens)
    off = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    return np.asarray(starts, np.int64)[b] + off, b


def second_order_places(starts, lens):
    """the places of pw / puv and of pdir that the build owns: every entry, and K + 1 directory places per segment"""
    entry, _ = owned_places(starts, lens)
    directory = []
    for a, n_b in zip(np.asarray(starts, np.int64).tolist(), np.asarray(lens, np.int64).tolist()):
        for seg in range(0, n_b, B.SEG):
            directory.append(a + seg + np.arange(B.cells(min(B.SEG, n_b - seg)) + 1))
    return entry, np.concatenate(directory) if directory else np.zeros(0, np.int64)


def same_rows(a, b):
    """two lists of up to four 32-bit columns hold the same multiset of rows"""
    def rows(cols):
        cols = [np.asarray(c).astype(np.uint64) for c in cols] + [np.zeros(len(cols[0]), np.uint64)] * (4 - len(cols))
        k1, k2 = (cols[0] << np.uint64(32)) | cols[1], (cols[2] << np.uint64(32)) | cols[3]
        order = np.lexsort((k2, k1))
        return k1[order], k2[order]
    if len(a[0]) != len(b[0]):
        return False
    (a1, a2), (b1, b2) = rows(a), rows(b)
    return np.array_equal(a1, b1) and np.array_equal(a2, b2)


def hold(T, model, union, vote_order=0, spread=True, fast=False):
    """assert everything that is determined of the tables T (ppf.Model.tables(), or simulate()) of `model` under `union`"""
    m, u = model, union
    for name, want in (("cap", m.cap), ("shift", m.shift), ("n_slices", m.n_slices), ("n_entries", m.n_entries),
                       ("num_model_keys", m.num_model_keys), ("ucap", u.ucap), ("ushift", u.ushift), ("n_ids", u.n_ids),
                       ("id_bits", u.id_bits), ("uinfo_stride", u.stride), ("kmap_bins", u.kmap_bins),
                       ("reach_words", u.reach_words), ("has_pw", int(not fast))):
        assert T[name] == want, (name, T[name], want)
    ne = m.n_entries
    # ---- slots
    slots = T["slots"]
    assert slots.shape == (m.n_slices, m.cap, 4)
    flat = slots.reshape(-1, 4)
    key, start, length, cur = (flat[:, c].astype(np.int64) for c in range(4))
    assert not np.any((key == 0) & ((length != 0) | (cur != 0))), "an empty slot with entries"
    padded = (length + 3) & ~3
    assert np.array_equal(start, np.cumsum(padded) - padded), "start is not the running sum of the padded lengths"
    assert int(padded.sum()) == ne
    assert np.array_equal(cur & 0x7FFFFFFF, length), "cur is not len"
    occ = np.nonzero(key)[0]
    by = np.lexsort((key[occ], occ // m.cap))                                 # the device's buckets in the restatement's order
    occ = occ[by]
    assert np.array_equal(occ // m.cap, m.b_slice) and np.array_equal(key[occ], m.b_key), "the key sets differ"
    assert np.array_equal(length[occ], m.b_len), "a bucket's length differs"
    assert np.array_equal((cur[occ] & MARK) != 0, m.b_force), "the marker flag differs"
    for s in range(m.n_slices):
        assert reachable(slots[s, :, 0], m.shift), ("a key of slice %d cannot be found by probing" % s)
    d_start = start[occ]                                                      # per restated bucket: where the device keeps it
    # ---- e4 / mi
    e4, mi = T["e4"], T["mi"]
    assert e4.shape == (ne + 256,) and mi.shape == (ne,)
    place, b = owned_places(d_start, m.b_len)
    assert np.array_equal(b, m.b_of)
    pad = np.ones(ne + 256, bool)
    pad[place] = False
    assert np.all(e4[pad] == SINK), "a padding word is not the sink row's"
    assert same_rows([b, e4[place], mi[place]], [m.b_of, m.word, m.mi]), "a bucket's (word, mi) differ"
    long_b = np.nonzero(m.b_len >= 2)[0]
    one_b = np.nonzero(m.b_len == 1)[0]
    if spread:
        for j in long_b.tolist():
            for seg in range(0, int(m.b_len[j]), B.SEG):
                a, n = int(d_start[j]) + seg, min(B.SEG, int(m.b_len[j]) - seg)
                k = B.spread_key(e4[a:a + n])
                want = np.empty(n, np.uint32)
                want[B.deal_positions(n)] = np.sort(k)
                assert np.array_equal(k, want), ("the spread keys of the segment at %d are not dealt as stated" % a)
    # ---- pw / puv / pdir
    if not fast:
        pw, puv, pdir = T["pw"], T["puv"].view(np.uint32), T["pdir"]
        assert pw.shape == (ne,) and puv.shape == (ne, 2) and pdir.shape == (ne + 256,)
        assert same_rows([b, pw[place], puv[place, 0], puv[place, 1]],
                         [m.b_of, m.word, m.uv[:, 0], m.uv[:, 1]]), "a bucket's (pw, puv) differ"
        s1 = d_start[one_b]
        assert np.array_equal(pw[s1], e4[s1]) and np.all(pdir[s1] == 0) and np.all(pdir[s1 + 1] == 1)
        for j in long_b.tolist():
            for seg in range(0, int(m.b_len[j]), B.SEG):
                a, n = int(d_start[j]) + seg, min(B.SEG, int(m.b_len[j]) - seg)
                order, directory = B.psort_segment(e4[a:a + n])
                assert np.array_equal(pw[a:a + n], e4[a:a + n][order]), ("pw of the segment at %d is not the stable sort by P" % a)
                assert np.array_equal(pdir[a:a + len(directory)], directory), ("the directory of the segment at %d" % a)
    else:
        assert "pw" not in T
    # ---- ukeys, weights, uids
    ukeys, uids, weights = T["ukeys"], T["uids"], T["weights"]
    assert ukeys.shape == uids.shape == weights.shape == (u.ucap,)
    uocc = np.nonzero(ukeys)[0]
    by_key = uocc[np.argsort(ukeys[uocc], kind="stable")]                      # union slot of every key, keys ascending
    assert np.array_equal(ukeys[by_key], u.keys), "the union's key set differs"
    assert reachable(ukeys, u.ushift), "a key of the union table cannot be found by probing"
    assert np.array_equal(weights[by_key], u.weights) and not np.any(weights[ukeys == 0]), "the weights differ"
    if vote_order in (0, 2):
        number = u.rank
    else:
        number = np.empty(u.n_ids, np.uint32)
        number[np.argsort(by_key, kind="stable")] = np.arange(u.n_ids, dtype=np.uint32)   # in union-slot order
    assert np.array_equal(uids[by_key], number) and not np.any(uids[ukeys == 0]), "the key numbers differ"
    # ---- reach, kmap
    assert np.array_equal(T["reach"], u.reach), "the reach bitset differs"
    want = np.where(u.kmap_index >= 0, number[np.maximum(u.kmap_index, 0)] if u.n_ids else 0, KMAP_NONE).astype(np.uint32)
    assert T["kmap"].shape == want.shape and np.array_equal(T["kmap"], want), "the key map differs"
    # ---- uinfo
    want = np.zeros((m.n_slices, u.stride, 2), np.uint32)
    num_of_bucket = number[np.searchsorted(u.keys, m.b_key)]
    want[m.b_slice, num_of_bucket, 0] = d_start
    want[m.b_slice, num_of_bucket, 1] = m.b_len | (m.b_force.astype(np.int64) << 31)
    assert T["uinfo"].shape == want.shape and np.array_equal(T["uinfo"], want), "uinfo differs"


# ---------------------------------------------------------------- a build in numpy, with a seeded arrival order
def _insert(cap, shift, keys, rng):
    table = np.zeros(cap, np.uint32)
    for k in rng.permutation(keys).tolist():
        s = int(home_of([k], shift)[0])
        while table[s] != 0:
            s = (s + 1) & (cap - 1)
        table[s] = k
    return table


def simulate(model, union, vote_order=0, spread=True, fast=False, seed=0):
    m, u = model, union
    rng = np.random.default_rng(seed)
    slots = np.zeros((m.n_slices, m.cap, 4), np.uint32)
    for s in range(m.n_slices):
        slots[s, :, 0] = _insert(m.cap, m.shift, m.b_key[m.b_slice == s], rng)
    flat = slots.reshape(-1, 4)
    occ = np.nonzero(flat[:, 0])[0]
    occ = occ[np.lexsort((flat[occ, 0], occ // m.cap))]
    flat[occ, 2] = m.b_len
    padded = (flat[:, 2].astype(np.int64) + 3) & ~3
    flat[:, 1] = np.cumsum(padded) - padded
    flat[occ, 3] = m.b_len | (m.b_force.astype(np.int64) << 31)
    ne = int(padded.sum())
    e4, uv, mi = np.full(ne, SINK, np.uint32), np.zeros((ne, 2), np.uint32), np.zeros(ne, np.uint16)
    place, _ = owned_places(flat[occ, 1], m.b_len)
    shuffle = np.lexsort((rng.random(len(m.b_of)), m.b_of))                   # a random arrival order inside every bucket
    e4[place], uv[place], mi[place] = m.word[shuffle], m.uv[shuffle], m.mi[shuffle]
    o = B.order_buckets(flat[:, 2], flat[:, 0], e4, uv, mi, with_uv=not fast, spread=spread)
    T = dict(cap=m.cap, shift=m.shift, n_slices=m.n_slices, n_entries=ne, num_model_keys=m.num_model_keys, ucap=u.ucap,
             ushift=u.ushift, n_ids=u.n_ids, id_bits=u.id_bits, uinfo_stride=u.stride, kmap_bins=u.kmap_bins,
             reach_words=u.reach_words, has_pw=int(not fast), slots=slots,
             e4=np.concatenate([o[0], np.full(256, SINK, np.uint32)]), mi=o[2])
    if not fast:
        T.update(pw=o[3], puv=o[4].view(np.float32), pdir=o[5])
    ukeys = _insert(u.ucap, u.ushift, u.keys, rng)
    uocc = np.nonzero(ukeys)[0]
    by_key = uocc[np.argsort(ukeys[uocc], kind="stable")]
    if vote_order in (0, 2):
        number = u.rank
    else:
        number = np.empty(u.n_ids, np.uint32)
        number[np.argsort(by_key, kind="stable")] = np.arange(u.n_ids, dtype=np.uint32)
    uids, weights = np.zeros(u.ucap, np.uint32), np.zeros(u.ucap, np.uint64)
    uids[by_key], weights[by_key] = number, u.weights
    kmap = np.where(u.kmap_index >= 0, number[np.maximum(u.kmap_index, 0)] if u.n_ids else 0, KMAP_NONE).astype(np.uint32)
    uinfo = np.zeros((m.n_slices, u.stride, 2), np.uint32)
    nb = number[np.searchsorted(u.keys, m.b_key)]
    uinfo[m.b_slice, nb, 0], uinfo[m.b_slice, nb, 1] = flat[occ, 1], flat[occ, 3]
    T.update(ukeys=ukeys, uids=uids, weights=weights, reach=u.reach.copy(), kmap=kmap, uinfo=uinfo)
    return T
