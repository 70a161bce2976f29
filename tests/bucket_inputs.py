"""Deterministic inputs at the edges of the two orders inside a model's buckets (k_bucket_spread, k_bucket_psort): bucket
lengths around a lane's four registers, a half wave, a chunk of 256, a segment of 4096 and its multiples; words that are
all equal, that tie in P, that tie in the spread key, that sit on the directory's cell edges; the row field's ends; the
launches that leave a kernel out; a slot with key 0.

Every case is a named builder that returns (buckets, flags, prove): `buckets` holds one (words, key) per bucket of the
launch in arrival order (key None = bucket number + 1), flags = dict(with_uv, spread, pad), and prove(launch) asserts
FROM THE RESTATEMENT ALONE (bucket_ref) that the case reaches the edge it is named for.  tests/test_bucket_host.py runs
every prove on a machine without a GPU; tests/test_gpu_bucket_order.py compares the device with the restatement on the
same inputs.  numpy only, seeded."""
import numpy as np

import bucket_ref as R

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257, 259, 260, 511, 512, 513, 1023, 1024, 1025, 4095, 4096,
           4097, 4099, 4100, 4101, 4351, 4352, 4353, 8191, 8192, 8193, 12289]
MAX_LEN = 12289
INV15 = pow(15, -1, 1 << 31)           # word * 30 = P mod 2^32  <=>  word = P / 2 * INV15 mod 2^31 (P is always even)

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def flags(with_uv=True, spread=True, pad=R.ROW_SINK):
    return dict(with_uv=with_uv, spread=spread, pad=pad)


def rnd(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def word_of_p(p):
    """a word whose P is p (p even); the other one is that word ^ 0x80000000"""
    p = np.asarray(p, np.uint64)
    return (((p >> np.uint64(1)) * np.uint64(INV15)) & np.uint64(0x7FFFFFFF)).astype(np.uint32)


# ---------------------------------------------------------------- what a prove looks at
class Launch:
    """a case's arrays, the restatement's answer and, per bucket, its segments"""

    def __init__(self, buckets, fl):
        self.buckets, self.flags = buckets, fl
        self.lens = np.array([len(w) for w, _ in buckets], np.uint32)
        self.keys = np.array([b + 1 if k is None else k for b, (_, k) in enumerate(buckets)], np.uint32)
        self.starts, self.total = R.starts_of(self.lens)
        rng = np.random.default_rng(len(buckets) * 7919 + self.total)
        self.e4 = np.full(self.total, fl["pad"], np.uint32)
        self.uv = rnd(rng, 2 * self.total).reshape(self.total, 2)           # any bits, NaNs included: they are only moved
        self.mi = rng.integers(0, 1 << 16, self.total).astype(np.uint16)
        for b, (w, _) in enumerate(buckets):
            a, n = int(self.starts[b]), len(w)
            self.e4[a:a + n] = w
            self.uv[a:a + n, 0] = (b << 16) | np.arange(n)                   # who an entry is: bucket and arrival index,
            self.mi[a:a + n] = np.arange(n)                                  # in uv and in mi (no bucket is above 2^16)
        self.want = R.order_buckets(self.lens, self.keys, self.e4, self.uv, self.mi, fl["with_uv"], fl["spread"])
        for a in (self.lens, self.keys, self.e4, self.uv, self.mi) + self.want:
            a.setflags(write=False)

    def segments(self, b):
        """(start place, n) of every segment of bucket b"""
        n_b, a = int(self.lens[b]), int(self.starts[b])
        return [(a + s, min(R.SEG, n_b - s)) for s in range(0, n_b, R.SEG)]

    def live(self, b):
        return self.keys[b] != 0 and self.lens[b] > 0

    def Ks(self):
        return {R.cells(n) for b in range(len(self.lens)) if self.live(b) for _, n in self.segments(b)}

    def arrival(self, b):
        """bucket b's entries after the spread: the arrival index of the entry at every position"""
        a, n = int(self.starts[b]), int(self.lens[b])
        return self.want[2][a:a + n].astype(np.int64)


def random_buckets(rng, lens):
    return [(rnd(rng, n), None) for n in lens]


def prove_lengths(L, lens):
    assert L.lens.tolist() == lens
    for b, n in enumerate(lens):
        assert len(L.segments(b)) == (n + R.SEG - 1) // R.SEG
        if n >= 2:                                                          # the spread moves something: not the identity
            assert n < 8 or not np.array_equal(L.arrival(b), np.arange(n))
            assert np.array_equal(np.sort(L.arrival(b)), np.arange(n))


# ---------------------------------------------------------------- lengths
@case
def lengths_up_to_four_chunks():
    rng = np.random.default_rng(11)
    lens = [n for n in LENGTHS if n <= 1025]

    def prove(L):
        prove_lengths(L, lens)
        assert {1, 2, 4, 64, 128, 256, 512} <= L.Ks()
        assert np.all(L.want[5][L.total:] == R.A5_16)                        # nothing behind the last bucket
        a = int(L.starts[lens.index(0)])
        assert a == int(L.starts[lens.index(0) + 1])                         # an empty bucket owns no place
    return random_buckets(rng, lens), flags(), prove


@case
def lengths_around_one_segment():
    rng = np.random.default_rng(12)
    lens = [4095, 4096, 4097, 4099, 4100, 4101, 4351, 4352, 4353]

    def prove(L):
        prove_lengths(L, lens)
        assert [L.segments(b)[-1][1] for b in range(len(lens))] == [4095, 4096, 1, 3, 4, 5, 255, 256, 257]
        assert {1, 2, 4, 128, 256, 2048} <= L.Ks()
    return random_buckets(rng, lens), flags(), prove


@case
def lengths_of_two_and_three_segments():
    rng = np.random.default_rng(13)
    lens = [8191, 8192, 8193, 12289]

    def prove(L):
        prove_lengths(L, lens)
        assert [len(L.segments(b)) for b in range(4)] == [2, 2, 3, 4]
        assert L.segments(3)[-1][1] == 1 and L.segments(2)[-1][1] == 1
        # the second segment is dealt from its own entries alone
        arr = L.arrival(1)
        assert arr[:4096].max() < 4096 <= arr[4096:].min()
    return random_buckets(rng, lens), flags(), prove


@case
def one_bucket():
    rng = np.random.default_rng(14)

    def prove(L):
        assert len(L.lens) == 1 and L.lens[0] == 383 and L.Ks() == {256}
    return random_buckets(rng, [383]), flags(), prove


# ---------------------------------------------------------------- words
@case
def all_words_equal():
    """every order is the index's alone; the directory has every entry in one cell"""
    lens = [1, 2, 5, 129, 257, 4097]
    values = [0, 0xFFFFFFFF, 0x12345678, 0x80000000, 0x7FFFFFFF, 0xDEADBEEF]
    buckets = [(np.full(n, v, np.uint32), None) for n, v in zip(lens, values)]

    def prove(L):
        for b, n in enumerate(lens):
            assert len(np.unique(L.want[0][int(L.starts[b]):int(L.starts[b]) + n])) == 1
            for a, m in L.segments(b):
                K = R.cells(m)
                d = L.want[5][a:a + K + 1].astype(np.int64)
                c = int(R.cell_of(R.p_of([values[b]]), K)[0])
                assert d.tolist() == [0] * (c + 1) + [m] * (K - c)           # one step: at the cell of the word
                # pw keeps the spread's order; the spread keeps the dealing of the arrival order
                assert np.array_equal(L.want[4][a:a + m, 0], L.want[1][a:a + m, 0])
                assert np.array_equal(L.want[1][a:a + m, 0] & 0xFFFF, (a - int(L.starts[b])) + R.spread_segment(np.zeros(m, np.uint32)))
    return buckets, flags(), prove


@case
def ties_in_p():
    """w and w ^ 0x80000000 have one P and differ: their order in pw is the order the spread left them in"""
    rng = np.random.default_rng(21)
    lens = [2, 8, 260, 4100]
    buckets = []
    for n in lens:
        w = rnd(rng, n // 2)
        both = np.concatenate([w, w ^ np.uint32(0x80000000)])
        buckets.append((both[rng.permutation(n)], None))

    def prove(L):
        for b, n in enumerate(lens):
            for a, m in L.segments(b):
                pw, e4 = L.want[3][a:a + m], L.want[0][a:a + m]
                p = R.p_of(pw)
                tie = p[1:] == p[:-1]
                assert tie.sum() >= m // 2 - 2 and np.all(pw[1:][tie] != pw[:-1][tie])
                where = {int(x): i for i, x in enumerate(L.want[1][a:a + m, 0])}     # position after the spread, by identity
                pos = np.array([where[int(x)] for x in L.want[4][a:a + m, 0]])
                assert np.all(pos[1:][tie] > pos[:-1][tie])
                assert np.array_equal(e4[pos], pw)
    return buckets, flags(), prove


@case
def spread_keys_equal_rows_differ():
    """one spread key under 30 different rows: the row term is taken off modulo 2^21, below zero for most of them, and
    the order is the arrival's"""
    rng = np.random.default_rng(22)
    lens = [30, 257, 1000]
    rows_ok = np.array([r for r in range(1023) if r % 32 <= 29])
    buckets = []
    for n in lens:
        c0 = int(rng.integers(0, 1 << 16))
        rows = rows_ok[rng.integers(0, len(rows_ok), n)]
        rows[:30] = rng.permutation(30)
        target = (c0 + (29 << 16) - ((rows % 32) << 16)) % (1 << 21)         # u = ((theta21 * 30) >> 5) that gives the key
        theta21 = (16 * target + 14) // 15
        half = rng.integers(0, 2, n)
        buckets.append(((theta21 << 11 | half << 10 | rows).astype(np.uint32), None))

    def prove(L):
        for b, n in enumerate(lens):
            w = L.buckets[b][0]
            assert len(np.unique(R.spread_key(w))) == 1 and len(np.unique(w & 0x3FF)) >= 30
            u = ((w.astype(np.int64) >> 11) * 30) >> 5
            assert np.count_nonzero(u - (((w.astype(np.int64) & 0x3FF) * 31) << 16) < 0) > n // 2
            assert np.array_equal(L.arrival(b), R.spread_segment(np.zeros(n, np.uint32)))
    return buckets, flags(), prove


@case
def p_on_the_cell_edges():
    """P = 0, P = 2^32 - 30, and P at and just below every k * 2^32 / K of the bucket's own directory"""
    rng = np.random.default_rng(23)
    lens = [2, 4, 8, 10, 260, 4096]
    buckets, edges_of = [], []
    for n in lens:
        K = R.cells(n)
        inner = np.arange(1, K)
        ks = inner if len(inner) <= (n - 2) // 2 else np.unique(np.concatenate([[1, K // 2, K - 1], rng.choice(inner, (n - 2) // 2 - 3)]))
        width = (1 << 32) // K
        p = np.concatenate([[0, (1 << 32) - 30], ks * width, ks * width - 2]).astype(np.uint64)
        w = word_of_p(p)
        w[rng.random(len(w)) < 0.5] ^= np.uint32(0x80000000)                 # either word of the pair: P is the same
        w = np.concatenate([w, rnd(rng, n - len(w))])
        edges_of.append(ks)
        buckets.append((w[rng.permutation(n)], None))

    def prove(L):
        assert L.Ks() == {1, 2, 4, 8, 256, 2048}
        for b, n in enumerate(lens):
            K = R.cells(n)
            width = (1 << 32) // K
            (a, m), = L.segments(b)
            p = R.p_of(L.want[3][a:a + m]).astype(np.int64)
            assert p[0] == 0 and p[-1] == (1 << 32) - 30 and np.all(p[1:] >= p[:-1])
            d = L.want[5][a:a + K + 1].astype(np.int64)
            assert d[0] == 0 and d[K] == n and np.all(d[1:] >= d[:-1])
            ks = edges_of[b]
            assert len(ks) == K - 1 if n in (2, 4, 8, 4096) else {1, K // 2, K - 1} <= set(ks.tolist())
            for k in ks.tolist():                                            # the entry at the edge opens cell k, the one below closes k - 1
                assert p[d[k]] == k * width and p[d[k] - 1] == k * width - 2
    return buckets, flags(), prove


@case
def row_field_ends():
    """rows 0, 1022 and 1023 (the sink row a padding word names), under both halves"""
    rng = np.random.default_rng(24)
    lens = [7, 259, 513]
    buckets = []
    for n in lens:
        rows = np.array([0, 1022, 1023])[rng.integers(0, 3, n)]
        half = rng.integers(0, 2, n)
        rows[:6], half[:6] = [0, 0, 1022, 1022, 1023, 1023], [0, 1, 0, 1, 0, 1]
        theta21 = rng.integers(0, 1 << 21, n)
        buckets.append(((theta21 << 11 | half << 10 | rows).astype(np.uint32), None))

    def prove(L):
        for b in range(len(lens)):
            w = L.buckets[b][0]
            assert {(int(x) & 0x3FF, int(x) >> 10 & 1) for x in w} == {(r, h) for r in (0, 1022, 1023) for h in (0, 1)}
            assert np.array_equal(np.sort(L.want[0][int(L.starts[b]):int(L.starts[b]) + len(w)]), np.sort(w))
    return buckets, flags(), prove


# ---------------------------------------------------------------- other settings
SETTING_LENS = [0, 1, 3, 5, 130, 258, 1000, 4097]


@case
def fast_mode_has_no_second_order():
    rng = np.random.default_rng(31)

    def prove(L):
        assert np.all(L.want[3] == R.A5_32) and np.all(L.want[4] == R.A5_32) and np.all(L.want[5] == R.A5_16)
        assert not np.array_equal(L.want[0], L.e4) and not np.array_equal(L.want[2], L.mi)   # the spread still runs
        assert np.array_equal(L.want[1], L.uv)                               # on e4 and mi: there is no uv to move
    return random_buckets(rng, SETTING_LENS), flags(with_uv=False), prove


@case
def no_spread():
    rng = np.random.default_rng(32)

    def prove(L):
        assert all(np.array_equal(w, g) for w, g in zip(L.want[:3], (L.e4, L.uv, L.mi)))
        assert L.Ks() == {1, 2, 4, 128, 256, 512, 2048}
        for b in range(len(L.lens)):
            for a, m in L.segments(b):                                       # the second order of the arrival order
                assert np.array_equal(L.want[3][a:a + m], L.e4[a:a + m][np.argsort(R.p_of(L.e4[a:a + m]), kind="stable")])
    return random_buckets(rng, SETTING_LENS), flags(spread=False), prove


@case
def nothing_launched():
    rng = np.random.default_rng(33)

    def prove(L):
        assert all(np.array_equal(w, g) for w, g in zip(L.want[:3], (L.e4, L.uv, L.mi)))
        assert np.all(L.want[3] == R.A5_32) and np.all(L.want[5] == R.A5_16)
    return random_buckets(rng, [2, 300]), flags(with_uv=False, spread=False), prove


@case
def slots_with_key_zero():
    """a slot with key 0 is skipped whatever its length; so is a keyed slot of length 0; their neighbours are not"""
    rng = np.random.default_rng(34)
    lens = [9, 300, 0, 4100, 6, 1, 0, 2]
    keys = [None, 0, 0, 0, 77, 0, 5, None]
    buckets = [(rnd(rng, n), k) for n, k in zip(lens, keys)]

    def prove(L):
        for b, k in enumerate(keys):
            a, n = int(L.starts[b]), int(L.lens[b])
            pad = ((n + 3) & ~3)
            if k == 0:
                assert np.array_equal(L.want[0][a:a + pad], L.e4[a:a + pad]) and np.array_equal(L.want[2][a:a + pad], L.mi[a:a + pad])
                assert np.all(L.want[3][a:a + pad] == R.A5_32) and np.all(L.want[5][a:a + pad] == R.A5_16)
            elif n:
                assert np.all(L.want[3][a:a + n] != R.A5_32) and L.want[5][a] == 0
        assert not np.array_equal(L.want[0], L.e4)
    return buckets, flags(), prove


@case
def padding_words_are_kept():
    """padding words that are not the sink row's come back as they went up, behind every bucket"""
    rng = np.random.default_rng(35)
    lens = [1, 2, 3, 5, 7, 9, 4097, 4099, 259]

    def prove(L):
        n_pad = 0
        for b, n in enumerate(lens):
            a = int(L.starts[b])
            for q in range(a + n, a + ((n + 3) & ~3)):
                n_pad += 1
                assert L.want[0][q] == 0xDEAD07FE and L.want[3][q] == R.A5_32 and np.all(L.want[4][q] == R.A5_32)
                assert np.array_equal(L.want[1][q], L.uv[q]) and L.want[2][q] == L.mi[q]
        assert n_pad == 3 + 2 + 1 + 3 + 1 + 3 + 3 + 1 + 1
        assert not np.any(L.want[0][L.e4 != 0xDEAD07FE] == 0xDEAD07FE)
    return random_buckets(rng, lens), flags(pad=0xDEAD07FE), prove


# ---------------------------------------------------------------- a launch's arrays
_REFS = {}


def reference(name):
    """-> (Launch, prove): the case's arrays and the restatement's answer, computed once per process and never changed"""
    if name not in _REFS:
        buckets, fl, prove = CASES[name]()
        _REFS[name] = (Launch(buckets, fl), prove)
    return _REFS[name]
