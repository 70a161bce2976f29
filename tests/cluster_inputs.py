"""Made-up pose sets for the pose tail's clustering (plain numpy, no fixtures): peak records whose poses land in
chosen translation cells with chosen rotations, counts and weights, so that every path of k_cluster_scores and of the
chain around it is reached on purpose.

A peak record is (scene ref << 32 | model ref << 6 | alpha, count); its pose is Ts^-1 * Rx(alpha) * Tm.  Every model
point and every scene point has the same normal here, so the rotation depends on alpha alone, and the translation of
(scene point s, model point m, alpha) is s + t0[m, alpha] with t0 measured once through the oracle (model point 0 lies
at the origin: t0[0, :] ~ 0).  One scene point per pose; scene point 0 is a dummy unless the all-zero code is asked for.

The builder never trusts its aim: reference_side() takes the real poses, translations and quaternions from the oracle
(trans_calc2, mat2transquat), derives cells, hashes and the sorted (hash, index) list from those, checks its numpy FNV
against the oracle's, and every case asserts the property it is named for from that data alone."""
import ctypes as C

import numpy as np

import cluster_ref as R

F = np.float32
M = 64
NORMAL = (np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])).astype(F)
CELL_DTYPE = np.dtype([("code", "<u8"), ("count", "<u4"), ("pad", "<u4")])
WAVE = 64


def model_cloud():
    rng = np.random.default_rng(7)
    mp = rng.uniform(-0.5, 0.5, (M, 3)).astype(F)
    mp[0] = 0
    return mp, np.tile(NORMAL, (M, 1)).astype(F)


_T0 = {}


def base_offsets(oracle):
    """t0[m, alpha]: the translation of (scene point at the origin, model point m, alpha), from the oracle"""
    if "t0" not in _T0:
        mp, mn = model_cloud()
        sp, sn = np.zeros((2, 3), F), np.tile(NORMAL, (2, 1)).astype(F)
        cells = np.zeros(M * 64, CELL_DTYPE)
        cells["code"] = (np.uint64(1) << np.uint64(32)) | np.arange(M * 64, dtype=np.uint64)
        cells["count"] = 1
        T = oracle.trans_calc2(cells, mp, mn, sp, sn)
        _T0["t0"] = T[:, [3, 7, 11]].astype(np.float64).reshape(M, 64, 3)
    return _T0["t0"]


def cell_point(c, frac, d):
    """a coordinate in cell c at the fraction frac of its width; the cell index truncates toward zero, so cell 0 is
    (-d, d) and cell c < 0 is ((c - 1) d, c d]"""
    if c > 0:
        return (c + frac) * d
    if c < 0:
        return (c - 1 + frac) * d
    return (2 * frac - 1) * d


class Builder:
    def __init__(self, oracle, d_dist=0.1, weights=None, use_l1=False, two_sorts=False, zero_at=None, mix=False):
        self.oracle, self.d = oracle, float(F(d_dist))
        self.weights = np.ones(M, F) if weights is None else np.asarray(weights, F).copy()
        self.use_l1, self.two_sorts, self.mix = bool(use_l1), bool(two_sorts), bool(mix)
        self.t0 = base_offsets(oracle)
        # scene point 0: a dummy far from everything, or where the all-zero code's pose WOULD land if it got one
        self.sp = [np.array([900.0, 900.0, 900.0]) * self.d if zero_at is None else self.xyz(*zero_at)]
        self.rec = []
        self.aim = {}                       # scene ref -> aimed cell

    def xyz(self, cell, frac=(0.5, 0.5, 0.5)):
        return np.array([cell_point(int(c), float(f), self.d) for c, f in zip(cell, frac)], np.float64)

    def add(self, cell, frac=(0.5, 0.5, 0.5), m=0, alpha=0, count=1):
        """one pose aimed at `cell`; returns its scene reference (its code's high word)"""
        s = len(self.sp)
        if self.mix and m == 0 and len(self.rec) % 3 == 1:
            m = 1                               # every third pose belongs to the model point with the fractional weight
        self.sp.append(self.xyz(cell, frac) - self.t0[m, alpha])
        self.rec.append(((s << 32) | (m << 6) | alpha, count))
        self.aim[s] = tuple(int(c) for c in cell)
        return s

    def add_at(self, xyz, m=0, alpha=0, count=1):
        s = len(self.sp)
        self.sp.append(np.asarray(xyz, np.float64) - self.t0[m, alpha])
        self.rec.append(((s << 32) | (m << 6) | alpha, count))
        return s

    def add_zero_code(self, count=1):
        self.rec.append((0, count))

    def finish(self, name, gmax=None):
        mp, mn = model_cloud()
        sp = np.asarray(self.sp, np.float64).astype(F)
        rec = np.zeros(len(self.rec), CELL_DTYPE)
        rec["code"] = [r[0] for r in self.rec]
        rec["count"] = [r[1] for r in self.rec]
        rec = rec[np.random.default_rng(len(rec)).permutation(len(rec))]        # the tails must order them themselves
        case = dict(name=name, mp=mp, mn=mn, sp=sp, sn=np.tile(NORMAL, (len(sp), 1)).astype(F), records=rec,
                    gmax=int(gmax if gmax is not None else rec["count"].max()), d=self.d, weights=self.weights,
                    use_l1=self.use_l1, two_sorts=self.two_sorts, aim=self.aim, thresh=0.0)
        case["ref"] = reference_side(self.oracle, case)
        return case


def reference_side(oracle, case):
    """kept cells in order, poses, translations, quaternions, cells, hashes, weighted votes, the sorted list"""
    rec, d = case["records"], case["d"]
    keep = rec["count"].astype(F) > F(case["thresh"]) * F(case["gmax"])                       # model.cu:164-167
    kept = rec[keep]
    kept = kept[np.lexsort((kept["code"], -kept["count"].astype(np.int64)))]                   # count desc, code asc
    n = len(kept)
    T = oracle.trans_calc2(kept, case["mp"], case["mn"], case["sp"], case["sn"])
    trans, quat = oracle.mat2transquat(T)
    cell = R.trans_cells(trans, d)
    h = R.fnv_cells(cell)
    # the numpy cells and FNV against the oracle's K8 (hash of every pose's cell and of its 27 neighbours)
    th, adj = np.zeros(n, np.uint32), np.zeros((n, 27), np.uint32)
    oracle.lib().orc_trans2idx(trans.ctypes.data_as(C.c_void_p), n, C.c_float(d), th.ctypes.data_as(C.c_void_p),
                               adj.ctypes.data_as(C.c_void_p))
    assert np.array_equal(th, h), "numpy cells / FNV differ from the oracle"
    probe = np.unique(np.linspace(0, n - 1, min(n, 64)).astype(int))
    for i in probe:
        assert np.array_equal(adj[i], R.neighbour_hashes(cell[i])), "numpy neighbour hashes differ from the oracle"
    if n:
        assert oracle.hash_bytes(cell[0].tobytes()) == int(h[0])
    m_r = ((kept["code"] & np.uint64(0xFFFFFFFF)) >> np.uint64(6)).astype(np.int64)
    wv = case["weights"][m_r] * kept["count"].astype(F)                                        # kernel.cu:777
    order = np.lexsort((np.arange(n), h))                                                      # (hash, index) ascending
    return dict(kept=kept, T=T, trans=trans, quat=quat, cell=cell, hash=h, wv=wv.astype(F), order=order,
                lists=R.hash_lists(h), s_ref=(kept["code"] >> np.uint64(32)).astype(np.int64),
                alpha=(kept["code"] & np.uint64(63)).astype(np.int64), m_r=m_r)


# ---- what the kernels will meet, computed from the reference side ----
def index_of(ref, s):
    """pose index of the record with scene reference s"""
    (i,) = np.nonzero(ref["s_ref"] == s)[0]
    return int(i)


def list_lens(ref, i):
    return R.candidates(ref, i)[1]


def windows(lens):
    """the 64-position windows of a candidate list with the 27 per-lane lengths `lens`: per window the number of
    cells it spans and whether it ends exactly on a cell's end"""
    incl = np.cumsum(lens)
    total = int(incl[-1])
    out = []
    for b in range(0, total, WAVE):
        e = min(b + WAVE, total)
        c0 = int(np.searchsorted(incl, b, side="right"))
        c1 = int(np.searchsorted(incl, e - 1, side="right"))
        spans = len([c for c in range(c0, c1 + 1) if lens[c] > 0])
        out.append(dict(one_cell=b + WAVE <= incl[c0], spans=spans, ends_on_cell=bool(e == incl[c1]), full=e - b == WAVE))
    return out


def whole_mode(ref):
    """weighted votes all whole numbers in [0, 2^24) with a sum below 2^24 - 1: lane-parallel sums, shared walks"""
    w = ref["wv"].astype(np.float64)
    ok = np.all((w >= 0) & (w < 2 ** 24) & (w == np.floor(w)))
    return bool(ok and w.sum() < 2 ** 24 - 1)


def wave_groups(ref, whole=None):
    """per wave of four sorted positions: the sizes G of the groups that share a walk"""
    whole = whole_mode(ref) if whole is None else whole
    o, h, cell = ref["order"], ref["hash"], ref["cell"]
    n, out = len(o), []
    for p0 in range(0, n, 4):
        g0, wave = 0, []
        while g0 < 4 and p0 + g0 < n:
            G = 1
            a = o[p0 + g0]
            while whole and g0 + G < 4 and p0 + g0 + G < n:
                b = o[p0 + g0 + G]
                if h[b] != h[a] or not np.array_equal(cell[b], cell[a]):
                    break
                G += 1
            wave.append(G)
            g0 += G
        out.append(tuple(wave))
    return out


def table_cap(n):
    cap = 64
    while cap < 2 * max(n, 1):
        cap <<= 1
    return cap


def home_slots(hashes, n):
    """cell_slot of every hash in the table that n poses get"""
    h = np.asarray(hashes, np.uint64)
    return ((h * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.int64) & (table_cap(n) - 1)


def aimed_cells_hit(case):
    """every pose landed in the cell it was aimed at"""
    ref = case["ref"]
    for i, s in enumerate(ref["s_ref"].tolist()):
        if s in case["aim"] and tuple(int(v) for v in ref["cell"][i]) != case["aim"][s]:
            return False
    return True


LANE = {v: k for k, v in enumerate(R.NEIGHBOURS)}


def toward(delta):
    """fraction inside the neighbour cell at offset delta (-1, 0, 1) that lies close to the centre cell's middle"""
    return 0.5 - 0.46 * delta


# =====================================================================================================================
# The cases.  Each returns a finished case whose structural property has been asserted from case["ref"].
# `w` names the weights: "one" (all 1: whole mode) or "frac" (one model point weighs 1.1: sequential mode, see _weights).
# =====================================================================================================================
def _weights(w):
    """"one": every weight 1.  "frac": model point 1 weighs 1.1, the others 1, and the builder gives every third pose to
    model point 1 -- one fractional weight makes the whole set sequential, and 1.1 is no dyadic fraction, so the float
    sums round and depend on their order"""
    wts = np.ones(M, F)
    if w == "frac":
        wts[1] = 1.1
    return wts


def _fill(b, cell, k, alphas=(10, 11, 12, 10, 40), counts=(1, 2, 3, 1, 5), frac=None, m=0, jitter=True):
    """k poses in `cell`, near the fraction frac, with cycling alphas and counts"""
    out = []
    frac = (0.5, 0.5, 0.5) if frac is None else frac
    for j in range(k):
        f = tuple(min(max(x + (0.02 * ((j * (a + 3)) % 5 - 2) / 5 if jitter else 0), 0.01), 0.99) for a, x in enumerate(frac))
        out.append(b.add(cell, f, m=m, alpha=alphas[j % len(alphas)], count=counts[j % len(counts)]))
    return out


def case_ragged(oracle, n, w="one"):
    """n poses in two adjacent cells: the last wave of four takes n % 4 positions"""
    b = Builder(oracle, weights=_weights(w), mix=w == "frac")
    for j in range(n):
        b.add((2 + j % 2, 2, 2), (0.9 - 0.8 * (j % 2), 0.5, 0.5), alpha=10 + j % 3, count=1 + j % 4)
    c = b.finish("ragged_%d_%s" % (n, w))
    assert len(c["ref"]["kept"]) == n and aimed_cells_hit(c)
    assert whole_mode(c["ref"]) == (w == "one")
    assert sum(wave_groups(c["ref"])[-1]) == (n % 4 or 4)
    assert max(int(list_lens(c["ref"], i).sum()) for i in range(n)) > 0
    return c


def case_isolated(oracle, every, w="one"):
    """one pose far from a small cluster (list total 0), or nothing but isolated poses"""
    b = Builder(oracle, weights=_weights(w), mix=w == "frac")
    if not every:
        _fill(b, (2, 2, 2), 3, frac=(0.9, 0.5, 0.5))
        _fill(b, (3, 2, 2), 4, frac=(0.1, 0.5, 0.5))
    lone = [b.add((10 + 3 * j, 5, -4 - 3 * (j % 3)), count=2 + j) for j in range(9 if every else 1)]
    c = b.finish("isolated_%s_%s" % ("all" if every else "one", w))
    ref = c["ref"]
    assert aimed_cells_hit(c)
    for s in lone:
        assert list_lens(ref, index_of(ref, s)).sum() == 0
    if every:
        assert all(list_lens(ref, i).sum() == 0 for i in range(len(ref["kept"])))
    return c


def case_list_length(oracle, L, w="one"):
    """cells A and B side by side: a pose of A walks exactly len(B) = L candidates"""
    b = Builder(oracle, weights=_weights(w), mix=w == "frac")
    a = _fill(b, (4, 3, 2), 3, frac=(0.9, 0.5, 0.5))
    _fill(b, (5, 3, 2), L, frac=(0.1, 0.5, 0.5), alphas=(10, 11, 12, 13, 10, 40, 11), counts=(1, 2, 3, 4, 1, 7))
    c = b.finish("list_%d_%s" % (L, w))
    ref = c["ref"]
    assert aimed_cells_hit(c)
    for s in a:
        lens = list_lens(ref, index_of(ref, s))
        assert lens.sum() == L and lens[LANE[(1, 0, 0)]] == L
    return c


def _around(b, centre, lens_by_lane, k_centre=1, alphas=(10, 11, 12, 10, 40)):
    """k_centre poses in the middle of `centre` and lens_by_lane[lane] poses in each neighbour cell, near the centre"""
    mid = _fill(b, centre, k_centre, alphas=alphas)
    for lane, k in lens_by_lane.items():
        dx, dy, dz = R.NEIGHBOURS[lane]
        _fill(b, (centre[0] + dx, centre[1] + dy, centre[2] + dz), k, frac=(toward(dx), toward(dy), toward(dz)), alphas=alphas,
              counts=(1, 2, 1, 3))
    return mid


def case_windows(oracle, kind, w="one"):
    """candidate lists whose 64-position windows straddle two and three cells / end exactly on cell ends / a full
    3x3x3 block with lanes 0 and 26 longer than the rest"""
    b = Builder(oracle, weights=_weights(w), mix=w == "frac")
    if kind == "straddle":
        want = {0: 3, 1: 70, 2: 1, 3: 130, 26: 5}
    elif kind == "exact":
        want = {0: 64, 1: 128, 2: 64}
    elif kind == "short":
        want = {0: 63, 1: 64, 2: 9}          # the first two windows hold 63 positions of their cell and ONE of the next
    else:
        want = {lane: 3 for lane in range(27) if lane != 13}
        want[0], want[26] = 7, 9
    mid = _around(b, (6, 6, 6), want, k_centre=5 if kind == "block" else 1)
    c = b.finish("windows_%s_%s" % (kind, w))
    ref = c["ref"]
    assert aimed_cells_hit(c)
    lens = list_lens(ref, index_of(ref, mid[0]))
    assert {k: int(v) for k, v in enumerate(lens) if v} == want
    win = windows(lens)
    if kind == "straddle":
        assert {x["spans"] for x in win} >= {2, 3} and not any(x["one_cell"] for x in win[:1])
    elif kind == "exact":
        # all four windows lie in one cell each, and three of them end exactly where their cell ends: b + 64 == incl[c0]
        assert len(win) == 4 and all(x["one_cell"] and x["full"] for x in win) and sum(x["ends_on_cell"] for x in win) == 3
    elif kind == "short":
        incl = np.cumsum(lens)
        assert [int(incl[np.searchsorted(incl, b0, side="right")]) - b0 for b0 in (0, 64)] == [63, 63]
        assert not win[0]["one_cell"] and not win[1]["one_cell"] and win[0]["spans"] == 2
    else:
        assert (lens[np.arange(27) != 13] > 0).all() and lens[0] == 7 and lens[26] == 9 and lens[13] == 0
    return c


def case_groups(oracle, w="one"):
    """cells in hash order with 4 | 1,3 | 3,1 | 2,2 | 1,1,1,1 | 5,3 | 9,3 poses: the waves of four see every split"""
    pool = [(3 * i + 1, 3 * j + 1, 2) for i in range(3) for j in range(3)]
    pairs = [(c, (c[0] + 1, c[1], c[2])) for c in pool]                       # every cell has a populated neighbour
    cells = [c for p in pairs for c in p]
    order = np.argsort(R.fnv_cells(np.asarray(cells, np.int32)), kind="stable")
    sizes = [4, 1, 3, 3, 1, 2, 2, 1, 1, 1, 1, 5, 3, 9, 3]
    b = Builder(oracle, weights=_weights(w), mix=w == "frac")
    for k, ci in enumerate(order[: len(sizes)]):
        cell = cells[int(ci)]
        left = int(ci) % 2 == 0
        _fill(b, cell, sizes[k], frac=(0.93 if left else 0.07, 0.5, 0.5), alphas=(10, 12, 11, 10, 15, 41, 13), counts=(1, 2, 3, 1, 4))
    c = b.finish("groups_%s" % w)
    ref = c["ref"]
    assert aimed_cells_hit(c) and (ref["hash"] != 0).all()
    g = set(wave_groups(ref))
    if w == "one":
        assert whole_mode(ref) and g >= {(4,), (1, 3), (3, 1), (2, 2), (1, 1, 1, 1)}
    else:
        assert not whole_mode(ref) and g <= {(1, 1, 1, 1), (1, 1, 1), (1, 1), (1,)}
        assert set(wave_groups(ref, whole=True)) >= {(4,), (1, 3), (3, 1), (2, 2)}      # the same layout would share walks
    assert max(int(list_lens(ref, i).sum()) for i in range(len(ref["kept"]))) >= 3
    return c


def case_order_sensitive(oracle):
    """weights over 1e-3..1e4: one pose's compatible neighbours add up differently in any other order"""
    for seed in range(11, 40):                            # the first draw whose reversed sum differs (asserted below)
        rng = np.random.default_rng(seed)
        wts = np.ones(M, F)
        wts[1:] = (10.0 ** rng.uniform(-3, 4, M - 1)).astype(F)
        b = Builder(oracle, weights=wts)
        p = b.add((4, 4, 4), (0.9, 0.5, 0.5), alpha=10, count=3)
        for j in range(48):
            b.add((5, 4, 4), (0.1, 0.5, 0.5), m=1 + j, alpha=10 + j % 2, count=1 + (j * 7) % 5)
        c = b.finish("order_sensitive")
        ref = c["ref"]
        i = index_of(ref, p)
        cand, lens = R.candidates(ref, i)
        ok = R.compatible(ref, i, cand, c["d"], False)
        v = ref["wv"][cand[ok]]
        if R.seq_sum(1, v) != R.seq_sum(1, v[::-1]):
            break
    assert lens.sum() == 48 and ok.sum() >= 40 and not whole_mode(ref)
    assert R.seq_sum(1, v) != R.seq_sum(1, v[::-1]), "the reversed sum must differ"
    assert float(ref["wv"].min()) < 1e-2 and float(ref["wv"].max()) > 1e3
    return c


def case_vote_total(oracle, total):
    """whole weighted votes whose sum is `total`: 2^24 - 2 is still whole mode, 2^24 - 1 and 2^24 are not"""
    b = Builder(oracle)
    small = [1, 2, 3, 1, 1, 2, 5, 1]
    a = _fill(b, (4, 4, 4), 3, frac=(0.9, 0.5, 0.5), alphas=(10,), counts=(1, 2, 1))
    for j, k in enumerate(small):
        b.add((5, 4, 4), (0.1, 0.5, 0.5), alpha=10 + j % 2, count=k)
    big = b.add((5, 4, 4), (0.1, 0.45, 0.5), alpha=10, count=total - 4 - sum(small))
    c = b.finish("vote_total_%d" % total)
    ref = c["ref"]
    assert aimed_cells_hit(c) and int(ref["wv"].astype(np.float64).sum()) == total
    assert whole_mode(ref) == (total < 2 ** 24 - 1)
    for s in a:                                           # the poses of the first cell count the large vote
        i = index_of(ref, s)
        cand, _ = R.candidates(ref, i)
        assert index_of(ref, big) in cand[R.compatible(ref, i, cand, c["d"], False)]
    return c


def case_sum_bound(oracle):
    """Only the SUM decides the mode here: every weighted vote is a whole number below 2^24 (the not-whole flag stays
    clear), their total lies well past 2^24, and all of one cell's are compatible with one pose, whose sequential sum
    passes 2^24 and stalls there -- any other order of adding (the lane-parallel one included) gives other bits"""
    b = Builder(oracle)
    p = b.add((4, 4, 4), (0.9, 0.5, 0.5), alpha=10, count=2)
    b.add((5, 4, 4), (0.1, 0.5, 0.5), alpha=10, count=2 ** 24 - 8)
    b.add((5, 4, 4), (0.1, 0.5, 0.5), alpha=11, count=2 ** 23 + 3)
    for j in range(70):
        b.add((5, 4, 4), (0.1, 0.5, 0.5), alpha=10 + j % 2, count=1)        # past 2^24 a float steps by 2: adding 1 stalls
    c = b.finish("sum_bound")
    ref = c["ref"]
    i = index_of(ref, p)
    cand, lens = R.candidates(ref, i)
    v = ref["wv"][cand[R.compatible(ref, i, cand, c["d"], False)]]
    w = ref["wv"].astype(np.float64)
    assert aimed_cells_hit(c) and len(v) == 72 and lens.sum() == 72
    assert ((w >= 0) & (w < 2 ** 24) & (w == np.floor(w))).all() and w.sum() > 2 ** 24 + 2 ** 23 and not whole_mode(ref)
    fwd, rev = R.seq_sum(1, v), R.seq_sum(1, v[::-1])
    pairwise = F(1) + np.add.reduce(v.reshape(-1, 8).sum(axis=1, dtype=F), dtype=F)
    assert fwd > 2 ** 24 and fwd != rev and fwd != pairwise and fwd != F(1 + v.astype(np.float64).sum())
    return c


def case_big_weight(oracle, negative=False):
    """one weighted vote of 2^24 among ones, placed so that the partial sums pass 2^24 and the order shows; or one
    negative weight"""
    wts = np.ones(M, F)
    wts[2] = -2.0 if negative else 2.0 ** 24
    b = Builder(oracle, weights=wts)
    p = b.add((4, 4, 4), (0.9, 0.5, 0.5), alpha=10, count=3)
    b.add((4, 4, 4), (0.9, 0.52, 0.5), alpha=11, count=3)
    for j in range(2):
        b.add((5, 4, 4), (0.1, 0.5, 0.5), alpha=10, count=2)
    for j in range(9):                                    # count 1: index order = order of adding
        b.add((5, 4, 4), (0.1, 0.5, 0.5), m=2 if j == 3 else 0, alpha=10 + j % 2, count=1)
    c = b.finish("negative_weight" if negative else "big_weight")
    ref = c["ref"]
    i = index_of(ref, p)
    cand, _ = R.candidates(ref, i)
    v = ref["wv"][cand[R.compatible(ref, i, cand, c["d"], False)]]
    assert not whole_mode(ref) and len(v) == 11
    if negative:
        assert v.min() < 0
    else:
        assert v.max() >= 2 ** 24 and R.seq_sum(1, v) != R.seq_sum(1, v[::-1]) and R.seq_sum(1, v) > 2 ** 24
    return c


def case_rotation(oracle, use_l1=False):
    """alphas 1..5 and 32 bins away from a pose's own, on both sides of the rotation threshold; and the all-zero code
    with neighbours around the origin: its pose is the zero matrix, not the pose of (scene 0, model 0, alpha 0)"""
    b = Builder(oracle, use_l1=use_l1, zero_at=((8, 8, 8), (0.9, 0.5, 0.5)))
    p = b.add((4, 4, 4), (0.9, 0.5, 0.5), alpha=10, count=2)
    diffs = [0, 1, 2, 3, 4, 5, -1, -2, -3, -4, -5, 30, 32]
    for k in diffs:
        b.add((5, 4, 4), (0.1, 0.5, 0.5), alpha=10 + k, count=1 + abs(k))
    # the quaternion is made with w >= 0, so its sign turns over where the pose's angle passes pi: there one alpha step
    # is rejected although the rotations are 12 degrees apart
    p2 = b.add((4, 8, 4), (0.9, 0.5, 0.5), alpha=0, count=2)
    for a in (0, 1, 2, 29, 30, 31, 59):
        b.add((5, 8, 4), (0.1, 0.5, 0.5), alpha=a, count=3)
    # a cluster where scene point 0 lies: the zero code's pose must not join it
    _fill(b, (8, 8, 8), 3, frac=(0.9, 0.5, 0.5), alphas=(0,))
    beside = _fill(b, (9, 8, 8), 3, frac=(0.1, 0.5, 0.5), alphas=(0,))
    b.add_zero_code(count=4)
    for cell in ((1, 0, 0), (-1, 0, 0), (0, 1, 1), (-1, -1, -1), (0, 0, 0), (1, 1, 0)):
        _fill(b, cell, 2, frac=tuple(toward(v) if v else 0.5 for v in cell), alphas=(10, 26))
    c = b.finish("rotation_%s" % ("l1" if use_l1 else "l2"))
    ref = c["ref"]
    i = index_of(ref, p)
    cand, _ = R.candidates(ref, i)
    ok = R.compatible(ref, i, cand, c["d"], True)
    d_alpha = ref["alpha"][cand] - 10
    inside = {int(k) for k in np.abs(d_alpha[ok])}
    outside = {int(k) for k in np.abs(d_alpha[~ok])}
    # 30 bins are a full turn: the same rotation and the same quaternion
    assert len(cand) == len(diffs) and 0 in inside and 5 in outside and 4 in outside and 30 in inside and 32 in (inside | outside)
    edge = max(k for k in inside if k < 10)
    assert edge + 1 in outside and edge >= 1, "the set holds the last alpha step inside the threshold and the first outside"
    i2 = index_of(ref, p2)
    cand2, _ = R.candidates(ref, i2)
    ok2 = R.compatible(ref, i2, cand2, c["d"], True)
    flipped = [int(a) for a, good in zip(ref["alpha"][cand2], ok2) if not good and a in (1, 29, 31, 59)]
    assert len(cand2) == 7 and flipped, "one alpha step across the sign change is rejected"
    z = index_of(ref, 0)
    assert not ref["T"][z].any() and not ref["cell"][z].any() and np.array_equal(ref["quat"][z], np.full(4, 0.5, F))
    assert list_lens(ref, z).sum() >= 8
    near = R.trans_cells(c["sp"][:1], c["d"])[0]
    assert tuple(near) == (8, 8, 8)                       # where a pose computed for the zero code would have landed ...
    for s in beside:                                      # ... with the alpha of the poses next door, which would count it
        k = index_of(ref, s)
        assert ref["alpha"][k] == 0 and tuple(ref["cell"][k]) == (9, 8, 8)
    return c


def threshold_kind(d_dist):
    """how the smallest float whose root reaches d_dist lies to fl(d_dist * d_dist): -1 below, 0 equal, 1 above"""
    d = F(d_dist)
    x = F(d * d)
    while np.sqrt(x) >= d:
        x = np.nextafter(x, F(0))
    while np.sqrt(x) < d:
        x = np.nextafter(x, F(np.inf))
    return int(np.sign(int(x.view(np.uint32)) - int(F(d * d).view(np.uint32)))), x


def case_distance(oracle, d_dist, use_l1=False):
    """200 pairs across a cell face next to the origin, about d_dist * (1 + k 2^-24) apart: two poses A in one cell, a hundred
    poses B in the next; every B walks just the two A, so each pair's comparison shows in a score of its own"""
    b = Builder(oracle, d_dist=d_dist, use_l1=use_l1)
    d = b.d
    y = cell_point(1, 0.5, d)
    xa = [1.7 * d, 1.7 * d + d * 2.0 ** -25]
    sa = [b.add_at((x, y, y - j * d * np.sqrt(0.31e-7)), count=3 + j) for j, x in enumerate(xa)]
    sb = []
    for idx in range(100):
        # translations near 0.2 move in steps of their own ulp, a few ulp of the squared distance apart: a small offset
        # across (z) fills the gaps between the separations d (1 + k 2^-24), k = -5 .. 4
        k, j = idx // 10 - 5, idx % 10
        sb.append(b.add_at((xa[0] + d * (1 + k * 2.0 ** -24), y, y + d * np.sqrt(j * 0.7e-7)), count=1 + idx % 2))
    c = b.finish("distance_%g_%s" % (d_dist, "l1" if use_l1 else "l2"))
    ref = c["ref"]
    _, thr = threshold_kind(d)
    ulps = []
    for s in sb:
        ib = index_of(ref, s)
        assert tuple(ref["cell"][ib]) == (2, 1, 1) and list_lens(ref, ib).sum() == 2
        for s2 in sa:
            ia = index_of(ref, s2)
            assert tuple(ref["cell"][ia]) == (1, 1, 1)
            e = ref["trans"][ib] - ref["trans"][ia]
            d2 = F(F(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            ulps.append(int(d2.view(np.uint32)) - int(thr.view(np.uint32)))
    ulps = np.asarray(ulps)
    assert len(ulps) == 200
    # where the threshold lies below fl(d^2), some pair lands between the two: d_dist * d_dist would accept it
    gap = int(F(F(d) * F(d)).view(np.uint32)) - int(thr.view(np.uint32))
    assert gap == 0 or ((ulps >= 0) & (ulps < gap)).any(), "no pair between the threshold and fl(d^2)"
    assert ((ulps >= -2) & (ulps < 0)).any() and ((ulps >= 0) & (ulps <= 2)).any(), "squared distances within 2 ulp on both sides"
    c["ulps"] = ulps
    return c


def pick_distances():
    """d_dist values by where the smallest float whose root reaches d_dist lies: below fl(d_dist^2) or on it.  It
    never lies above: fl(d^2) = d^2 (1 + e) with |e| <= 2^-24, its root is d (1 + e/2 + ...) and |e/2| d <= 2^-25 d is
    less than half an ulp of d, so the correctly rounded root of fl(d^2) is d itself and the threshold is at most
    fl(d^2).  Checked here for every candidate; the cases take one value on the product and two below it."""
    kinds = {float(F(v)): threshold_kind(F(v))[0] for v in (0.1, 0.25, 0.3, 1.0 / 3.0, 0.7)}
    assert set(kinds.values()) == {-1, 0}, kinds
    picked = [float(F(0.1)), float(F(0.25)), float(F(1.0 / 3.0))]
    assert [kinds[v] for v in picked] == [-1, 0, -1]
    return picked


ZERO_HASH_CELLS = [(-170, 60, -17), (460, -367, 7), (818, -403, 7)]
COLLISIONS = [((3, 2, 1), (1332, 271, -855)), ((0, 0, 1), (355, -512, -1154))]


def case_zero_hash(oracle, w="one"):
    """a pose whose own cell hashes to 0, with populated neighbours, and a zero-hash cell next to a cluster: such a cell
    is never entered and never searched -- its poses score, and nobody counts them"""
    assert (R.fnv_cells(np.asarray(ZERO_HASH_CELLS, np.int32)) == 0).all()
    b = Builder(oracle, weights=_weights(w), mix=w == "frac")
    z = []
    for zc in ZERO_HASH_CELLS[:2]:
        z += _fill(b, zc, 3, alphas=(10, 11))
        _around(b, zc, {12: 4, 14: 3, 4: 2, 22: 70}, k_centre=0, alphas=(10, 11))
    c = b.finish("zero_hash_%s" % w)
    ref = c["ref"]
    assert aimed_cells_hit(c)
    for s in z:
        i = index_of(ref, s)
        lens = list_lens(ref, i)              # (0, 0, -1) of one zero-hash cell shares its hash with the other's: 4 + 4
        assert ref["hash"][i] == 0 and lens[LANE[(1, 0, 0)]] == 70 and lens.sum() in (79, 83)
    for i in np.nonzero(ref["hash"] != 0)[0]:
        cand, _ = R.candidates(ref, int(i))
        assert (ref["hash"][cand] != 0).all()
    return c


def case_collision(oracle, use_l1, own=False, w="one"):
    """two far-apart cells with one hash.  own=False: one of them next to a cluster (the far cell's poses are candidates:
    counted under use_l1, never without).  own=True: the far cell shares the hash of the cluster's OWN cell, so their poses
    interleave in the sorted list and a group must break on the cell comparison"""
    for a, f in COLLISIONS:
        assert len(set(R.fnv_cells(np.asarray([a, f], np.int32)).tolist())) == 1
    b = Builder(oracle, use_l1=use_l1, weights=_weights(w), mix=w == "frac")
    seen = []
    for near, far in COLLISIONS:
        if own:
            for j in range(5):                                # alternate: indices interleave in the hash's list
                seen.append(b.add(near, (0.9, 0.5, 0.5), alpha=10 + j % 2, count=2))
                b.add(far, (0.5, 0.5, 0.5), alpha=10 + j % 2, count=2)
            _fill(b, (near[0] + 1, near[1], near[2]), 6, frac=(0.1, 0.5, 0.5), alphas=(10, 11))
            _fill(b, (far[0] + 1, far[1], far[2]), 2, frac=(0.1, 0.5, 0.5), alphas=(10, 11))
        else:
            seen += _fill(b, (near[0] - 1, near[1], near[2]), 4, frac=(0.9 if near[0] - 1 > 0 else 0.95, 0.5, 0.5), alphas=(10, 11))
            _fill(b, near, 3, frac=(0.1 if near[0] > 0 else 0.3, 0.5, 0.5), alphas=(10, 11))
            _fill(b, far, 5, alphas=(10, 11, 10, 11, 50), counts=(3, 4))
    c = b.finish("collision_%s_%s_%s" % ("own" if own else "near", "l1" if use_l1 else "l2", w))
    ref = c["ref"]
    assert aimed_cells_hit(c)
    if own:
        if w == "one":
            assert whole_mode(ref)
        # inside one hash's list the cell changes from position to position
        o = ref["order"]
        flips = sum(1 for a, bb in zip(o[:-1], o[1:]) if ref["hash"][a] == ref["hash"][bb] and not np.array_equal(ref["cell"][a], ref["cell"][bb]))
        assert flips >= 8
    else:
        for s in seen:
            i = index_of(ref, s)
            cand, lens = R.candidates(ref, i)
            far_c = [k for k in cand if abs(int(ref["cell"][k][0]) - int(ref["cell"][i][0])) > 1]
            assert len(far_c) == 5
            ok = R.compatible(ref, i, cand, c["d"], use_l1)
            counted = [k for k, good in zip(cand, ok) if good and k in far_c]
            assert (len(counted) >= 2) if use_l1 else (len(counted) == 0)
    return c


def case_probe_chains(oracle):
    """cells whose table slots collide: three hashes with one home slot, and three whose home is the LAST slot, so that
    the chain wraps to slot 0"""
    n = 24
    cap = table_cap(n)
    grid = np.asarray([(3 * i + 1, 3 * j + 1, 3 * k + 1) for i in range(14) for j in range(14) for k in range(14)], np.int32)
    gh = R.fnv_cells(grid)
    home = home_slots(gh, n)
    last = [int(i) for i in np.nonzero(home == cap - 1)[0][:3]]
    mid = [int(i) for i in np.nonzero(home == 20)[0][:3]]
    assert len(last) == 3 and len(mid) == 3
    b = Builder(oracle)
    for i in last + mid:
        cell = tuple(int(v) for v in grid[i])
        _fill(b, cell, 2, frac=(0.9, 0.5, 0.5), alphas=(10, 11), counts=(1, 3))
        _fill(b, (cell[0] + 1, cell[1], cell[2]), 2, frac=(0.1, 0.5, 0.5), alphas=(10, 11), counts=(2, 5))
    c = b.finish("probe_chains")
    ref = c["ref"]
    assert aimed_cells_hit(c) and len(ref["kept"]) == n and table_cap(len(ref["kept"])) == cap
    hs = np.unique(ref["hash"])
    slots = home_slots(hs, n)
    assert (slots == cap - 1).sum() >= 3 and (slots == 20).sum() >= 3 and len(hs) == 12
    # whatever the order of insertion, three keys with one home occupy three slots in a row from it: a chain of three,
    # and from the last slot the chain goes on at slot 0
    return c


def case_order(oracle, kind, two_sorts=False):
    """the order of the kept cells: counts 1 .. 2^31 under global_max 2^32 - 1 (the widest packed keys), or many equal
    counts where the code decides"""
    b = Builder(oracle, two_sorts=two_sorts)
    if kind == "wide":
        counts = [1 << k for k in range(32)] + [3, 3, 1 << 31, 1 << 30, 5, 1]
        gmax = 2 ** 32 - 1
        b.sp += [np.array([900.0 + k, 900.0, 900.0]) * b.d for k in range(4000)]      # unused scene points: 12 bits of scene reference
    else:
        counts = [7] * 90 + [8] * 5 + [6] * 5
        gmax = None
    for j, k in enumerate(counts):
        b.add((2 + j % 2, 2 + (j // 2) % 3, 2), (0.9 - 0.8 * (j % 2), 0.5, 0.5), m=j % 5, alpha=10 + j % 3, count=k)
    c = b.finish("order_%s_%d" % (kind, two_sorts), gmax=gmax)
    ref = c["ref"]
    k = ref["kept"]
    assert len(k) == len(counts)
    assert all((a["count"] > bb["count"]) or (a["count"] == bb["count"] and a["code"] < bb["code"]) for a, bb in zip(k[:-1], k[1:]))
    if kind == "wide":
        # the packed key: 6 alpha bits + the model reference's + the scene reference's + the count's
        key_bits = 6 + (M - 1).bit_length() + (len(c["sp"]) - 1).bit_length() + c["gmax"].bit_length()
        assert key_bits == 56 and int(ref["s_ref"].min()) > 4000
        assert int(k["count"].max()) == 2 ** 31 and int(k["count"].min()) == 1 and len(set(k["count"].tolist())) < len(k)
    else:
        assert (k["count"] == 7).sum() == 90
    return c


def case_best_blocks(oracle):
    """n = 8193: k_pose_best runs three blocks, block b takes the indices i with (i / 1024) % 3 == b.  Three equal top
    scores, one per block; the lowest index lies in the LAST block"""
    n = 8193
    tops = {t: None for t in BEST_BLOCKS_TOPS}
    assert sorted((i // 1024) % 3 for i in tops) == [0, 1, 2] and (min(tops) // 1024) % 3 == 2
    b = Builder(oracle)
    spot = 0
    for i in range(n):                                    # every count is 1: index = order of adding
        base = None
        for t in tops:
            if i == t or (i - t - 1) in range(20):
                base = t
        if base is not None:
            k = sorted(tops).index(base)
            cell = (70 + 4 * k, 2, 2)
            if i == base:
                tops[base] = b.add(cell, (0.9, 0.5, 0.5))
            else:
                b.add((cell[0] + 1, 2, 2), (0.1, 0.5, 0.5))
            continue
        # filler: pairs two cells apart from the next pair, scores 1 or 2
        ix, iy, iz = spot % 21, (spot // 21) % 21, spot // 441
        b.add((3 * ix + 1, 3 * iy + 1, 3 * iz + 1), alpha=(spot % 5) * 8)
        spot += 1
    c = b.finish("best_blocks")
    ref = c["ref"]
    assert len(ref["kept"]) == n
    for t, s in tops.items():
        assert index_of(ref, s) == t and list_lens(ref, t).sum() == 20
    return c


def case_stride(oracle):
    """n = 64 * 64 * 65 = 266240: every (model point, alpha) for 65 scene points that lie far apart, so that the 65 sets
    of 4096 poses are copies of one another and the top score comes back in set after set.  k_pose_best runs 64 blocks
    of 1024 threads; from index 64 * 4096 = 262144 on a thread is at its fifth index, and the first maximum lies lower"""
    b = Builder(oracle, d_dist=0.0625)
    pts = [np.array([4.0 * (k % 5) + 2, 4.0 * ((k // 5) % 5) + 2, 4.0 * (k // 25) + 2]) for k in range(65)]
    b.sp += pts
    low = np.arange(4096, dtype=np.int64)
    b.rec = [((s << 32) | int(v), 1) for s in range(1, 66) for v in low]
    c = b.finish("stride")
    assert len(c["ref"]["kept"]) == 266240 and whole_mode(c["ref"])
    return c


def check_stride(case, scores):
    """from the reference's scores: the maximum is shared, first below 262144 and again at or past it, and two of the
    equal maxima lie a multiple of 64 * 1024 apart: ONE thread of k_pose_best meets both on its grid stride, the later
    one at or past 262144, and must keep the earlier"""
    top = np.nonzero(scores == scores.max())[0]
    assert len(top) >= 2 and top[0] < 262144 <= top[-1], top
    late = top[top >= 262144]
    assert any(((late - t) % 65536 == 0).any() for t in top[top < 262144]), "no thread meets two of the maxima"
    assert ((late - top[0]) % 65536 == 0).any(), "the thread of the first maximum meets no later one"


BEST_BLOCKS_TOPS = (2500, 5000, 7000)


def check_best_blocks(case, scores):
    """from the reference's scores: the three cluster heads tie at the maximum, and the first of them is the winner"""
    t = list(BEST_BLOCKS_TOPS)
    assert (scores[t] == scores.max()).all() and int(np.argmax(scores)) == t[0]
    assert sorted((i // 1024) % 3 for i in np.nonzero(scores == scores.max())[0]) == [0, 1, 2]


def host_tail_scores(ppf, c):
    """The tap's path 0 without a model or a device, for the host test: the case's records -> filter, order, the host
    loop (oslam_pose_stage_ex, no hook) -> (kept cells, scores, winner's index, its T 4x4)"""
    lib = ppf.lib()
    kept = np.ascontiguousarray(c["records"], CELL_DTYPE).copy()
    k = lib.oslam_filter_cells(ppf._p(kept), len(kept), float(c["thresh"]), int(c["gmax"]))
    kept = kept[:k].copy()
    lib.oslam_sort_cells(ppf._p(kept), k)
    T, sc, best = np.zeros(16, F), np.zeros(max(k, 1), F), C.c_uint32(0)
    w = np.ascontiguousarray(c["weights"], F)
    rc = lib.oslam_pose_stage_ex(ppf._p(kept), k, ppf._p(c["mp"]), ppf._p(c["mn"]), len(c["mp"]), ppf._p(c["sp"]), ppf._p(c["sn"]),
                                 len(c["sp"]), float(c["d"]), 0, int(c["use_l1"]), 0, ppf._p(w), ppf._p(T), None, None, None,
                                 ppf._p(sc), C.byref(best))
    assert rc == 0, rc
    return kept, sc[:k].copy(), int(best.value), T.reshape(4, 4)


# ---- the registry: name -> builder(oracle) ----
CASES = {}
for _n in (2, 3, 5, 6, 7):
    for _w in ("one", "frac"):
        CASES["ragged_%d_%s" % (_n, _w)] = lambda o, n=_n, w=_w: case_ragged(o, n, w)
for _w in ("one", "frac"):
    CASES["isolated_one_%s" % _w] = lambda o, w=_w: case_isolated(o, False, w)
    CASES["groups_%s" % _w] = lambda o, w=_w: case_groups(o, w)
    CASES["zero_hash_%s" % _w] = lambda o, w=_w: case_zero_hash(o, w)
    CASES["collision_own_l2_%s" % _w] = lambda o, w=_w: case_collision(o, False, True, w)
    for _k in ("straddle", "exact", "short", "block"):
        CASES["windows_%s_%s" % (_k, _w)] = lambda o, k=_k, w=_w: case_windows(o, k, w)
    for _L in (1, 63, 64, 65, 255, 256, 257, 513):
        CASES["list_%d_%s" % (_L, _w)] = lambda o, L=_L, w=_w: case_list_length(o, L, w)
CASES["isolated_all_one"] = lambda o: case_isolated(o, True)
CASES["order_sensitive"] = case_order_sensitive
for _t in (2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24):
    CASES["vote_total_%d" % _t] = lambda o, t=_t: case_vote_total(o, t)
CASES["sum_bound"] = case_sum_bound
CASES["big_weight"] = lambda o: case_big_weight(o, False)
CASES["negative_weight"] = lambda o: case_big_weight(o, True)
for _l1 in (False, True):
    _t = "l1" if _l1 else "l2"
    CASES["rotation_%s" % _t] = lambda o, l1=_l1: case_rotation(o, l1)
    CASES["collision_near_%s" % _t] = lambda o, l1=_l1: case_collision(o, l1, False)
    for _d in (0.1, 0.25, 1.0 / 3.0):
        CASES["distance_%.3f_%s" % (_d, _t)] = lambda o, d=_d, l1=_l1: case_distance(o, float(F(d)), l1)
CASES["collision_own_l1_one"] = lambda o: case_collision(o, True, True)
CASES["probe_chains"] = case_probe_chains
for _s in (False, True):
    CASES["order_wide_%d" % _s] = lambda o, s=_s: case_order(o, "wide", s)
    CASES["order_equal_%d" % _s] = lambda o, s=_s: case_order(o, "equal", s)
CASES["best_blocks"] = case_best_blocks
CASES["stride"] = case_stride

_BUILT = {}


def get_case(name, oracle):
    """the finished case with the reference's scores and winner, made once per process and left unchanged"""
    if name not in _BUILT:
        c = CASES[name](oracle)
        c["scores"], c["best"] = R.scores(c["ref"], c["d"], c["use_l1"])
        if name == "stride":
            check_stride(c, c["scores"])
        if name == "best_blocks":
            check_best_blocks(c, c["scores"])
        for v in (c["scores"], c["records"], c["sp"]):
            v.setflags(write=False)
        _BUILT[name] = c
    return _BUILT[name]
