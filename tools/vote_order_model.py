"""Scratch (CPU, oracle keys): a replay of k_vote's scheduling on the bench workload, for the two orders in which its
work can be handed out (oslam_params.vote_order).  Not part of the product or of a test.

Inside a workgroup (one reference point x one table slice, 16 waves): the runs of the reference point are sorted by key
number.  Items above VOTE_GIANT iterations are cut into units of one chunk pass and dealt round-robin first; the
remaining runs are taken in blocks of 16 runs, in key-number order, by whichever wave is free.  A step (64 hits of a
run against one 256-entry chunk) costs 42 + 20 x hits instructions, a block 60.  Printed for an arbitrary numbering of
the keys (a random permutation, as the atomic counter gave) and for keys numbered by descending total bucket length:
the share of wave time spent waiting at the barrier behind the votes, and the summed makespan.

Across the grid: the sampled workgroups' makespans are drawn 37 500 times (12 500 reference points x 3 slices) and
replayed on 256 CUs, one workgroup per CU, in index order and heaviest first (by the reference point's hits, the
host's measure), against the ideal total / 256.

  python tools/vote_order_model.py [sampled reference points, default 64]

Compare with the -DVOTE_PROF phase shares."""
import heapq
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("objective-slam_amd")
synth = pkg.synth
from oracle import oracle as O  # noqa: E402

M, S, df, tau = 5000, 100000, 8, 0.025
n_sample = int(sys.argv[1]) if len(sys.argv) > 1 else 64
SLICE, WAVES, GIANT, BLOCK = 2046, 16, 16, 16
STEP, PER_HIT, BLOCK_COST = 42, 20, 60

mp, mn = synth.make_model(0, M)
d = synth.d_dist_for(mp, tau)
sp, sn, _ = synth.make_scene([0], S, 2002, instance_points=M, noise_sigma=0.1 * d)
keys = np.empty((M, M), np.uint32)
for r in range(M):
    keys[r] = O.ppf_row_keys(mp, mn, r, d)
sl = (np.arange(M) // SLICE).astype(np.uint64)
comb = ((sl[:, None] << np.uint64(32)) | keys.astype(np.uint64))[keys != 0]
uk, cnt = np.unique(comb, return_counts=True)                 # (slice, key) -> bucket length
allk, inv = np.unique(uk & np.uint64(0xffffffff), return_inverse=True)
weight = np.bincount(inv, weights=cnt).astype(np.int64)       # key -> entries over all slices
nsl = (M + SLICE - 1) // SLICE
rng = np.random.default_rng(1)
number = {"arbitrary": rng.permutation(len(allk)),
          "by weight": np.argsort(np.lexsort((allk, -weight)))}  # rank of every key: weight descending, key ascending


def step_cost(hits):
    return STEP + PER_HIT * hits


def workgroup(ln, R):
    """makespan and waiting share of one workgroup whose runs (bucket length ln, hits R) are in dispatch order"""
    nch = (ln + 255) // 256
    free = [0] * WAVES
    giant = nch * R > GIANT
    w = 0
    for n, r in zip(nch[giant], R[giant]):                    # units of one chunk dealt round-robin
        for _ in range(int(n)):
            free[w % WAVES] += step_cost(int(r))
            w += 1
    heapq.heapify(free)
    cost = (nch * (STEP + PER_HIT * R))[~giant]
    for b in range(0, len(cost), BLOCK):                      # blocks of 16 runs to whichever wave is free
        t = heapq.heappop(free)
        heapq.heappush(free, t + BLOCK_COST + int(cost[b:b + BLOCK].sum()))
    end = max(free)
    return end, sum(end - t for t in free) / (WAVES * end) if end else 0.0


refs = rng.choice(np.arange(0, S, df), n_sample, replace=False)
span = {k: [] for k in number}
wait = {k: [] for k in number}
hits_of = []
for r in refs:
    k = O.ppf_row_keys(sp, sn, int(r), d)
    k = k[k != 0].astype(np.uint64)
    pos = np.searchsorted(allk, k)
    pos[pos >= len(allk)] = 0
    pos = pos[allk[pos] == k]
    dk, R = np.unique(pos, return_counts=True)                 # runs: index of the key in allk, hits
    hits_of.append(len(pos))
    for name, num in number.items():
        o = np.argsort(num[dk])
        for s in range(nsl):
            ck = (np.uint64(s) << np.uint64(32)) | allk[dk[o]]
            p = np.searchsorted(uk, ck)
            p[p >= len(uk)] = 0
            m = uk[p] == ck
            ln, Rm = cnt[p[m]], R[o][m]
            e, wshare = workgroup(ln, np.minimum(Rm, 64))
            span[name].append(e)
            wait[name].append(wshare * e)
base = float(np.sum(span["arbitrary"]))
for name in number:
    sp_ = np.array(span[name], float)
    print("%-10s wait behind the votes %.1f%% of wave time, summed makespan %.3f (p90 %.2f, p99 %.2f, max %.2f x mean)"
          % (name, 100.0 * np.sum(wait[name]) / np.sum(sp_), np.sum(sp_) / base,
             np.percentile(sp_, 90) / sp_.mean(), np.percentile(sp_, 99) / sp_.mean(), sp_.max() / sp_.mean()))

# the grid: 37 500 workgroups drawn from the sampled reference points, one per CU, 256 CUs
sp_ = np.array(span["by weight"], float).reshape(len(refs), nsl)
n_ref, cus = (S + df - 1) // df, 256
pick = rng.integers(0, len(refs), n_ref)
demand = np.array(hits_of)[pick]
for name, order in (("index order", np.arange(n_ref)), ("heaviest first", np.argsort(-demand, kind="stable"))):
    free = [0.0] * cus
    heapq.heapify(free)
    for i in order:
        for s in range(nsl):
            heapq.heappush(free, heapq.heappop(free) + sp_[pick[i], s])
    print("%-14s grid makespan %.4f x ideal" % (name, max(free) / (sp_[pick].sum() / cus)))
