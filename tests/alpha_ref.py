"""Float64 statement of the alpha bin of kernel.cu:338-342, for the votes of one scene reference point.

From the float32 operands the reference computes for a vote -- u = T_m_g * m_i and v = T_s_g * s_i, of which only
the y and z components enter (oracle.FusedModel.vote_dump) -- alpha + pi = atan2(u_y v_z - u_z v_y, u_y v_y + u_z v_z)
+ pi is evaluated in float64, with its bin, its nearest bin edge and its distance from that edge in bins.  The edges
are the multiples of the reference's float32 bin width D (its quantisation is x - fmodf(x, D), exact); edge 30 is
the edge 0 and borders bins 29, 30 and 0 (the reference's bin 30 is alpha + pi rounded up to 2 pi).

Degenerate operands are flagged by the rule of ppf_core.h:pc_angle_t22 (a vector that is zero, not finite or
outside 2^-40..2^40) and follow the stated rule of each vote mode, not a slack:
  exact mode  the reference's own float32 sequence decides (the oracle's bin is taken as it is);
  fast mode   the degenerate side counts as theta = 0, i.e. atan2 + pi = 0 (include/oslam.h, OSLAM_VOTE_FAST).

Only the alpha step is checked here.  The frames T_g themselves are the reference's float32 frames, taken as given
(the operands come from the oracle); how far those lie from the exact rigid transforms is out of scope.
"""
import numpy as np

NBIN = 30
D32 = float(np.float32(np.float32(2.0) * np.float32(3.141592654)) / np.float32(30.0))   # kernel.h:16 in float32


def degenerate(y, z):
    """pc_angle_t22's marker rule on float32 (y, z)."""
    by = np.asarray(y, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    bz = np.asarray(z, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    e = np.maximum(by, bz) >> np.uint32(23)
    return (e < 87) | (e > 167)


def alpha64(uy, uz, vy, vz, vote_mode=0):
    """-> (x, degenerate): x = (alpha + pi) / D in float64 for every vote; for fast mode with a degenerate side the
    stated rule (theta = 0 on that side) gives x, for exact mode x is NaN there."""
    uy, uz, vy, vz = (np.asarray(a, np.float32).astype(np.float64) for a in (uy, uz, vy, vz))
    du, dv = degenerate(uy.astype(np.float32), uz.astype(np.float32)), degenerate(vy.astype(np.float32), vz.astype(np.float32))
    deg = du | dv
    with np.errstate(all="ignore"):
        x = (np.arctan2(uy * vz - uz * vy, uy * vy + uz * vz) + np.pi) / D32
        if vote_mode == 1:
            tu = np.where(du, 0.0, np.arctan2(uz, uy) + np.pi)
            tv = np.where(dv, 0.0, np.arctan2(vz, vy) + np.pi)
            xs = np.mod(tv - tu + np.pi, 2.0 * np.pi) / D32
            x = np.where(deg, xs, x)
        else:
            x = np.where(deg, np.nan, x)
    return x, deg


def edges(x):
    """-> (bin, nearest edge k, distance |x - k| in bins) of float64 positions x in [0, 30]."""
    b = np.clip(np.floor(x), 0, NBIN).astype(np.int64)
    k = np.rint(x).astype(np.int64)
    return b, k, np.abs(x - k)


def bin_errors(bins, x, deg, eps):
    """Votes whose given bin is not the float64 one and is not the neighbour across the nearest edge within eps.
    -> (indices of such votes, number of bins that differ, largest distance from its edge of a differing bin)."""
    ok = ~np.isnan(x)
    b, k, d = edges(np.where(ok, x, 0.0))
    bins = np.asarray(bins, np.int64)
    same = (bins == b) | ((bins == 0) & (b == NBIN))
    across = np.where(x < k, k % NBIN, (k - 1) % NBIN)
    across_ok = (bins == across) | ((k % NBIN == 0) & np.isin(bins, (NBIN - 1, NBIN, 0)))
    differ = ok & ~same
    bad = differ & ~(across_ok & (d <= eps))
    worst = float(d[differ].max()) if differ.any() else 0.0
    return np.nonzero(bad)[0], int(differ.sum()), worst


def below_edge(x, width):
    """votes that lie within `width` bins below an edge (the ones a shifted base moves into the next bin)"""
    k = np.ceil(x)
    return np.isfinite(x) & (k - x > 0) & (k - x <= width)


def interval_check(acc, m_r, uy, uz, vy, vz, eps, vote_mode=0, exact_bins=None):
    """Every cell of the dense accumulator acc[M][32] of one reference point against the float64 bins of its votes:
    lo = the votes whose float64 bin is the cell and that lie farther than eps from an edge, hi = lo + the votes within
    eps of an edge that borders the cell; passes when lo <= acc <= hi everywhere and the totals are equal.  Exact mode:
    the degenerate votes count in the bin exact_bins gives them (the oracle's float32 bins), in lo and hi alike.
    -> list of (row, bin, lo, acc, hi) of the cells that fail (empty: passed)."""
    acc = np.asarray(acc, np.int64)
    M, W = acc.shape
    m_r = np.asarray(m_r, np.int64)
    x, deg = alpha64(uy, uz, vy, vz, vote_mode)
    lo = np.zeros((M, W), np.int64)
    hi = np.zeros((M, W), np.int64)
    fixed = np.isnan(x)
    if fixed.any():
        assert exact_bins is not None, "exact mode needs the oracle's bins of the degenerate votes"
        fb = np.asarray(exact_bins, np.int64)[fixed]
        np.add.at(lo, (m_r[fixed], fb), 1)
        np.add.at(hi, (m_r[fixed], fb), 1)
    live = ~fixed
    b, k, d = edges(np.where(live, x, 0.0))
    far = live & (d > eps)
    near = live & (d <= eps)
    np.add.at(lo, (m_r[far], b[far] % NBIN), 1)
    np.add.at(hi, (m_r[far], b[far] % NBIN), 1)
    kn = k[near] % NBIN
    rn = m_r[near]
    # edge k borders bins k - 1 and k; edge 0 (= 30) borders 29, 30 and 0
    np.add.at(hi, (rn, (kn - 1) % NBIN), 1)
    np.add.at(hi, (rn, kn), 1)
    np.add.at(hi, (rn[kn == 0], np.full(int((kn == 0).sum()), NBIN)), 1)
    bad = np.argwhere((acc < lo) | (acc > hi))
    fails = [(int(r), int(c), int(lo[r, c]), int(acc[r, c]), int(hi[r, c])) for r, c in bad]
    if int(acc.sum()) != len(m_r):
        fails.append((-1, -1, len(m_r), int(acc.sum()), len(m_r)))
    return fails
