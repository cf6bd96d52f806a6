"""The yardstick of the tests of nghmm_ibd_longest (include/nghmm.h), in numpy, twice:

(A) float64, a DIFFERENT algorithm: the posterior chain augmented by the first site of the current
    run.  U[a] is the mass inside a run that began at a and has not reached the threshold, carried
    site by site as a running product (U[a] *= r_s(1, 1)); it is absorbed the moment len(a, s)
    reaches L_k.  Nothing is subtracted, and a chromosome start inside a region is walked through
    (the old run ends, a new one begins).  O(S x window).  pi and r_s from
    sample_util.forward_filter and a backward vector normalised at every site.
(B) np.longdouble: pi, r_s and ln rho in log space, then the recursion of include/nghmm.h itself --
    N, V, Hit with G_s = sum of tau_a exp(Q_s - Q_a) over the starts a with b_k(a) = s, Q the prefix
    sum of ln rho restarted at every blocked step -- likewise walked through chromosome starts.

Both carry exact zeros.  enumerate_longest is brute force over all 2^S paths (S <= 12) from the
path probabilities and the run definition alone; path_longest gives the longest run of given 0/1
paths.  tests/test_longest_cpu.py checks A and B against the enumeration before
tests/test_gpu_longest.py uses B.  The device uses a third arrangement: pi propagated from a
chromosome's first site, a ring per lane, the parts of a region per chromosome combined as
independent."""
import numpy as np

import bylength_util as bu
import expect_util as xu
import sample_util as su

FIELDS = ("p_any", "p_none")
DTYPE = np.dtype([(f, np.float64) for f in FIELDS])


def cells_a(eprob, pos, F, alpha):
    """Yardstick A's per-cell quantities, float64: (pi [I][S][2], r [I][S][2][2])."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    q = np.stack([1 - F, F], axis=1)
    f = su.forward_filter(eprob, pos, F, alpha)
    fprev = np.concatenate([q[:, None, :], f[:, :-1]], axis=1)
    e = np.exp(eprob - eprob.max(axis=2, keepdims=True))
    c = su.coancestry(alpha, pos)
    m = np.empty((I, S, 2, 2))
    w = np.ones((I, 2))
    for s in range(S - 1, -1, -1):
        u = e[:, s] * w
        off = (1 - c[:, s, None]) * q
        T = np.stack([np.stack([off[:, 0] + c[:, s], off[:, 1]], axis=1),
                      np.stack([off[:, 0], off[:, 1] + c[:, s]], axis=1)], axis=1)
        m[:, s] = T * u[:, None, :]
        w = m[:, s].sum(axis=2)
        w = w / w.sum(axis=1, keepdims=True)
    n = fprev[..., None] * m
    xi = n / n.sum(axis=(2, 3), keepdims=True)
    pi = xi.sum(axis=2)
    row = m.sum(axis=3, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(row > 0, m / row, 0.0)
    return pi, r


def cells_b(eprob, pos, F, alpha):
    """Yardstick B's per-cell quantities, np.longdouble from log space: (pi [I][S][2],
    r [I][S][2][2], ln rho [I][S], -inf where the step is blocked)."""
    ld = np.longdouble
    eprob = np.asarray(eprob).astype(ld)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,)).astype(ld)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)).astype(ld)
    posf = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(posf)
    start = np.isinf(posf)
    d = np.where(start, 0.0, posf).astype(ld)
    c = np.exp(-alpha[:, None] * d[None, :])
    c[:, start] = 0
    q = np.stack([1 - F, F], axis=1)
    with np.errstate(divide="ignore"):
        lq = np.log(q)
        loff = np.log((1 - c)[..., None] * q[:, None, :])
        ldiag = np.log((1 - c)[..., None] * q[:, None, :] + c[..., None])
    lT = np.stack([np.stack([ldiag[..., 0], loff[..., 1]], axis=-1),
                   np.stack([loff[..., 0], ldiag[..., 1]], axis=-1)], axis=-2)
    lf = np.empty((I, S, 2), dtype=ld)
    lb = np.empty((I, S, 2), dtype=ld)
    with np.errstate(invalid="ignore"):
        v = lq
        for s in range(S):
            v = np.logaddexp(v[:, 0, None] + lT[:, s, 0, :], v[:, 1, None] + lT[:, s, 1, :]) + eprob[:, s]
            lf[:, s] = v
        w = np.zeros((I, 2), dtype=ld)
        for s in range(S - 1, -1, -1):
            lb[:, s] = w
            u = eprob[:, s] + w
            w = np.logaddexp(lT[:, s, :, 0] + u[:, 0, None], lT[:, s, :, 1] + u[:, 1, None])
        lfprev = np.concatenate([np.broadcast_to(lq[:, None, :], (I, 1, 2)), lf[:, :-1]], axis=1)
        lm = lT + (eprob + lb)[:, :, None, :]
        lm = np.where(np.isnan(lm), -np.inf, lm)
        ln_n = lfprev[..., None] + lm
        ln_n = np.where(np.isnan(ln_n), -np.inf, ln_n)
        lz = np.logaddexp(np.logaddexp(ln_n[..., 0, 0], ln_n[..., 0, 1]),
                          np.logaddexp(ln_n[..., 1, 0], ln_n[..., 1, 1]))
        xi = np.exp(ln_n - lz[..., None, None])
        lrow = np.logaddexp(lm[..., 0], lm[..., 1])[..., None]
        r = np.where(np.isneginf(lrow) | np.isneginf(lm), ld(0), np.exp(lm - lrow))
        lrho = xu._ln_share_log(lm[:, :, 1, 1], lm[:, :, 1, 0])
    pi = xi.sum(axis=2)
    lrho = np.array(lrho, dtype=ld)
    lrho[:, cs] = -np.inf
    return pi, np.asarray(r, dtype=ld), lrho


def _resolved_at(bk, S):
    """For every threshold and site s the starts a with b_k(a) = s, a contiguous range
    [a_lo[k][s], a_hi[k][s]) (b_k is non-decreasing inside a chromosome); empty: a_lo >= a_hi."""
    K = len(bk)
    a_lo = np.full((K, S), S, dtype=np.int64)
    a_hi = np.zeros((K, S), dtype=np.int64)
    for k in range(K):
        a = np.flatnonzero(bk[k] >= 0)
        np.minimum.at(a_lo[k], bk[k, a], a)
        np.maximum.at(a_hi[k], bk[k, a], a + 1)
    return a_lo, a_hi


def records_a(cells, pos, min_len, unit, regions):
    """Yardstick A: [I][R][K] of DTYPE."""
    pi, r = cells
    I, S = pi.shape[:2]
    cs = xu.chrom_start(pos)
    bk = bu.window_ends(pos, min_len, unit)
    K = len(bk)
    a_lo, a_hi = _resolved_at(bk, S)
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((I, len(reg), K), dtype=DTYPE)
    for g, (lo, hi) in enumerate(reg):
        for k in range(K):
            U = np.zeros((I, hi - lo))                  # by the run's first site, minus lo
            N = pi[:, lo, 0].copy()
            hit = np.zeros(I)
            ap = lo
            for s in range(lo, hi):
                if s == lo:
                    U[:, 0] = pi[:, lo, 1]
                else:
                    tot = U[:, ap - lo:s - lo].sum(axis=1)
                    new = N * r[:, s, 0, 1]
                    N = N * r[:, s, 0, 0] + tot * r[:, s, 1, 0]
                    if cs[s]:                           # the old run ends, a new one begins
                        new = new + tot * r[:, s, 1, 1]
                        U[:, ap - lo:s - lo] = 0.0
                        ap = s
                    else:
                        U[:, ap - lo:s - lo] *= r[:, s, 1, 1][:, None]
                    U[:, s - lo] = new
                x0, x1 = max(a_lo[k, s], lo), a_hi[k, s]
                if x0 < x1:
                    hit = hit + U[:, x0 - lo:x1 - lo].sum(axis=1)
                    U[:, x0 - lo:x1 - lo] = 0.0
                while ap <= s and 0 <= bk[k, ap] <= s:
                    ap += 1
            out["p_any"][:, g, k] = hit
            out["p_none"][:, g, k] = N + U[:, min(ap, hi) - lo:].sum(axis=1)
    return out


def records_b(cells, pos, min_len, unit, regions):
    """Yardstick B: the recursion of include/nghmm.h in np.longdouble, returned as float64."""
    ld = np.longdouble
    pi, r, lrho = cells
    I, S = pi.shape[:2]
    cs = xu.chrom_start(pos)
    blocked = np.isneginf(lrho)
    with np.errstate(over="ignore"):
        rho = np.where(blocked, ld(0), np.exp(np.where(blocked, ld(0), lrho)))
    Q = np.zeros((I, S), dtype=ld)
    q = np.zeros(I, dtype=ld)
    for s in range(S):
        q = np.where(blocked[:, s], ld(0), q + np.where(blocked[:, s], ld(0), lrho[:, s]))
        Q[:, s] = q
    nb = np.cumsum(blocked, axis=1)
    bk = bu.window_ends(pos, min_len, unit)
    K = len(bk)
    a_lo, a_hi = _resolved_at(bk, S)
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((I, len(reg), K), dtype=DTYPE)
    for g, (lo, hi) in enumerate(reg):
        for k in range(K):
            tau = np.zeros((I, hi - lo), dtype=ld)
            N = pi[:, lo, 0].copy()
            V = np.zeros(I, dtype=ld)
            hit = np.zeros(I, dtype=ld)
            for s in range(lo, hi):
                if s == lo:
                    t = pi[:, lo, 1]
                    keep = np.zeros(I, dtype=ld)
                else:
                    t = N * r[:, s, 0, 1]
                    if cs[s]:
                        t = t + V * r[:, s, 1, 1]
                    N = N * r[:, s, 0, 0] + V * r[:, s, 1, 0]
                    keep = V * rho[:, s]
                tau[:, s - lo] = t
                x0, x1 = max(a_lo[k, s], lo), a_hi[k, s]
                G = np.zeros(I, dtype=ld)
                if x0 < x1:
                    aa = np.arange(x0, x1)
                    W = np.where(nb[:, aa] == nb[:, s, None], np.exp(Q[:, s, None] - Q[:, aa]), ld(0))
                    G = (tau[:, aa - lo] * W).sum(axis=1)
                hit = hit + G
                V = np.maximum(keep + t - G, ld(0))
            out["p_any"][:, g, k] = hit.astype(np.float64)
            out["p_none"][:, g, k] = (N + V).astype(np.float64)
    return out


def path_longest(paths, pos, unit):
    """The longest run of given 0/1 paths [..][S] (runs of 1 cut at chromosome starts): [..] in
    sites, or in Mb (first site to last, so a one-site run is 0 Mb); -1 for a path without a run."""
    z = np.asarray(paths).astype(bool)
    shape, S = z.shape[:-1], z.shape[-1]
    z = z.reshape(-1, S)
    N = len(z)
    pos = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(pos)
    d = np.where(np.isinf(pos), 0.0, pos)
    out = np.full(N, -1.0)
    nr = S + 1
    for lo in range(0, N, 256):
        zz = z[lo:lo + 256]
        n = len(zz)
        prev = np.concatenate([np.zeros((n, 1), dtype=bool), zz[:, :-1]], axis=1)
        st = zz & (~prev | cs[None, :])
        gid = (np.arange(n)[:, None] * nr + np.cumsum(st, axis=1))[zz]
        sites = np.bincount(gid, minlength=n * nr).reshape(n, nr)
        if unit == "mb":
            lens = np.bincount(gid, weights=np.where(st, 0.0, d[None, :])[zz], minlength=n * nr).reshape(n, nr)
        else:
            lens = sites.astype(np.float64)
        out[lo:lo + n] = np.where(sites > 0, lens, -1.0).max(axis=1)
    return out.reshape(shape)


def enumerate_longest(eprob, pos, F, alpha, min_len, unit, regions):
    """Brute force over all 2^S paths (S <= 12): [I][R][K] of DTYPE from the path probabilities and
    path_longest of the region's sites alone (a region's first site cuts a run like a chromosome
    start)."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    c = su.coancestry(alpha, pos)
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1
    e = np.exp(eprob)
    L = np.atleast_1d(np.asarray(min_len, dtype=np.float64))
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((I, len(reg), len(L)), dtype=DTYPE)
    pos = np.asarray(pos, dtype=np.float64)
    longest = []
    for lo, hi in reg:
        sub = pos[lo:hi].copy()
        sub[0] = np.inf
        longest.append(path_longest(z[:, lo:hi].astype(np.uint8), sub, unit))
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        p = p / p.sum()
        for g in range(len(reg)):
            for k, l in enumerate(L):
                hit = longest[g] >= l
                out["p_any"][i, g, k] = p[hit].sum()
                out["p_none"][i, g, k] = p[~hit].sum()
    return out


def spread(a, b):
    """Largest |A - B| per field of two record arrays."""
    return {f: float(np.max(np.abs(a[f] - b[f]))) if a[f].size else 0.0 for f in FIELDS}


def sampler_check(longest, p_any, min_len, tag=""):
    """The condition of the test against the sampler, on longest [R][I] (path_longest of R draws)
    and the exact p_any of the whole data [I][K]: per threshold the cohort total of the hits within
    5 standard errors sqrt(sum p (1 - p) / R) of the exact total, and every individual within
    5 sqrt(p (1 - p) / R); no case is left out.  Returns the largest |z| (0 / 0 counts as 0)."""
    R = longest.shape[0]
    worst = 0.0
    for k, l in enumerate(np.atleast_1d(min_len)):
        p = np.clip(p_any[:, k], 0.0, 1.0)
        freq = (longest >= l).mean(axis=0)                                   # [I]
        var = p * (1 - p) / R
        dev, se = abs(freq.sum() - p.sum()), np.sqrt(var.sum())
        assert dev <= 5 * se, (tag, k, "cohort", dev, se)
        devi = np.abs(freq - p)
        assert (devi <= 5 * np.sqrt(var)).all(), (tag, k, devi.max())
        with np.errstate(invalid="ignore", divide="ignore"):
            zi = np.where(devi > 0, devi / np.sqrt(var), 0.0)
        worst = max(worst, dev / se if se > 0 else 0.0, float(zi.max()))
    return worst


# The spread of the two yardsticks on support_util.gpu_cohort, largest |A - B| per unit and field
# over all the region sets of expect_util.region_sets(5003, pos, 80) and the thresholds
# bylength_util.COHORT_LEN, as tests/test_longest_cpu.py measures and prints it (float64 run-start
# chain against the longdouble recursion).  See there for how to re-measure.  Nothing here is taken
# from a device.  The largest figures belong to the SHORT regions (windows of 7 sites, single
# sites): they are the error of A's forward and backward vectors in pi at a region's first site,
# as support_util.SPREAD's; over the whole data the two agree to 1e-14.
SPREAD = {"sites": {"p_any": 7.716e-14, "p_none": 7.727e-14},
          "mb": {"p_any": 1.004e-13, "p_none": 1.005e-13}}
# 16 x the spread, support_util's rule and margin
TOL = {u: {f: 16 * v for f, v in s.items()} for u, s in SPREAD.items()}
