"""The yardstick of the tests of nghmm_ibd_count (include/nghmm.h), in numpy, twice, after
longest_util.py:

(A) float64, a DIFFERENT algorithm: the posterior chain augmented by (count level, first site of
    the current run).  U[c][a] is the mass inside a run that began at a, with c long runs before
    it, and has not reached the threshold, carried site by site as a running product
    (U[c][a] *= r_s(1, 1)); the moment len(a, s) reaches L_k it moves to Rm[c + 1], the mass inside
    a counted run (to the absorbing top level from c = M - 1).  Nothing is subtracted, and a
    chromosome start inside a region is walked through (the old run ends, a new one begins at the
    same level).  Cells from longest_util.cells_a.
(B) np.longdouble: the recursion of include/nghmm.h itself on longest_util.cells_b -- N_c, V_c, R_c,
    Top with G_c(s) = sum of tau_{a,c} exp(Q_s - Q_a) over the starts a with b_k(a) = s -- likewise
    walked through chromosome starts.

Both carry exact zeros.  enumerate_count is brute force over all 2^S paths (S <= 12) from the path
probabilities and the run definition alone; path_count counts the long runs of given 0/1 paths.
tests/test_count_cpu.py checks A and B against the enumeration before tests/test_gpu_count.py uses
B.  The device uses a third arrangement: pi propagated from a chromosome's first site, a ring per
lane, the parts of a region per chromosome combined by a convolution cut off at M."""
import numpy as np

import bylength_util as bu
import expect_util as xu
import longest_util as lu
import sample_util as su


def records_a(cells, pos, min_len, unit, regions, M):
    """Yardstick A: float64 [I][R][K][M + 1]."""
    pi, r = cells
    I, S = pi.shape[:2]
    cs = xu.chrom_start(pos)
    bk = bu.window_ends(pos, min_len, unit)
    K = len(bk)
    a_lo, a_hi = lu._resolved_at(bk, S)
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((I, len(reg), K, M + 1))
    for g, (lo, hi) in enumerate(reg):
        for k in range(K):
            U = np.zeros((M, I, hi - lo))               # by level and the run's first site, minus lo
            N = np.zeros((M, I))
            Rm = np.zeros((M, I))
            N[0] = pi[:, lo, 0]
            top = np.zeros(I)
            ap = lo
            for s in range(lo, hi):
                if s == lo:
                    U[0, :, 0] = pi[:, lo, 1]
                else:
                    tot = U[:, :, ap - lo:s - lo].sum(axis=2) + Rm
                    new = N * r[None, :, s, 0, 1]
                    N = N * r[None, :, s, 0, 0] + tot * r[None, :, s, 1, 0]
                    if cs[s]:                           # the old run ends, a new one begins
                        new = new + tot * r[None, :, s, 1, 1]
                        U[:, :, ap - lo:s - lo] = 0.0
                        Rm = np.zeros((M, I))
                        ap = s
                    else:
                        U[:, :, ap - lo:s - lo] *= r[None, :, s, 1, 1][:, :, None]
                        Rm = Rm * r[None, :, s, 1, 1]
                    U[:, :, s - lo] = new
                x0, x1 = max(a_lo[k, s], lo), a_hi[k, s]
                if x0 < x1:
                    got = U[:, :, x0 - lo:x1 - lo].sum(axis=2)
                    U[:, :, x0 - lo:x1 - lo] = 0.0
                    Rm[1:] = Rm[1:] + got[:-1]
                    top = top + got[-1]
                while ap <= s and 0 <= bk[k, ap] <= s:
                    ap += 1
            out[:, g, k, :M] = (N + U[:, :, min(ap, hi) - lo:].sum(axis=2) + Rm).T
            out[:, g, k, M] = top
    return out


def records_b(cells, pos, min_len, unit, regions, M):
    """Yardstick B: the recursion of include/nghmm.h in np.longdouble, returned as float64
    [I][R][K][M + 1]."""
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
    a_lo, a_hi = lu._resolved_at(bk, S)
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((I, len(reg), K, M + 1))
    for g, (lo, hi) in enumerate(reg):
        for k in range(K):
            tau = np.zeros((M, I, hi - lo), dtype=ld)
            N = np.zeros((M, I), dtype=ld)
            V = np.zeros((M, I), dtype=ld)
            Rm = np.zeros((M, I), dtype=ld)
            N[0] = pi[:, lo, 0]
            top = np.zeros(I, dtype=ld)
            for s in range(lo, hi):
                if s == lo:
                    t = np.zeros((M, I), dtype=ld)
                    t[0] = pi[:, lo, 1]
                    keep = np.zeros((M, I), dtype=ld)
                    keep_r = np.zeros((M, I), dtype=ld)
                else:
                    t = N * r[None, :, s, 0, 1]
                    if cs[s]:
                        t = t + (V + Rm) * r[None, :, s, 1, 1]
                    N = N * r[None, :, s, 0, 0] + (V + Rm) * r[None, :, s, 1, 0]
                    keep = V * rho[None, :, s]
                    keep_r = Rm * rho[None, :, s]
                tau[:, :, s - lo] = t
                x0, x1 = max(a_lo[k, s], lo), a_hi[k, s]
                G = np.zeros((M, I), dtype=ld)
                if x0 < x1:
                    aa = np.arange(x0, x1)
                    W = np.where(nb[:, aa] == nb[:, s, None], np.exp(Q[:, s, None] - Q[:, aa]), ld(0))
                    G = (tau[:, :, aa - lo] * W[None]).sum(axis=2)
                V = np.maximum(keep + t - G, ld(0))
                Rm = keep_r
                Rm[1:] = Rm[1:] + G[:-1]
                top = top + G[-1]
            out[:, g, k, :M] = (N + V + Rm).T.astype(np.float64)
            out[:, g, k, M] = top.astype(np.float64)
    return out


def path_count(paths, pos, unit, L):
    """The number of runs of length >= L of given 0/1 paths [..][S] (runs of 1 cut at chromosome
    starts; in sites, or in Mb first site to last, so a one-site run is 0 Mb): int64 [..], or
    [..][K] for a list of K thresholds."""
    z = np.asarray(paths).astype(bool)
    shape, S = z.shape[:-1], z.shape[-1]
    z = z.reshape(-1, S)
    n_paths = len(z)
    pos = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(pos)
    d = np.where(np.isinf(pos), 0.0, pos)
    Ls = np.atleast_1d(np.asarray(L, dtype=np.float64))
    out = np.zeros((n_paths, len(Ls)), dtype=np.int64)
    nr = S + 1
    for lo in range(0, n_paths, 256):
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
        for k, l in enumerate(Ls):
            out[lo:lo + n, k] = ((sites > 0) & (lens >= l)).sum(axis=1)
    return out.reshape(shape + (len(Ls),)) if np.ndim(L) else out[:, 0].reshape(shape)


def enumerate_count(eprob, pos, F, alpha, min_len, unit, regions, M):
    """Brute force over all 2^S paths (S <= 12): float64 [I][R][K][M + 1] from the path
    probabilities and path_count of the region's sites alone (a region's first site cuts a run like
    a chromosome start)."""
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
    out = np.zeros((I, len(reg), len(L), M + 1))
    pos = np.asarray(pos, dtype=np.float64)
    counts = []
    for lo, hi in reg:
        sub = pos[lo:hi].copy()
        sub[0] = np.inf
        counts.append([np.minimum(path_count(z[:, lo:hi].astype(np.uint8), sub, unit, l), M) for l in L])
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        p = p / p.sum()
        for g in range(len(reg)):
            for k in range(len(L)):
                out[i, g, k] = np.bincount(counts[g][k], weights=p, minlength=M + 1)
    return out


def spread(a, b):
    """Largest |A - B| of two arrays of records."""
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def sampler_check(counts, prob, min_len, tag=""):
    """longest_util.sampler_check's rule on counts [R][I][K] (path_count of R draws at the K
    thresholds) and the exact prob of the whole data [I][K][M + 1]: per threshold and per
    probability prob[c] the cohort total of the draws with that count (c = M: M or more) within
    5 standard errors sqrt(sum p (1 - p) / R) of the exact total, and every individual within
    5 sqrt(p (1 - p) / R); no case is left out.  Returns the largest |z| (0 / 0 counts as 0)."""
    R = counts.shape[0]
    M = prob.shape[-1] - 1
    worst = 0.0
    for k, l in enumerate(np.atleast_1d(min_len)):
        for c in range(M + 1):
            p = np.clip(prob[:, k, c], 0.0, 1.0)
            hit = counts[:, :, k] == c if c < M else counts[:, :, k] >= M
            freq = hit.mean(axis=0)                                              # [I]
            var = p * (1 - p) / R
            dev, se = abs(freq.sum() - p.sum()), np.sqrt(var.sum())
            assert dev <= 5 * se, (tag, k, c, "cohort", dev, se)
            devi = np.abs(freq - p)
            assert (devi <= 5 * np.sqrt(var)).all(), (tag, k, c, devi.max())
            with np.errstate(invalid="ignore", divide="ignore"):
                zi = np.where(devi > 0, devi / np.sqrt(var), 0.0)
            worst = max(worst, dev / se if se > 0 else 0.0, float(zi.max()))
    return worst


# The spread of the two yardsticks on support_util.gpu_cohort, largest |A - B| per unit over all
# the region sets of expect_util.region_sets(5003, pos, 80), the thresholds bylength_util.COHORT_LEN
# and M = 16, as tests/test_count_cpu.py measures and prints it (float64 run-start chain against the
# longdouble recursion).  To re-measure: pytest -s tests/test_count_cpu.py -k spread, and copy the
# printed maxima.  Nothing here is taken from a device.
SPREAD = {"sites": 7.727e-14, "mb": 1.005e-13}
# 16 x the spread, support_util's rule and margin
TOL = {u: 16 * v for u, v in SPREAD.items()}
