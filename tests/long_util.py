"""The yardstick of the tests of nghmm_ibd_long (include/nghmm.h), in numpy, twice, on the cells
of tests/bylength_util.py:

(A) float64, linear space, on cells_a: W(lo, s) as a running product per window width, T_k from
    bylength_util.terms_a, and B_k(s) as the terms of the window themselves, added from s
    backwards -- no prefix, no difference;
(B) np.longdouble on cells_b: W = exp(Q_s - Q_lo) from the prefix of ln rho and B_k(s) as a
    difference of the prefix of T_k, both restarting at every blocked step.

Both carry exact zeros.  enumerate_long is brute force over all 2^S paths (S <= 12) from the path
probabilities and the tract definition alone: it uses none of the formulas.
tests/test_long_cpu.py checks A and B against the enumeration before tests/test_gpu_long.py uses
B.  The device uses a third arrangement (its own rescaling, the lane-chunk grouping of the
prefixes)."""
import numpy as np

import bylength_util as bu
import expect_util as xu
import sample_util as su

REGION_FIELDS = ("sites", "mb")
SITE_FIELDS = ("sum", "count")
REGION_DTYPE = np.dtype([(f, np.float64) for f in REGION_FIELDS])
SITE_DTYPE = np.dtype([("sum", np.float64), ("count", np.uint64)])
NONE = -1


def window_starts(pos, min_len, unit):
    """lo_k(s) [K][S]: the largest a <= s in s's chromosome with len(a, s) >= L_k, NONE if there is
    none; from the definition (every pair of sites of a chromosome is tested)."""
    pos = np.asarray(pos, dtype=np.float64)
    S = len(pos)
    L = np.atleast_1d(np.asarray(min_len, dtype=np.float64))
    cs = np.flatnonzero(xu.chrom_start(pos))
    cum = bu.cum_mb(pos)
    out = np.full((len(L), S), NONE, dtype=np.int64)
    for c0, c1 in zip(cs, np.r_[cs[1:], S]):
        idx = np.arange(c0, c1)
        if unit == "mb":
            ln = cum[None, c0:c1] - cum[c0:c1, None]                           # [a][s]
        else:
            ln = (idx[None, :] - idx[:, None] + 1).astype(np.float64)
        behind = idx[:, None] <= idx[None, :]
        for k, l in enumerate(L):
            ok = behind & (ln >= l)                                            # [a][s]
            last = (c1 - c0 - 1) - ok[::-1].argmax(axis=0)
            out[k, c0:c1] = np.where(ok.any(axis=0), c0 + last, NONE)
    return out


def _back_reach(pos, lo):
    """How far back the window sum of every site goes, [K][S]: s - lo_k(s), or s - c0 + 1 without lo."""
    S = len(pos)
    cs = xu.chrom_start(pos)
    c0 = np.maximum.accumulate(np.where(cs, np.arange(S), 0))
    s = np.arange(S)[None, :]
    return np.where(lo >= 0, s - lo, s - c0[None, :] + 1)


def post_a(eprob, pos, F, alpha, min_len, unit):
    """Yardstick A: (P, T), each [K][I][S] float64."""
    sigma, rho = bu.cells_a(eprob, pos, F, alpha)
    pi = xu.terms_a(eprob, pos, F, alpha)["ibd"]
    I, S = sigma.shape
    tr, _ = bu.terms_a(eprob, pos, F, alpha, min_len, unit)                    # [I][S][K]
    T = np.ascontiguousarray(np.moveaxis(tr, 2, 0))
    lo = window_starts(pos, min_len, unit)
    K = len(lo)
    reach = _back_reach(pos, lo)
    live = T.reshape(K, -1).any(axis=1)
    P = np.zeros((K, I, S))
    W = np.ones((I, S))                                                        # W(a, a + w)
    acc = np.zeros((K, I, S))                                                  # T_k(s) + .. + T_k(s - w + 1)
    for w in range(int(reach.max()) + 1):
        if w:
            W[:, :S - w] *= rho[:, w:]
            W[:, S - w:] = 0.0
        for k in range(K):
            s = np.flatnonzero(reach[k] == w)
            if len(s):
                with_lo = lo[k, s] >= 0
                a = np.where(with_lo, lo[k, s], 0)
                P[k][:, s] = np.where(with_lo[None, :], pi[:, a] * W[:, a], 0.0) + acc[k][:, s]
            if live[k] and w < S:
                acc[k][:, w:] += T[k][:, :S - w]
    return np.minimum(P, pi[None]), T


def post_b(eprob, pos, F, alpha, min_len, unit):
    """Yardstick B: the same in np.longdouble from ln rho and two prefixes, returned as float64."""
    ld = np.longdouble
    sigma, lrho = bu.cells_b(eprob, pos, F, alpha)
    pi = xu.terms_b(eprob, pos, F, alpha)["ibd"]
    I, S = sigma.shape
    blocked = np.isneginf(lrho)
    Q = np.zeros((I, S), dtype=ld)
    q = np.zeros(I, dtype=ld)
    for s in range(S):
        q = np.where(blocked[:, s], ld(0), q + np.where(blocked[:, s], ld(0), lrho[:, s]))
        Q[:, s] = q
    n = np.cumsum(blocked, axis=1)
    bk = bu.window_ends(pos, min_len, unit)
    lo = window_starts(pos, min_len, unit)
    K = len(bk)
    P = np.zeros((K, I, S))
    Tout = np.zeros((K, I, S))
    for k in range(K):
        T = np.zeros((I, S), dtype=ld)
        a = np.flatnonzero(bk[k] >= 0)
        b = bk[k, a]
        T[:, a] = sigma[:, a].astype(ld) * np.where(n[:, b] == n[:, a], np.exp(Q[:, b] - Q[:, a]), ld(0))
        U = np.zeros((I, S), dtype=ld)
        u = np.zeros(I, dtype=ld)
        for s in range(S):
            u = np.where(blocked[:, s], T[:, s], u + T[:, s])
            U[:, s] = u
        with_lo = lo[k] >= 0
        l = np.where(with_lo, lo[k], 0)
        same = with_lo[None, :] & (n[:, l] == n)
        with np.errstate(over="ignore", invalid="ignore"):
            A = np.where(same, pi[:, l].astype(ld) * np.exp(np.where(same, Q - Q[:, l], ld(0))), ld(0))
        B = np.where(same, np.maximum(U - U[:, l], ld(0)), U)
        P[k] = np.minimum((A + B).astype(np.float64), pi)
        Tout[k] = T.astype(np.float64)
    return P, Tout


def region_records(PT, pos, regions):
    """[I][R][K] of REGION_DTYPE from (P, T): sites = sum of P over the region; mb = sum of
    d_s (P - T) over its sites that are no chromosome start."""
    P, T = PT
    pos = np.asarray(pos, dtype=np.float64)
    d = np.where(xu.chrom_start(pos), 0.0, np.where(np.isinf(pos), 0.0, pos))
    joint = d[None, None, :] * (P - T)
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((P.shape[1], len(reg), P.shape[0]), dtype=REGION_DTYPE)
    for r, (a, b) in enumerate(reg):
        out["sites"][:, r] = P[:, :, a:b].sum(axis=2).T
        out["mb"][:, r] = joint[:, :, a:b].sum(axis=2).T
    return out


def site_records(P, threshold=0.5):
    """[S][K] of SITE_DTYPE: P added over the individuals in index order, and the individuals at or
    above the threshold."""
    K, I, S = P.shape
    out = np.zeros((S, K), dtype=SITE_DTYPE)
    acc = np.zeros((K, S))
    for i in range(I):
        acc += P[:, i]
    out["sum"] = acc.T
    out["count"] = (P >= threshold).sum(axis=1).T
    return out


def path_long(paths, pos, min_len, unit):
    """Of given 0/1 paths [N][S]: [N][K][S] bool, whether the site lies in a tract (a run of 1 cut at
    chromosome starts) of length >= L_k, in sites or in Mb (first site to last)."""
    z = np.asarray(paths).astype(bool)
    N, S = z.shape
    pos = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(pos)
    d = np.where(np.isinf(pos), 0.0, pos)
    L = np.atleast_1d(np.asarray(min_len, dtype=np.float64))
    prev = np.concatenate([np.zeros((N, 1), dtype=bool), z[:, :-1]], axis=1)
    st = z & (~prev | cs[None, :])
    run = np.cumsum(st, axis=1)                                                # [N][S], 1-based inside runs
    nr = S + 1
    gid = (np.arange(N)[:, None] * nr + run)[z]
    sites = np.bincount(gid, minlength=N * nr).reshape(N, nr)
    if unit == "mb":
        lens = np.bincount(gid, weights=np.where(st, 0.0, d[None, :])[z], minlength=N * nr).reshape(N, nr)
    else:
        lens = sites.astype(np.float64)
    out = np.zeros((N, len(L), S), dtype=bool)
    for k, l in enumerate(L):
        sel = (sites > 0) & (lens >= l)
        out[:, k] = z & np.take_along_axis(sel, run, axis=1)
    return out


def enumerate_long(eprob, pos, F, alpha, min_len, unit):
    """Brute force over all 2^S paths (S <= 12): (P, J), each [K][I][S]: P = P(s lies in a tract of
    length >= L_k | y) and J = P(s - 1 and s lie in the same such tract | y) (0 at a chromosome
    start), from the path probabilities and path_long alone."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    c = su.coancestry(alpha, pos)
    cs = xu.chrom_start(pos)
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1
    e = np.exp(eprob)
    inl = path_long(z.astype(np.uint8), pos, min_len, unit).astype(np.float64)      # [paths][K][S]
    zprev = np.concatenate([np.zeros((len(z), 1), dtype=np.int64), z[:, :-1]], axis=1)
    both = inl * ((zprev == 1) & ~cs[None, :])[:, None, :]
    K = inl.shape[1]
    P = np.empty((K, I, S))
    J = np.empty((K, I, S))
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        p = p / p.sum()
        P[:, i] = np.tensordot(p, inl, axes=(0, 0))
        J[:, i] = np.tensordot(p, both, axes=(0, 0))
    return P, J


def enumerated_regions(PJ, pos, regions):
    """region_records' layout from enumerate_long's (P, J)."""
    P, J = PJ
    return region_records((P, P - J), pos, regions)


def spread(a, b):
    """Largest |A - B| per field of two record arrays."""
    return {f: float(np.max(np.abs(a[f].astype(np.float64) - b[f].astype(np.float64)))) if a[f].size else 0.0
            for f in a.dtype.names}


# The spread of the two yardsticks on support_util.gpu_cohort, largest |A - B| per unit and output
# field -- post [K][I][S]; sum of the site records; sites and mb of the region records over all the
# region sets of expect_util.region_sets(5003, pos, 80) -- at the thresholds bylength_util.COHORT_LEN,
# as tests/test_long_cpu.py measures and prints it (float64 running products and plain window sums
# against longdouble prefixes).  See there for how to re-measure.  The largest figures belong to
# the whole data (sums of 5003 terms); nothing here is taken from a device.
SPREAD = {"sites": {"post": 1.007e-13, "sum": 1.226e-13, "sites": 2.183e-11, "mb": 2.217e-12},
          "mb": {"post": 1.006e-13, "sum": 1.208e-13, "sites": 1.091e-11, "mb": 1.023e-12}}
# 16 x the spread, support_util's rule and margin: the device groups and rescales its products
# unlike either restatement.
TOL = {u: {f: 16 * v for f, v in s.items()} for u, s in SPREAD.items()}
