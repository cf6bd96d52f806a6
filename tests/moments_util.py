"""The yardstick of the posterior-moment tests (nghmm_ibd_moments, include/nghmm.h), in numpy,
twice, plus brute force:

(A) float64 jets of the statistics CENTRED PER SITE by their own posterior terms (pi_s(1), start_s,
    mb_s of expect_util.terms_a): two passes, the first for the terms; the means are the sums of
    the terms plus a closing correction of the order of rounding;
(B) uncentred jets in np.longdouble: one pass, Var = Z_AA / Z - (Z_A / Z)^2 as it stands.

Both carry, per individual, the forward vector times the second-order jet of the current region
(six components of two entries), normalised to sum 1 of the value component at every site, and
close with a backward vector normalised likewise; both are vectorised over the individuals AND over
region sets: a list of region sets takes one pass.  enumerate_moments is brute force over all 2^S
paths (S <= 12) from the path probabilities and the paths' own statistics.
tests/test_moments_cpu.py checks A and B against it before tests/test_gpu_moments.py uses B.  The
device uses a third arrangement (one pass, centred by offsets that move with the products)."""
import numpy as np

import expect_util as xu
import sample_util as su

FIELDS = ("mean_a", "mean_t", "var_a", "cov_at", "var_t")
DTYPE = np.dtype([(f, np.float64) for f in FIELDS])
LENGTHS = ("sites", "mb")


def _site_ops(eprob, pos, F, alpha, dtype):
    """M [I][S][2][2] = T_s diag(e_s) (the emissions relative to the cell's larger one), q [I][2]."""
    eprob = np.asarray(eprob)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,)).astype(dtype)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)).astype(dtype)
    posf = np.asarray(pos, dtype=np.float64)
    start = np.isinf(posf)
    d = np.where(start, 0.0, posf).astype(dtype)
    c = np.exp(-alpha[:, None] * d[None, :])
    c[:, start] = 0
    q = np.stack([1 - F, F], axis=1)
    ep = eprob.astype(dtype)
    e = np.exp(ep - ep.max(axis=2, keepdims=True))
    T = (1 - c)[..., None, None] * q[:, None, None, :] + c[..., None, None] * np.eye(2, dtype=dtype)
    return T * e[:, :, None, :], q


def _masks(pos, length, dtype):
    """phiA, phiT [S][2][2] (k, l) of include/nghmm.h."""
    posf = np.asarray(pos, dtype=np.float64)
    S = len(posf)
    cs = xu.chrom_start(posf)
    d = np.where(np.isinf(posf), 0.0, posf)
    pa = np.zeros((S, 2, 2), dtype=dtype)
    pt = np.zeros((S, 2, 2), dtype=dtype)
    if length == "sites":
        pa[:, :, 1] = 1
    else:
        pa[:, 1, 1] = np.where(cs, 0.0, d)
    pt[:, 0, 1] = 1
    pt[cs, 1, 1] = 1
    return pa, pt


def _moments(eprob, pos, F, alpha, region_sets, length, dtype, centre):
    assert length in LENGTHS
    sets = [np.asarray(r, dtype=np.int64).reshape(-1, 2) for r in region_sets]
    M, q = _site_ops(eprob, pos, F, alpha, dtype)
    I, S = M.shape[:2]
    K = len(sets)
    pa, pt = _masks(pos, length, dtype)
    if centre is not None:
        ca, ct = (np.asarray(x, dtype=dtype) for x in centre)       # [I][S]
    # backward vectors behind every site, normalised
    beta = np.empty((I, S + 1, 2), dtype=dtype)
    w = np.ones((I, 2), dtype=dtype)
    beta[:, S] = w
    for s in range(S - 1, -1, -1):
        w = np.einsum("ikl,il->ik", M[:, s], w)
        w = w / w.sum(axis=1, keepdims=True)
        beta[:, s] = w
    begins = np.zeros((K, S), dtype=bool)
    ends = np.full((K, S), -1, dtype=np.int64)
    for k, r in enumerate(sets):
        begins[k, r[:, 0]] = True
        ends[k, r[:, 1] - 1] = np.arange(len(r))
    out = [np.zeros((I, len(r)), dtype=DTYPE) for r in sets]
    x = np.zeros((K, I, 6, 2), dtype=dtype)                          # V, A, T, AA, AT, TT
    x[:, :, 0] = q[None]
    off = np.zeros((K, I, 2), dtype=dtype)                           # the centres added so far
    for s in range(S):
        b = begins[:, s]
        if b.any():
            x[b, :, 1:] = 0
            off[b] = 0
        m = M[:, s]                                                  # [I][2][2]
        if centre is None:
            fa, ft = pa[s][None], pt[s][None]
        else:
            fa, ft = pa[s][None] - ca[:, s, None, None], pt[s][None] - ct[:, s, None, None]
            off[:, :, 0] += ca[None, :, s]
            off[:, :, 1] += ct[None, :, s]
        mul = lambda v, mat: np.einsum("kij,ijl->kil", v, mat)
        V, A, T_, AA, AT, TT = (x[:, :, c] for c in range(6))
        n = np.empty_like(x)
        n[:, :, 0] = mul(V, m)
        n[:, :, 1] = mul(A, m) + mul(V, m * fa)
        n[:, :, 2] = mul(T_, m) + mul(V, m * ft)
        n[:, :, 3] = mul(AA, m) + 2 * mul(A, m * fa) + mul(V, m * fa * fa)
        n[:, :, 4] = mul(AT, m) + mul(A, m * ft) + mul(T_, m * fa) + mul(V, m * fa * ft)
        n[:, :, 5] = mul(TT, m) + 2 * mul(T_, m * ft) + mul(V, m * ft * ft)
        x = n / n[:, :, 0].sum(axis=2)[:, :, None, None]
        for k in np.flatnonzero(ends[:, s] >= 0):
            z = np.einsum("icl,il->ic", x[k], beta[:, s + 1])        # [I][6]
            with np.errstate(invalid="ignore", divide="ignore"):
                g = z[:, 1:] / z[:, :1]
            ga, gt = g[:, 0], g[:, 1]
            o = out[k]
            r = ends[k, s]
            o["mean_a"][:, r] = off[k, :, 0] + ga
            o["mean_t"][:, r] = off[k, :, 1] + gt
            o["var_a"][:, r] = np.maximum(g[:, 2] - ga * ga, 0)
            o["cov_at"][:, r] = g[:, 3] - ga * gt
            o["var_t"][:, r] = np.maximum(g[:, 4] - gt * gt, 0)
    return out


def moments_a(eprob, pos, F, alpha, region_sets, length):
    """Yardstick A: [set] of [I][R] records of DTYPE."""
    t = xu.terms_a(eprob, pos, F, alpha)
    centre = (t["ibd"] if length == "sites" else t["mb"], t["start"])
    return _moments(eprob, pos, F, alpha, region_sets, length, np.float64, centre)


def moments_b(eprob, pos, F, alpha, region_sets, length):
    """Yardstick B: uncentred, np.longdouble."""
    return _moments(eprob, pos, F, alpha, region_sets, length, np.longdouble, None)


def path_terms(z, pos):
    """(phiN, phiT, phiL) [paths][S] of paths z [paths][S] (0/1): the terms sample_util.path_stats
    adds to ibd_sites, n_tracts and ibd_mb, site by site."""
    z = np.asarray(z).astype(bool)
    posf = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(posf)[None, :]
    prev = np.concatenate([np.zeros((len(z), 1), dtype=bool), z[:, :-1]], axis=1)
    d = np.where(np.isinf(posf), 0.0, posf)[None, :]
    return (z.astype(np.float64), (z & (~prev | cs)).astype(np.float64),
            np.where(z & prev & ~cs, d, 0.0))


def enumerate_moments(eprob, pos, F, alpha, regions, length):
    """Brute force over all 2^S paths (S <= 12): [I][R] records of DTYPE from the path
    probabilities and the paths' statistics restricted to every region."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12 and length in LENGTHS
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    c = su.coancestry(alpha, pos)
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1
    e = np.exp(eprob)
    pn, pt, pl = path_terms(z, pos)
    st = su.path_stats(z.astype(np.uint8)[None], pos)[0]
    assert np.array_equal(pn.sum(axis=1), st["ibd_sites"]) and np.array_equal(pt.sum(axis=1), st["n_tracts"])
    np.testing.assert_allclose(pl.sum(axis=1), st["ibd_mb"], rtol=1e-14)
    pa = pn if length == "sites" else pl
    out = np.zeros((I, len(reg)), dtype=DTYPE)
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        p = p / p.sum()
        for r, (a, b) in enumerate(reg):
            A, T_ = pa[:, a:b].sum(axis=1), pt[:, a:b].sum(axis=1)
            ma, mt = (p * A).sum(), (p * T_).sum()
            out[i, r] = (ma, mt, (p * (A - ma) ** 2).sum(), (p * (A - ma) * (T_ - mt)).sum(),
                         (p * (T_ - mt) ** 2).sum())
    return out


def spread(a, b):
    """Largest |A - B| per field of two record arrays."""
    return {f: float(np.max(np.abs(a[f] - b[f]))) if a[f].size else 0.0 for f in FIELDS}


def small_regions(S=12, cs=7):
    """The region sets of the 3 x 12 case: the whole data, the chromosomes, [3, 9) (a chromosome
    start inside), every single site."""
    return {"whole": np.array([[0, S]]), "chrom": np.array([[0, cs], [cs, S]]),
            "mid": np.array([[3, 9]]), "cells": xu.single_site_regions(S)}


def confident_case(pkg):
    """4 x 20011, two chromosomes: a true path with mean run length 400, emission log-ratios
    ln(e1 / e0) drawn N(+-1.5, 1) around it (clipped to [-6, 4.5]) and realised by likelihoods at
    frequency 0.01 -- a chain whose posterior is confident, with long tracts: the means are large
    and the variances small, which is where an uncentred float64 jet loses its digits.
    Returns (log likelihoods [S][I][3], distances, indF, alpha, freq, regions [2][R][2])."""
    rng = np.random.default_rng(101)
    I, S, f = 4, 20011, 0.01
    z = np.zeros((I, S), dtype=bool)
    for i in range(I):
        s, state = 0, bool(i & 1)
        while s < S:
            n = int(rng.geometric(1 / 400.0))
            z[i, s:s + n] = state
            state = not state
            s += n
    ell = np.clip(rng.normal(np.where(z, 1.5, -1.5), 1.0), -6.0, 4.5)           # [I][S]
    # p = (1e-12, x, 1): e1 / e0 = (f + 1e-12 (1 - f)) / (f^2 + 2 x f (1 - f) + 1e-12 (1 - f)^2)
    x = np.maximum((np.exp(-ell) - f) / (2 * (1 - f)), 0.0)
    p = np.stack([np.full((I, S), 1e-12), x, np.ones((I, S))], axis=-1)
    gl = np.log(p / p.max(axis=-1, keepdims=True)).transpose(1, 0, 2)           # [S][I][3]
    pos = rng.uniform(0.0005, 0.002, S)
    pos[0] = pos[9973] = np.inf
    F = np.array([0.4, 0.5, 0.55, 0.6])
    A = np.full(I, 1.0 / (400 * 0.00125))
    regions = {"whole": np.array([[0, S]]), "inner": np.array([[3001, 16789]])}
    return np.ascontiguousarray(gl), pos, F, A, f, regions


# The lane length the spread is measured with (expect_util.SPREAD_LANE_SITES: what
# NgsFHMM.layout() reports for the 20 x 5003 cohort with one wave per individual).
SPREAD_LANE_SITES = xu.SPREAD_LANE_SITES
# The spread of the two yardsticks, largest |A - B| per length and field, (1) on
# support_util.gpu_cohort over all the region sets of expect_util.region_sets(5003, pos, 80) and
# (2) on confident_case over its two regions, as tests/test_moments_cpu.py measures and prints them
# (float64 centred per site against uncentred longdouble).  See there for how to re-measure.
# Nothing here is taken from a device.
COHORT_SPREAD = {
    "sites": {"mean_a": 1.819e-11, "mean_t": 5.4e-13, "var_a": 8.185e-10, "cov_at": 1.876e-12, "var_t": 3.268e-13},
    "mb": {"mean_a": 1.535e-12, "mean_t": 5.4e-13, "var_a": 9.038e-12, "cov_at": 2.238e-13, "var_t": 3.268e-13},
}
CONFIDENT_SPREAD = {
    "sites": {"mean_a": 6.185e-11, "mean_t": 1.528e-13, "var_a": 6.577e-10, "cov_at": 8.375e-13, "var_t": 4.961e-15},
    "mb": {"mean_a": 4.974e-14, "mean_t": 1.528e-13, "var_a": 2.092e-15, "cov_at": 2.391e-15, "var_t": 4.961e-15},
}
# 16 x the spread, the project's rule and margin (expect_util.REGION_TOL): the device groups and
# rescales its products unlike either restatement.
COHORT_TOL = {L: {k: 16 * v for k, v in d.items()} for L, d in COHORT_SPREAD.items()}
CONFIDENT_TOL = {L: {k: 16 * v for k, v in d.items()} for L, d in CONFIDENT_SPREAD.items()}

# draws and seed of the tests against the sampler: tests/test_moments_cpu.py checks on the
# restatement of the sampler that the cohort satisfies sampler_check with them
SAMPLER_DRAWS, SAMPLER_SEED = xu.SAMPLER_DRAWS, xu.SAMPLER_SEED


def _var_z(x, want):
    """|s^2 - want| / se per column of x [R][n], se = sqrt((m4 - s^4) / R) with the fourth central
    sample moment m4; (z, vary)."""
    R = x.shape[0]
    dx = x - x.mean(axis=0)
    s2 = (dx ** 2).sum(axis=0) / (R - 1)
    m4 = (dx ** 4).mean(axis=0)
    vary = s2 > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(np.maximum(m4 - s2 ** 2, 0) / R)
        z = np.abs(s2 - want) / se
    return z, vary & (se > 0)


def sampler_check(stats, sites, mb):
    """The condition of the tests against the sampler, on stats [R][I] (path statistics of R draws)
    and the exact whole-data records [I] for both lengths: per statistic (ibd_sites, n_tracts,
    ibd_mb) the sample variance of the draws per individual within 5 standard errors of the exact
    variance (se = sqrt((m4 - s^4) / R)), the same for the cohort total against the sum of the
    individuals' variances, the sample covariance of (ibd_sites, n_tracts) within 5 standard
    errors of cov_at, and at most 5 of 20 individuals left out per statistic because their draws
    do not vary.  Returns the largest |z| seen."""
    R = stats.shape[0]
    worst = 0.0
    for st, want in (("ibd_sites", sites["var_a"]), ("n_tracts", sites["var_t"]), ("ibd_mb", mb["var_a"])):
        x = stats[st].astype(np.float64)
        z, vary = _var_z(x, want)
        assert (~vary).sum() <= 5, (st, int((~vary).sum()))
        assert (z[vary] <= 5).all(), (st, z[vary].max())
        zt, ok = _var_z(x.sum(axis=1)[:, None], np.array([want.sum()]))
        assert ok.all() and zt[0] <= 5, (st, "cohort", zt[0])
        worst = max(worst, z[vary].max(), zt[0])
    a, t = stats["ibd_sites"].astype(np.float64), stats["n_tracts"].astype(np.float64)
    da, dt = a - a.mean(axis=0), t - t.mean(axis=0)
    prod = da * dt
    cov = prod.sum(axis=0) / (R - 1)
    se = prod.std(axis=0, ddof=1) / np.sqrt(R)
    vary = se > 0
    assert (~vary).sum() <= 5, ("cov", int((~vary).sum()))
    z = np.abs(cov - sites["cov_at"])[vary] / se[vary]
    assert (z <= 5).all(), ("cov", z.max())
    return max(worst, z.max())
