"""The yardstick of the path-expectation tests (nghmm_ibd_expect, include/nghmm.h), in numpy,
twice:

(A) float64 on sample_util.forward_filter and a backward vector normalised at every site: the four
    products n_s(k, l) = f_{s-1}(k) T_s(k, l) e_s(l) beta_s(l) in linear space, ln r from the small
    side with np.log1p;
(B) the direct form xi = f T e beta / Z in log space in np.longdouble.

Both carry exact zeros (an emission that is 0 stays 0): a state the data exclude makes its xi
entries exactly 0, its entropy terms 0 and ln r of a step into it -inf.  enumerate_expect is brute
force over all 2^S paths (S <= 12) and uses the path probabilities alone.
tests/test_expect_cpu.py checks A and B against it before tests/test_gpu_expect.py uses B.  The
device uses a third arrangement (its own rescaling, the lane-chunk grouping of the sums)."""
import numpy as np

import sample_util as su
import support_util as sup

REGION_FIELDS = ("ibd", "starts", "switches", "ibd_mb", "entropy", "log_p_path")
SITE_FIELDS = ("on", "off", "ibd", "entropy")
REGION_DTYPE = np.dtype([(f, np.float64) for f in REGION_FIELDS])
SITE_DTYPE = np.dtype([(f, np.float64) for f in SITE_FIELDS])
# the per-cell terms [I][S] a yardstick returns
TERMS = ("ibd", "start", "on", "off", "mb", "h", "lp")


def chrom_start(pos):
    """Sites that start a chromosome: d = +inf, and the first site."""
    cs = np.isinf(np.asarray(pos, dtype=np.float64))
    cs[0] = True
    return cs


def _ln_share(a, b):
    """ln(a / (a + b)) for a, b >= 0 from the small side; -inf where a == 0 (0/0 included)."""
    a, b = np.broadcast_arrays(a, b)
    big = b <= a
    num, den = np.where(big, b, a), np.where(big, a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = num / den
        out = np.where(big, -np.log1p(x), np.log(a / (a + b)))
    return np.where(a > 0, out, -np.inf)


def _ln_share_log(la, lb):
    """The same from la = ln a, lb = ln b (any float type)."""
    big = lb <= la
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(big, lb - la, la - lb)
        l1p = np.log1p(np.exp(d))
        out = np.where(big, -l1p, (la - lb) - l1p)
    return np.where(np.isneginf(la) | np.isnan(out), -np.inf, out)


def _finish(xi, L, pi_L, pos, cs, path):
    """The per-cell terms from xi [I][S][2][2] (k, l), L = ln r likewise, pi_L [I][S][2] = ln pi."""
    xi = np.asarray(xi, dtype=np.float64)
    I, S = xi.shape[:2]
    pi = xi[:, :, 0, :] + xi[:, :, 1, :]
    st = cs[None, :]
    d = np.where(np.isinf(pos), 0.0, np.asarray(pos, dtype=np.float64))[None, :]

    def plogp(p, lp):
        with np.errstate(invalid="ignore"):
            return np.where(p > 0, p * np.asarray(lp, dtype=np.float64), 0.0)

    h_in = -plogp(xi, L).sum(axis=(2, 3))
    h_st = -plogp(pi, pi_L).sum(axis=2)
    out = {"ibd": pi[..., 1],
           "start": np.where(st, pi[..., 1], xi[:, :, 0, 1]),
           "on": np.where(st, 0.0, xi[:, :, 0, 1]),
           "off": np.where(st, 0.0, xi[:, :, 1, 0]),
           "mb": np.where(st, 0.0, d * xi[:, :, 1, 1]),
           "h": np.where(st, h_st, h_in)}
    if path is not None:
        z = np.asarray(path).astype(np.int64)
        zp = np.concatenate([np.zeros((I, 1), dtype=np.int64), z[:, :-1]], axis=1)
        ii, ss = np.meshgrid(np.arange(I), np.arange(S), indexing="ij")
        lp_in = np.asarray(L, dtype=np.float64)[ii, ss, zp, z]
        lp_st = np.asarray(pi_L, dtype=np.float64)[ii, ss, z]
        out["lp"] = np.where(st, lp_st, lp_in)
    else:
        out["lp"] = np.zeros((I, S))
    return out


def terms_a(eprob, pos, F, alpha, path=None):
    """Yardstick A.  eprob [I][S][2] log emissions, pos [S] distances (+inf: a chromosome start),
    path [I][S] (0/1) or None.  Returns the per-cell terms {name: [I][S]}."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    q = np.stack([1 - F, F], axis=1)
    cs = chrom_start(pos)
    f = su.forward_filter(eprob, pos, F, alpha)
    fprev = np.concatenate([q[:, None, :], f[:, :-1]], axis=1)                 # f_{s-1}
    e = np.exp(eprob - eprob.max(axis=2, keepdims=True))
    c = su.coancestry(alpha, pos)
    xi = np.empty((I, S, 2, 2))
    m = np.empty((I, S, 2, 2))
    w = np.ones((I, 2))
    for s in range(S - 1, -1, -1):
        u = e[:, s] * w                                                        # e_s(l) beta_s(l)
        off = (1 - c[:, s, None]) * q                                          # T(k, l), k != l
        T = np.stack([np.stack([off[:, 0] + c[:, s], off[:, 1]], axis=1),
                      np.stack([off[:, 0], off[:, 1] + c[:, s]], axis=1)], axis=1)   # [I][k][l]
        m[:, s] = T * u[:, None, :]
        w = m[:, s].sum(axis=2)
        w = w / w.sum(axis=1, keepdims=True)
    n = fprev[..., None] * m
    xi = n / n.sum(axis=(2, 3), keepdims=True)
    L = _ln_share(m, m[..., ::-1])
    col = n.sum(axis=2)                                                        # [I][S][l]
    return _finish(xi, L, _ln_share(col, col[..., ::-1]), pos, cs, path)


def terms_b(eprob, pos, F, alpha, path=None):
    """Yardstick B: log space, np.longdouble."""
    ld = np.longdouble
    eprob = np.asarray(eprob).astype(ld)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,)).astype(ld)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)).astype(ld)
    posf = np.asarray(pos, dtype=np.float64)
    cs = chrom_start(posf)
    start = np.isinf(posf)
    d = np.where(start, 0.0, posf).astype(ld)
    c = np.exp(-alpha[:, None] * d[None, :])
    c[:, start] = 0
    q = np.stack([1 - F, F], axis=1)
    with np.errstate(divide="ignore"):
        lq = np.log(q)
        loff = np.log((1 - c)[..., None] * q[:, None, :])                      # ln T_s(j, k), j != k
        ldiag = np.log((1 - c)[..., None] * q[:, None, :] + c[..., None])
    # lT [I][S][k][l]
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
        lm = lT + (eprob + lb)[:, :, None, :]                                  # ln m_s(k, l)
        ln_n = lfprev[..., None] + lm
        ln_n = np.where(np.isnan(ln_n), -np.inf, ln_n)
        lz = np.logaddexp(np.logaddexp(ln_n[..., 0, 0], ln_n[..., 0, 1]),
                          np.logaddexp(ln_n[..., 1, 0], ln_n[..., 1, 1]))
        xi = np.exp(ln_n - lz[..., None, None])
        L = _ln_share_log(lm, lm[..., ::-1])
        lcol = np.logaddexp(ln_n[:, :, 0, :], ln_n[:, :, 1, :])
        lpi = _ln_share_log(lcol, lcol[..., ::-1])
    return _finish(xi, L, lpi, posf, cs, path)


def region_records(terms, regions):
    """[I][R] of REGION_DTYPE: the per-cell terms added over every region [begin, end)."""
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    I = terms["ibd"].shape[0]
    out = np.zeros((I, len(reg)), dtype=REGION_DTYPE)
    for k, (a, b) in enumerate(reg):
        out["ibd"][:, k] = terms["ibd"][:, a:b].sum(axis=1)
        out["starts"][:, k] = terms["start"][:, a:b].sum(axis=1)
        out["switches"][:, k] = (terms["on"][:, a:b] + terms["off"][:, a:b]).sum(axis=1)
        out["ibd_mb"][:, k] = terms["mb"][:, a:b].sum(axis=1)
        out["entropy"][:, k] = terms["h"][:, a:b].sum(axis=1)
        out["log_p_path"][:, k] = terms["lp"][:, a:b].sum(axis=1)
    return out


def site_records(terms):
    """[S] of SITE_DTYPE: the per-cell terms added over the individuals."""
    out = np.zeros(terms["ibd"].shape[1], dtype=SITE_DTYPE)
    out["on"], out["off"] = terms["on"].sum(axis=0), terms["off"].sum(axis=0)
    out["ibd"], out["entropy"] = terms["ibd"].sum(axis=0), terms["h"].sum(axis=0)
    return out


def enumerate_expect(eprob, pos, F, alpha, path=None):
    """Brute force over all 2^S paths (S <= 12), from the path probabilities alone.  Returns
    (totals, terms): totals = {n_tracts, ibd_sites, ibd_mb, switches, entropy, log_p_path}, each
    [I] (E[.] of sample_util.path_stats' statistics, the number of switches inside chromosomes,
    H = -sum p ln p, ln P(path | y)), and the per-cell terms {name: [I][S]} from the enumerated
    pairwise marginals; lp is NaN where the path leaves a state of probability 0 (0/0)."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    c = su.coancestry(alpha, pos)
    cs = chrom_start(pos)
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1              # [paths][S]
    e = np.exp(eprob)
    stats = su.path_stats(z.astype(np.uint8)[None], pos)[0]                    # [paths]
    sw = ((z[:, 1:] != z[:, :-1]) & ~cs[None, 1:]).sum(axis=1)
    tot = {k: np.empty(I) for k in ("n_tracts", "ibd_sites", "ibd_mb", "switches", "entropy", "log_p_path")}
    xi = np.zeros((I, S, 2, 2))
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        p = p / p.sum()
        tot["n_tracts"][i] = (p * stats["n_tracts"]).sum()
        tot["ibd_sites"][i] = (p * stats["ibd_sites"]).sum()
        tot["ibd_mb"][i] = (p * stats["ibd_mb"]).sum()
        tot["switches"][i] = (p * sw).sum()
        nz = p > 0
        tot["entropy"][i] = -(p[nz] * np.log(p[nz])).sum()
        if path is not None:
            idx = int((np.asarray(path[i]).astype(np.int64) << np.arange(S)).sum())
            with np.errstate(divide="ignore"):
                tot["log_p_path"][i] = np.log(p[idx])
        else:
            tot["log_p_path"][i] = 0.0
        for s in range(S):
            for l in (0, 1):
                if s == 0:
                    xi[i, 0, 0, l] = p[z[:, 0] == l].sum()                     # (k has no meaning)
                else:
                    for k in (0, 1):
                        xi[i, s, k, l] = p[(z[:, s - 1] == k) & (z[:, s] == l)].sum()
    pi = xi.sum(axis=2)
    row = xi.sum(axis=3, keepdims=True)                                        # pi_{s-1}(k)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.log(xi / row)
        lpi = np.log(pi)
    # (a 0/0 entry -- a step out of a state that the data exclude -- stays NaN: the path
    # probabilities alone do not define it; only lp of a path through such a state shows it)
    return tot, _finish(xi, L, lpi, np.asarray(pos, dtype=np.float64), cs, path)


def small_case():
    """3 x 12: two chromosomes (a start at site 7), random likelihoods with a missing cell
    (uniform likelihoods) and one called heterozygote ((0, 1, 0): the IBD state is excluded), one
    frequency per site.  Returns (log emissions, distances, indF, alpha, path): the path of
    individual 1 goes through the excluded state, so its log_p_path is -inf."""
    rng = np.random.default_rng(23)
    I, S = 3, 12
    gl = np.log(rng.dirichlet(np.ones(3), size=(S, I)))
    gl[2, 0] = np.log(1.0 / 3.0)
    with np.errstate(divide="ignore"):
        gl[4, 1] = np.log(np.array([0.0, 1.0, 0.0]))
    pos = rng.uniform(0.01, 0.6, S)
    pos[0] = pos[7] = np.inf
    freq = rng.uniform(0.1, 0.5, S)
    e = su.emissions_np(gl, freq)
    F, A = np.array([0.3, 0.6, 0.85]), np.array([0.4, 1.5, 0.05])
    path = np.array([[0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0],
                     [1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1],
                     [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]], dtype=np.uint8)
    return e, pos, F, A, path, gl, freq


def single_site_regions(S):
    return np.stack([np.arange(S), np.arange(S) + 1], axis=1).astype(np.int64)


def region_sets(n_sites, pos, lane_sites):
    """Region sets {name: [R][2]} in the spirit of support_util.hand_ranges: the chromosomes;
    windows of 7, 64, 2048 and 2049 sites; single sites on both sides of every lane-chunk boundary
    (multiples of lane_sites, if > 0); a region across a chromosome start among regions with
    gaps; the whole data.  Each set is sorted and disjoint."""
    S = n_sites
    cs = np.flatnonzero(chrom_start(pos))
    sets = {"whole": np.array([[0, S]], dtype=np.int64),
            "chrom": np.stack([cs, np.r_[cs[1:], S]], axis=1).astype(np.int64)}
    for w in (7, 64, 2048, 2049):
        b = np.arange(0, S, w)
        sets[f"win{w}"] = np.stack([b, np.minimum(b + w, S)], axis=1).astype(np.int64)
    if lane_sites:
        t = np.arange(lane_sites, S, lane_sites)
        one = np.unique(np.r_[t - 1, t, 0, S - 1])
        sets["edges"] = np.stack([one, one + 1], axis=1).astype(np.int64)
    gaps = []
    if len(cs) > 1:
        gaps.append((max(int(cs[1]) - 13, 0), int(cs[1]) + 17))                # across a start
    lo = gaps[-1][1] + 5 if gaps else 3
    k = 0
    while lo + 40 < S:                                                         # odd ends, gaps between
        n = 1 if k % 3 == 0 else 9 + 11 * (k % 8)
        gaps.append((lo, min(lo + n, S)))
        lo += n + 1 + 37 * (k % 5)
        k += 1
    sets["gaps"] = np.array(sorted(gaps), dtype=np.int64)
    return sets


def spread(a, b):
    """Largest |A - B| per field of two record arrays (wherever both are finite)."""
    out = {}
    for f in a.dtype.names:
        fin = np.isfinite(a[f]) & np.isfinite(b[f])
        out[f] = float(np.max(np.abs(a[f][fin] - b[f][fin]))) if fin.any() else 0.0
    return out


# draws and seed of the test against the sampler: tests/test_expect_cpu.py checks on the
# restatement of the sampler that the cohort satisfies sampler_check with them
SAMPLER_DRAWS, SAMPLER_SEED = 400, 77


def sampler_check(stats, exact):
    """The condition of the test against the sampler, on stats [R][I] (path statistics of R draws)
    and the exact region records of the whole data [I]: the cohort totals of the draw means within
    5 standard errors of the exact totals, the same per individual whose draws vary, and at most 5
    of 20 individuals without variance per statistic.  Returns the largest |z| seen."""
    R = stats.shape[0]
    worst = 0.0
    for st, f in (("n_tracts", "starts"), ("ibd_sites", "ibd"), ("ibd_mb", "ibd_mb")):
        x = stats[st].astype(np.float64)                                     # [R][I]
        tot = x.sum(axis=1)
        se = tot.std(ddof=1) / np.sqrt(R)
        z = abs(tot.mean() - exact[f].sum()) / se
        assert z <= 5, (st, "cohort", z)
        worst = max(worst, z)
        sd = x.std(axis=0, ddof=1)
        vary = sd > 0
        assert (~vary).sum() <= 5, (st, int((~vary).sum()))
        zi = np.abs(x.mean(axis=0) - exact[f])[vary] / (sd[vary] / np.sqrt(R))
        assert (zi <= 5).all(), (st, zi.max())
        worst = max(worst, zi.max())
    return worst


# The lane length the spread is measured with: what NgsFHMM.layout() reports for the 20 x 5003
# cohort of support_util.gpu_cohort with ONE wave per individual (NGHMM_FAST_C=1; by itself the
# cohort gets 5 waves and lanes of 16 sites, tests/test_gpu_layouts.py prints both).  The region
# sets only use it to place single-site regions, and exact mode's tests fall back on it.
SPREAD_LANE_SITES = 80
# The spread of the two yardsticks on support_util.gpu_cohort, largest |A - B| per field over all
# the region sets of region_sets(5003, pos, 80) and over the site records, with the decoded path
# taken from yardstick B's own posteriors (>= 0.5), as tests/test_expect_cpu.py measures and prints
# it (float64 linear space against longdouble log space).  See there for how to re-measure.
# The largest figures belong to the longest regions (the whole data: sums of 5003 terms, ibd of
# the order of a thousand); nothing here is taken from a device.
REGION_SPREAD = {"ibd": 1.091e-11, "starts": 9.27e-14, "switches": 9.77e-14, "ibd_mb": 1.023e-12,
                 "entropy": 6.182e-13, "log_p_path": 2.405e-12}
SITE_SPREAD = {"on": 5.324e-14, "off": 5.618e-14, "ibd": 1.208e-13, "entropy": 2.744e-13}
# 16 x the spread, support_util's rule and margin: the device groups and rescales its products
# unlike either restatement.
REGION_TOL = {k: 16 * v for k, v in REGION_SPREAD.items()}
SITE_TOL = {k: 16 * v for k, v in SITE_SPREAD.items()}
