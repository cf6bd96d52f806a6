"""The yardstick of the tests of nghmm_ibd_by_length (include/nghmm.h), in numpy, twice:

(A) float64, linear space, on sample_util.forward_filter and a backward vector normalised at every
    site: sigma_s and rho_s from the four products, M and D by their recursions, and W(a, b) as a
    running product per start site (all start sites advance by one site per step);
(B) np.longdouble, log space: ln rho from the small side, W(a, b) = exp(Q_b - Q_a) from a prefix
    sum that restarts at every blocked step, M and D by the recursions on exp(ln rho).

Both carry exact zeros: a state the data exclude makes sigma and rho of a step into it exactly 0.
enumerate_by_length is brute force over all 2^S paths (S <= 12) from the path probabilities and
the tract definition alone; path_by_length gives the statistics of given 0/1 paths.
tests/test_bylength_cpu.py checks A and B against the enumeration before
tests/test_gpu_bylength.py uses B.  The device uses a third arrangement (its own rescaling, the
lane-chunk grouping of the sums and of the prefix)."""
import numpy as np

import expect_util as xu
import sample_util as su

FIELDS = ("tracts", "length")
DTYPE = np.dtype([(f, np.float64) for f in FIELDS])
NONE = -1

# the thresholds of the tests (80 and 81 sites straddle a lane length of 80,
# expect_util.SPREAD_LANE_SITES; tests/test_gpu_bylength.py adds T and T + 1 for the lane length T
# the device reports; 2000 sites exceed every chromosome of the cohort)
SMALL_LEN = {"sites": (1, 2, 3, 5), "mb": (0.0, 0.2, 0.7)}
COHORT_LEN = {"sites": (1, 2, 8, 80, 81, 400, 2000), "mb": (0.0, 0.05, 0.5, 2.0, 10.0)}
SAMPLER_LEN = {"sites": (1, 2, 8, 80, 81), "mb": (0.0, 0.5, 2.0, 10.0)}


def cum_mb(pos):
    """cum_s: 0 at a chromosome start, else cum_{s-1} + d_s, in float64 in site order."""
    pos = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(pos)
    out = np.zeros(len(pos))
    c = 0.0
    for s in range(len(pos)):
        c = 0.0 if cs[s] else c + pos[s]
        out[s] = c
    return out


def window_ends(pos, min_len, unit):
    """b_k(a) [K][S]: the smallest b >= a in a's chromosome with len(a, b) >= L_k, NONE if there is
    none; from the definition (every pair of sites of a chromosome is tested)."""
    pos = np.asarray(pos, dtype=np.float64)
    S = len(pos)
    L = np.atleast_1d(np.asarray(min_len, dtype=np.float64))
    cs = np.flatnonzero(xu.chrom_start(pos))
    cum = cum_mb(pos)
    out = np.full((len(L), S), NONE, dtype=np.int64)
    for c0, c1 in zip(cs, np.r_[cs[1:], S]):
        idx = np.arange(c0, c1)
        if unit == "mb":
            ln = cum[None, c0:c1] - cum[c0:c1, None]                           # [a][b]
        else:
            ln = (idx[None, :] - idx[:, None] + 1).astype(np.float64)
        ahead = idx[None, :] >= idx[:, None]
        for k, l in enumerate(L):
            ok = ahead & (ln >= l)
            first = ok.argmax(axis=1)
            out[k, c0:c1] = np.where(ok.any(axis=1), c0 + first, NONE)
    return out


def _window_len(pos, a, b, unit):
    cum = cum_mb(pos)
    return cum[b] - cum[a] if unit == "mb" else (b - a + 1).astype(np.float64)


def cells_a(eprob, pos, F, alpha):
    """Yardstick A's per-cell quantities: (sigma, rho), each [I][S] float64."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    q = np.stack([1 - F, F], axis=1)
    cs = xu.chrom_start(pos)
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
    sigma = np.where(cs[None, :], xi[:, :, 0, 1] + xi[:, :, 1, 1], xi[:, :, 0, 1])
    row = m[:, :, 1, 0] + m[:, :, 1, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(row > 0, m[:, :, 1, 1] / row, 0.0)
    rho[:, cs] = 0.0
    return sigma, rho


def cells_b(eprob, pos, F, alpha):
    """Yardstick B's per-cell quantities: (sigma float64, ln rho longdouble, -inf where blocked)."""
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
        ln_n = lfprev[..., None] + lm
        ln_n = np.where(np.isnan(ln_n), -np.inf, ln_n)
        lz = np.logaddexp(np.logaddexp(ln_n[..., 0, 0], ln_n[..., 0, 1]),
                          np.logaddexp(ln_n[..., 1, 0], ln_n[..., 1, 1]))
        xi = np.exp(ln_n - lz[..., None, None]).astype(np.float64)
        lrho = xu._ln_share_log(lm[:, :, 1, 1], lm[:, :, 1, 0])
    sigma = np.where(cs[None, :], xi[:, :, 0, 1] + xi[:, :, 1, 1], xi[:, :, 0, 1])
    lrho = np.array(lrho, dtype=ld)
    lrho[:, cs] = -np.inf
    return sigma, lrho


def _remaining(rho, pos, unit):
    """rem_s [I][S] by M_s = rho_{s+1} (1 + M_{s+1}) (D: d_{s+1} for 1); a blocked step gives 0."""
    I, S = rho.shape
    d = np.where(np.isinf(pos), 0.0, np.asarray(pos, dtype=np.float64))
    rem = np.zeros((I, S), dtype=rho.dtype)
    for s in range(S - 2, -1, -1):
        inc = d[s + 1] if unit == "mb" else 1.0
        rem[:, s] = np.where(rho[:, s + 1] > 0, rho[:, s + 1] * (inc + rem[:, s + 1]), 0.0)
    return rem


def terms_a(eprob, pos, F, alpha, min_len, unit):
    """Yardstick A: (tracts, length), each [I][S][K] float64: the terms of every start site."""
    sigma, rho = cells_a(eprob, pos, F, alpha)
    I, S = sigma.shape
    bk = window_ends(pos, min_len, unit)
    K = len(bk)
    rem = _remaining(rho, pos, unit)
    reach = np.where(bk >= 0, bk - np.arange(S)[None, :], -1)                  # [K][S]
    tr = np.zeros((I, S, K))
    ln = np.zeros((I, S, K))
    W = np.ones((I, S))                                                        # W(a, a + w)
    for w in range(int(reach.max()) + 1):
        if w:
            W[:, :S - w] *= rho[:, w:]
            W[:, S - w:] = 0.0
        for k in range(K):
            a = np.flatnonzero(reach[k] == w)
            if len(a):
                b = a + w
                t = sigma[:, a] * W[:, a]
                tr[:, a, k] = t
                ln[:, a, k] = t * (_window_len(pos, a, b, unit)[None, :] + rem[:, b])
    return tr, ln


def terms_b(eprob, pos, F, alpha, min_len, unit):
    """Yardstick B: the same in np.longdouble from ln rho, returned as float64."""
    ld = np.longdouble
    sigma, lrho = cells_b(eprob, pos, F, alpha)
    I, S = sigma.shape
    blocked = np.isneginf(lrho)
    with np.errstate(over="ignore"):
        rho = np.where(blocked, ld(0), np.exp(np.where(blocked, ld(0), lrho)))
    rem = _remaining(rho, pos, unit)
    Q = np.zeros((I, S), dtype=ld)
    q = np.zeros(I, dtype=ld)
    for s in range(S):
        q = np.where(blocked[:, s], ld(0), q + np.where(blocked[:, s], ld(0), lrho[:, s]))
        Q[:, s] = q
    n = np.cumsum(blocked, axis=1)
    bk = window_ends(pos, min_len, unit)
    K = len(bk)
    tr = np.zeros((I, S, K))
    ln = np.zeros((I, S, K))
    for k in range(K):
        a = np.flatnonzero(bk[k] >= 0)
        b = bk[k, a]
        W = np.where(n[:, b] == n[:, a], np.exp(Q[:, b] - Q[:, a]), ld(0))
        t = sigma[:, a].astype(ld) * W
        tr[:, a, k] = t.astype(np.float64)
        ln[:, a, k] = (t * (_window_len(pos, a, b, unit).astype(ld)[None, :] + rem[:, b])).astype(np.float64)
    return tr, ln


def region_records(terms, regions):
    """[I][R][K] of DTYPE: the terms added over the start sites of every region [begin, end)."""
    tr, ln = terms
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((tr.shape[0], len(reg), tr.shape[2]), dtype=DTYPE)
    for r, (a, b) in enumerate(reg):
        out["tracts"][:, r] = tr[:, a:b].sum(axis=1)
        out["length"][:, r] = ln[:, a:b].sum(axis=1)
    return out


def path_by_length(paths, pos, min_len, unit):
    """The statistics of given 0/1 paths [..][S]: (tracts, length), each [..][K]: the number of
    tracts (runs of 1 cut at chromosome starts) of length >= L_k and their total length, in sites
    or in Mb (first site to last: the distances of a tract's sites but the first)."""
    z = np.asarray(paths).astype(bool)
    shape, S = z.shape[:-1], z.shape[-1]
    z = z.reshape(-1, S)
    N = len(z)
    pos = np.asarray(pos, dtype=np.float64)
    cs = xu.chrom_start(pos)
    d = np.where(np.isinf(pos), 0.0, pos)
    L = np.atleast_1d(np.asarray(min_len, dtype=np.float64))
    tr = np.zeros((N, len(L)))
    ln = np.zeros((N, len(L)))
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
        for k, l in enumerate(L):
            sel = (sites > 0) & (lens >= l)
            tr[lo:lo + n, k] = sel.sum(axis=1)
            ln[lo:lo + n, k] = (lens * sel).sum(axis=1)
    return tr.reshape(shape + (len(L),)), ln.reshape(shape + (len(L),))


def enumerate_by_length(eprob, pos, F, alpha, min_len, unit):
    """Brute force over all 2^S paths (S <= 12): (tracts, length), each [I][K] = E[. | y] of
    path_by_length's statistics under the path probabilities."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    c = su.coancestry(alpha, pos)
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1
    e = np.exp(eprob)
    st_tr, st_ln = path_by_length(z.astype(np.uint8), pos, min_len, unit)     # [paths][K]
    tr = np.empty((I, st_tr.shape[1]))
    ln = np.empty((I, st_tr.shape[1]))
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        p = p / p.sum()
        tr[i] = p @ st_tr
        ln[i] = p @ st_ln
    return tr, ln


def spread(a, b):
    """Largest |A - B| per field of two record arrays."""
    return {f: float(np.max(np.abs(a[f] - b[f]))) if a[f].size else 0.0 for f in FIELDS}


def sampler_check(tr, ln, exact, tag=""):
    """The condition of the tests against the sampler, on tr, ln [R][I][K] (path_by_length of R
    draws) and the exact records of the whole data [I][K]: per threshold and statistic the cohort
    total of the draw means within 5 standard errors of the exact total, the same per individual
    whose draws vary, and at most 5 of 20 individuals without variance.  Returns the largest |z|."""
    R = tr.shape[0]
    worst = 0.0
    for name, x_all in (("tracts", tr), ("length", ln)):
        for k in range(x_all.shape[2]):
            x = x_all[:, :, k]
            want = exact[name][:, k]
            tot = x.sum(axis=1)
            se = tot.std(ddof=1) / np.sqrt(R)
            z = abs(tot.mean() - want.sum()) / se
            assert z <= 5, (tag, name, k, "cohort", z)
            sd = x.std(axis=0, ddof=1)
            vary = sd > 0
            assert (~vary).sum() <= 5, (tag, name, k, int((~vary).sum()))
            zi = np.abs(x.mean(axis=0) - want)[vary] / (sd[vary] / np.sqrt(R))
            assert (zi <= 5).all(), (tag, name, k, zi.max())
            worst = max(worst, z, zi.max())
    return worst


# The spread of the two yardsticks on support_util.gpu_cohort, largest |A - B| per unit and field
# over all the region sets of expect_util.region_sets(5003, pos, 80) and the thresholds COHORT_LEN,
# as tests/test_bylength_cpu.py measures and prints it (float64 running products against
# longdouble prefix sums).  See there for how to re-measure.  The largest figures belong to the
# whole data (sums of 5003 terms); nothing here is taken from a device.
SPREAD = {"sites": {"tracts": 9.293e-14, "length": 9.663e-11},
          "mb": {"tracts": 9.281e-14, "length": 9.649e-12}}
# 16 x the spread, support_util's rule and margin: the device groups and rescales its products
# unlike either restatement.
TOL = {u: {f: 16 * v for f, v in s.items()} for u, s in SPREAD.items()}
