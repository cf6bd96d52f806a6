"""The yardstick of the tract-support tests (nghmm_tract_support, include/nghmm.h), in numpy,
twice:

(A) the conditional-product form in float64 on sample_util.forward_filter,
        P(z_a..b = k | y) = P(z_b = k | y) prod_{s = a..b-1} P(z_s = k | z_{s+1} = k, y_1..s),
    the factor = f_s(k) T_{s+1}(k, k) / sum_j f_s(j) T_{s+1}(j, k) -- what sample_util.cond_probs
    restates for the sampler, here for both states without forming 1 - p;
(B) the direct form f_a(k) prod_{s = a+1..b} T_s(k, k) e_s(k) beta_b(k) / Z in log space in
    np.longdouble.

Both carry exact zeros (an emission that is 0 stays 0, its logarithm -inf): a range with a state
the data exclude is -inf in both, and a 0/0 factor counts as 0.  tests/test_support_cpu.py checks
both against enumeration before tests/test_gpu_support.py uses B.  The device itself uses a third
form (the mirror image of A, with beta)."""
import numpy as np

import sample_util as su
import tracts_util

SCORE_FIELDS = ("log_p_ibd", "log_p_non", "post_min", "post_min_site")


def as_ranges(tracts):
    """(ind, first, last) integer arrays of ibd_tracts' records or of [n][3] (ind, first, n)."""
    t = np.asarray(tracts)
    if t.dtype.names is None:
        t = t.reshape(-1, 3)
        ind, a, n = t[:, 0], t[:, 1], t[:, 2]
    else:
        ind, a, n = t["ind"], t["first_site"], t["n_sites"]
    ind, a, n = (np.asarray(v).astype(np.int64) for v in (ind, a, n))
    return ind, a, a + n - 1


def to_records(ranges):
    """[n][3] (ind, first_site, n_sites) from a list of (ind, first, last), sorted as the call wants."""
    r = sorted((int(i), int(a), int(b)) for i, a, b in ranges)
    return np.array([(i, a, b - a + 1) for i, a, b in r], dtype=np.int64).reshape(-1, 3)


def _log0(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.log(x)
    return np.where(np.isnan(out), -np.inf, out)      # 0/0: a state that is excluded already


def posterior2(a, eprob, pos, F, alpha):
    """sample_util.posterior for both states: P(z_s = k | data) [I][S][2], unsnapped."""
    I, S, _ = a.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    q = np.stack([1 - F, F], axis=1)
    e = np.exp(eprob - eprob.max(axis=2, keepdims=True))
    c = su.coancestry(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)), pos)
    post = np.empty((I, S, 2))
    w = np.ones((I, 2))
    for s in range(S - 1, -1, -1):
        x = a[:, s] * w
        with np.errstate(invalid="ignore", divide="ignore"):
            post[:, s] = x / x.sum(axis=1, keepdims=True)
        cs = c[:, s, None]
        uu = e[:, s] * w
        w = cs * uu + (1 - cs) * (q * uu).sum(axis=1, keepdims=True)
        w = w / w.sum(axis=1, keepdims=True)
    return post


def _scores(n):
    return np.zeros(n, dtype=[("log_p_ibd", np.float64), ("log_p_non", np.float64),
                              ("post_min", np.float64), ("post_min_site", np.uint64),
                              ("runner_up", np.float64)])


def _post_min(out, k, p1, a):
    """post_min, its lowest site, and the smallest posterior at any OTHER site (inf: none)."""
    m = int(np.argmin(p1))                      # the first of equal minima
    out["post_min"][k] = p1[m]
    out["post_min_site"][k] = a + m
    rest = np.delete(p1, m)
    out["runner_up"][k] = rest.min() if len(rest) else np.inf


def support_a(eprob, pos, F, alpha, tracts):
    """Yardstick A.  eprob [I][S][2] log emissions, pos [S] distances (+inf: a chromosome start)."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    f = su.forward_filter(eprob, pos, F, alpha)
    post = posterior2(f, eprob, pos, F, alpha)
    nxt = np.r_[np.asarray(pos, dtype=np.float64)[1:], np.inf]
    c = su.coancestry(alpha, nxt)               # c_{s+1}; 0 at a chromosome start
    q = np.stack([1 - F, F], axis=1)[:, None, :]                       # [I][1][2]
    off = (1 - c)[..., None] * q                                       # T_{s+1}(j, k), j != k
    diag = off + c[..., None]                                          # T_{s+1}(k, k)
    num = f * diag
    den = num + f[..., ::-1] * off
    with np.errstate(invalid="ignore", divide="ignore"):
        lcond = _log0(num / den)                # [I][S][2]: ln P(z_s = k | z_{s+1} = k, y_1..s)
    lpost = _log0(post)
    ind, a, b = as_ranges(tracts)
    out = _scores(len(ind))
    for k, (i, lo, hi) in enumerate(zip(ind, a, b)):
        tot = lpost[i, hi] + lcond[i, lo:hi].sum(axis=0)
        out["log_p_non"][k], out["log_p_ibd"][k] = tot[0], tot[1]
        _post_min(out, k, post[i, lo:hi + 1, 1], lo)
    return out


def support_b(eprob, pos, F, alpha, tracts):
    """Yardstick B: log space, np.longdouble."""
    ld = np.longdouble
    eprob = np.asarray(eprob).astype(ld)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,)).astype(ld)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)).astype(ld)
    pos = np.asarray(pos, dtype=np.float64)
    start = np.isinf(pos)
    d = np.where(start, 0.0, pos).astype(ld)
    c = np.exp(-alpha[:, None] * d[None, :])
    c[:, start] = 0
    q = np.stack([1 - F, F], axis=1)
    with np.errstate(divide="ignore"):
        lq = np.log(q)
        loff = np.log((1 - c)[..., None] * q[:, None, :])               # ln T_s(j, k), j != k
        ldiag = np.log((1 - c)[..., None] * q[:, None, :] + c[..., None])
    lf = np.empty((I, S, 2), dtype=ld)
    lb = np.empty((I, S, 2), dtype=ld)
    with np.errstate(invalid="ignore"):
        v = lq
        for s in range(S):
            stay, move = v + ldiag[:, s], v[:, ::-1] + loff[:, s]
            v = np.logaddexp(stay, move) + eprob[:, s]
            lf[:, s] = v
        w = np.zeros((I, 2), dtype=ld)
        for s in range(S - 1, -1, -1):
            lb[:, s] = w
            u = eprob[:, s] + w
            w = np.logaddexp(ldiag[:, s] + u, loff[:, s, ::-1] + u[:, ::-1])
        lz = np.logaddexp(lf[:, -1, 0], lf[:, -1, 1])
        step = ldiag + eprob                                             # ln T_s(k, k) e_s(k)
        lpost = lf + lb - lz[:, None, None]
        post1 = np.exp(lpost[..., 1]).astype(np.float64)
    ind, a, b = as_ranges(tracts)
    out = _scores(len(ind))
    for k, (i, lo, hi) in enumerate(zip(ind, a, b)):
        with np.errstate(invalid="ignore"):
            tot = lf[i, lo] + step[i, lo + 1:hi + 1].sum(axis=0) + lb[i, hi] - lz[i]
        tot = np.where(np.isnan(tot), -np.inf, tot)
        out["log_p_non"][k], out["log_p_ibd"][k] = float(tot[0]), float(tot[1])
        _post_min(out, k, post1[i, lo:hi + 1], lo)
    return out


def enumerate_support(eprob, pos, F, alpha, tracts):
    """Brute force over all 2^S paths (S <= 12): (log_p_ibd, log_p_non) per range, and the
    per-site posteriors P(z_s = 1 | y) [I][S]."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    c = su.coancestry(alpha, pos)
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1        # [paths][S]
    e = np.exp(eprob)
    prob = np.empty((I, 2 ** S))
    for i in range(I):
        q = np.array([1 - F[i], F[i]])
        p = q[z[:, 0]] * e[i, 0, z[:, 0]]
        for s in range(1, S):
            T = (1 - c[i, s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], c[i, s], 0.0)
            p = p * T * e[i, s, z[:, s]]
        prob[i] = p
    Z = prob.sum(axis=1)
    post = np.stack([(prob[i][:, None] * z).sum(axis=0) / Z[i] for i in range(I)])
    ind, a, b = as_ranges(tracts)
    out = np.empty((len(ind), 2))
    for k, (i, lo, hi) in enumerate(zip(ind, a, b)):
        seg = z[:, lo:hi + 1]
        with np.errstate(divide="ignore"):
            out[k, 0] = np.log(prob[i][seg.all(axis=1)].sum() / Z[i])
            out[k, 1] = np.log(prob[i][~seg.any(axis=1)].sum() / Z[i])
    return out, post


def gpu_cohort(pkg, n_ind=20, n_sites=5003):
    """The cohort of tests/test_gpu_support.py, shared with the yardstick-spread measurement of
    tests/test_support_cpu.py: 20 x 5003 (ragged against every block size), three chromosomes,
    missing cells, random indF; alpha = 1e-3 for the first five individuals (tracts that span many
    lane-chunks), random for the rest; one frequency.  (n_ind, n_sites: the same recipe at another
    size, for tests/test_gpu_layouts.py.)
    Returns (simulated data, normalised log likelihoods, indF, alpha, freq)."""
    I, S = n_ind, n_sites
    d = pkg.simulate.simulate(I, S, seed=41, n_chrom=3, indF="r", alpha="r", missing_rate=0.03)
    rng = np.random.default_rng(42)
    F, A = rng.uniform(0.02, 0.95, I), rng.uniform(0.01, 2.0, I)
    A[:5] = 1e-3
    F[:5] = rng.uniform(0.3, 0.9, 5)
    return d, pkg.simulate.normalise_log_gl(d.gl), F, A, 0.15


def hand_ranges(n_ind, n_sites, pos, lane_sites):
    """Hand-made ranges [(ind, first, last)]: ends on every residue mod 8 and on both sides of
    every lane boundary (multiples of lane_sites, if > 0), the whole data, one-site ranges, a
    range across a chromosome start, two adjacent ranges.  Disjoint within an individual."""
    S = n_sites
    out = [(0, 0, S - 1)]                                                # the whole data
    # individual 1: one-site ranges and ends on every residue mod 8
    s, k = 0, 0
    while s + 40 < min(S, 1500):
        length = 1 if k % 3 == 0 else 9 + (k % 8)
        out.append((1, s, s + length - 1))
        s += length + 1 + (k % 5)
        k += 1
    # individual 2: a range across the first chromosome start, and two adjacent ranges
    cs = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    lo = 0
    if cs:
        out.append((2, cs[0] - 13, cs[0] + 17))
        lo = cs[0] + 18
    out.append((2, lo + 5, lo + 60))
    out.append((2, lo + 61, lo + 130))
    # individuals 3 and 4: both sides of every lane boundary
    if lane_sites:
        bounds = list(range(lane_sites, S, lane_sites))
        for n, t in enumerate(bounds):
            # ends exactly at the boundary's last / first site, and a range across it
            if n % 2 == 0:
                out.append((3, max(t - 5, 0), t - 1))                    # last site in front of it
                if t + 4 < S:
                    out.append((3, t, t + 4))                            # first site behind it
            elif t + 3 < S:
                out.append((4, t - 3, t + 3))                            # across it
        # individual 5: a long range across many lanes, with odd ends
        out.append((5, 3, min(S - 2, 37 * lane_sites + 5)))
    return sorted(set(out))


def cohort_ranges(post, pos, lane_sites):
    """The ranges of the spread measurement: posterior tracts at 0.5 and 0.9 (of the yardstick's
    own posteriors) and the hand-made ranges, as lists of records to score one after the other
    (the tracts of two thresholds overlap)."""
    cs = np.isinf(pos)
    sets = []
    for thr in (0.5, 0.9):
        sets.append(np.array([(i, a, n) for i, a, n, _ in tracts_util.rle_tracts(post >= thr, cs)],
                             dtype=np.int64).reshape(-1, 3))
    sets.append(to_records(hand_ranges(post.shape[0], post.shape[1], pos, lane_sites)))
    return sets


def spread(a, b):
    """Largest |A - B| per field over the ranges (all finite)."""
    return {f: float(np.max(np.abs(a[f] - b[f]))) for f in ("log_p_ibd", "log_p_non", "post_min")}


# The spread of the two yardsticks on gpu_cohort, largest |A - B| per field over the posterior
# tracts at 0.5 and 0.9 and the hand-made ranges, as tests/test_support_cpu.py measures and prints
# it (float64 forward filter against longdouble log space).  It does NOT grow in proportion to the
# length of a range: 4.1e-13 at one site, 4.0e-13 at 1668 sites, 1.0e-12 at 5003 -- it is the error
# of A's forward and backward vectors at the two ends, so the tolerance made of it is flat too.
SPREAD = {"log_p_ibd": 5.3e-13, "log_p_non": 1.03e-12, "post_min": 1.04e-13}
# 16 x the spread; the margin is there because the device rescales and orders its products unlike
# either restatement.  Far inside the project's own bound on posteriors for chains of this
# length: 1e-9 per site of the range for the two logarithms (so 1e-9 for a range of one site),
# 1e-9 for post_min.
LOG_TOL = 16 * max(SPREAD["log_p_ibd"], SPREAD["log_p_non"])
POST_TOL = 16 * SPREAD["post_min"]
