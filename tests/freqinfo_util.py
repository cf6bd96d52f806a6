"""The yardstick of the per-site frequency-likelihood tests (nghmm_freq_info, include/nghmm.h), in
numpy, twice:

(A) scaled linear-space forward-backward in float64, vectorised over the individuals: both
    vectors divided by their sum after every site;
(B) log space in np.longdouble.

Both form the cavity weights (1 - c, c) of every cell from the forward PREDICTION of the site (the
forward vector of the site before, pushed through the site's transition, the site's own emission
not applied) times the backward vector, each weight from its own product; then per site the sums
over the individuals of ln bracket, u, u^2 - (1 - c) e0'' / bracket and ln(bracket at a level /
bracket), bracket = (1 - c) e0(f) + c e1(f).  Both carry exact zeros: a bracket that is 0 has the
logarithm -inf, and a chromosome's first site restarts both recursions, so that an individual
whose data one chromosome excludes (likelihood 0 there) is well defined on the others.
tests/test_freqinfo_cpu.py checks both against enumeration and whole-chain likelihoods before
tests/test_gpu_freqinfo.py uses B.

Every function takes LINEAR likelihoods p [S][I][3], distances pos [S] (+inf: a chromosome start),
F and alpha [I], freq [S], levels [K], and returns a dict of float64 arrays:
    w0, cavity [I][S]       the two weights (1 - c) and c
    ll, score, info [S]     nghmm_freq_stat's fields
    curve [S][K]
    abs_ll, abs_score, abs_info [S], abs_curve [S][K]   the sum of the absolute values of the terms
                            of the entry (info: |u^2| + |(1 - c) e0'' / bracket| per individual)
"""
import numpy as np

FIELDS = ("cavity", "ll", "score", "info", "curve")


def _site_part(w0, w1, p, freq, levels, dt):
    """The sums over the individuals; w0, w1 [S][I] in dtype dt."""
    p = np.asarray(p).astype(dt)
    f = np.asarray(freq, dtype=np.float64).astype(dt)[:, None]
    p0, p1, p2 = p[..., 0], p[..., 1], p[..., 2]

    def bracket(x):
        om = 1 - x
        return w0 * (p0 * om * om + 2 * p1 * x * om + p2 * x * x) + w1 * (p0 * om + p2 * x)

    om = 1 - f
    with np.errstate(divide="ignore", invalid="ignore"):
        B = bracket(f)
        d0 = -2 * p0 * om + 2 * p1 * (om - f) + 2 * p2 * f
        d1 = p2 - p0
        dd0 = 2 * p0 - 4 * p1 + 2 * p2
        u = (w0 * d0 + w1 * d1) / B
        t_ll = np.log(B)
        t_a, t_b = u * u, w0 * dd0 / B
        out = {"ll": t_ll.sum(axis=1), "score": u.sum(axis=1), "info": (t_a - t_b).sum(axis=1),
               "abs_ll": np.abs(t_ll).sum(axis=1), "abs_score": np.abs(u).sum(axis=1),
               "abs_info": (np.abs(t_a) + np.abs(t_b)).sum(axis=1)}
        K = len(levels)
        curve = np.zeros((p.shape[0], K), dtype=dt)
        acurve = np.zeros((p.shape[0], K), dtype=dt)
        for k, x in enumerate(levels):
            t = np.log(bracket(dt(x)) / B)
            curve[:, k] = t.sum(axis=1)
            acurve[:, k] = np.abs(t).sum(axis=1)
    dead = np.isneginf(out["ll"])
    for name in ("score", "info"):
        out[name] = np.where(dead, np.nan, out[name])
    curve[dead] = np.nan
    out["curve"], out["abs_curve"] = curve, acurve
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def _emissions(p, freq, dt):
    p = np.asarray(p).astype(dt)
    f = np.asarray(freq, dtype=np.float64).astype(dt)[:, None]
    om = 1 - f
    e0 = p[..., 0] * om * om + 2 * p[..., 1] * f * om + p[..., 2] * f * f
    e1 = p[..., 0] * om + p[..., 2] * f
    return np.stack([e0, e1], axis=2)                                   # [S][I][2]


def _coancestry(alpha, pos, dt):
    pos = np.asarray(pos, dtype=np.float64)
    start = np.isinf(pos)
    d = np.where(start, 0.0, pos).astype(dt)
    c = np.exp(-np.asarray(alpha, dtype=np.float64).astype(dt)[None, :] * d[:, None])   # [S][I]
    c[start] = 0
    return c


def freq_info_a(p, pos, F, alpha, freq, levels=()):
    """Yardstick A: float64, linear space, both vectors rescaled to sum 1 after every site."""
    dt = np.float64
    p = np.asarray(p, dtype=dt)
    S, I, _ = p.shape
    F = np.broadcast_to(np.asarray(F, dtype=dt), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=dt), (I,))
    q = np.stack([1 - F, F], axis=1)                                    # [I][2]
    e = _emissions(p, freq, dt)
    c = _coancestry(alpha, pos, dt)
    start = np.isinf(np.asarray(pos, dtype=np.float64))
    pred = np.empty((S, I, 2))
    v = q.copy()
    for s in range(S):
        cs = c[s][:, None]
        # (a chromosome's first site: the prediction is q whatever came before, also after an
        # individual whose data the chromosome before excludes)
        pr = q if start[s] else cs * v + (1 - cs) * q * v.sum(axis=1, keepdims=True)
        pred[s] = pr
        v = pr * e[s]
        with np.errstate(invalid="ignore"):
            v = v / v.sum(axis=1, keepdims=True)
    x = np.empty((S, I, 2))
    w = np.ones((I, 2))
    for s in range(S - 1, -1, -1):
        x[s] = pred[s] * w
        cs = c[s][:, None]
        uu = e[s] * w
        w = cs * uu + (1 - cs) * (q * uu).sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            w = np.ones((I, 2)) if start[s] else w / w.sum(axis=1, keepdims=True)
    tot = x.sum(axis=2)
    w0, w1 = x[..., 0] / tot, x[..., 1] / tot
    out = _site_part(w0, w1, p, freq, levels, dt)
    out["w0"], out["cavity"] = np.ascontiguousarray(w0.T), np.ascontiguousarray(w1.T)
    return out


def freq_info_b(p, pos, F, alpha, freq, levels=()):
    """Yardstick B: log space, np.longdouble."""
    ld = np.longdouble
    p = np.asarray(p).astype(ld)
    S, I, _ = p.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,)).astype(ld)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)).astype(ld)
    q = np.stack([1 - F, F], axis=1)
    c = _coancestry(alpha, pos, ld)
    with np.errstate(divide="ignore"):
        le = np.log(_emissions(p, freq, ld))
        lq = np.log(q)
        loff = np.log((1 - c)[..., None] * q[None, :, :])               # ln T_s(j, k), j != k
        ldiag = np.log((1 - c)[..., None] * q[None, :, :] + c[..., None])
    start = np.isinf(np.asarray(pos, dtype=np.float64))
    lpred = np.empty((S, I, 2), dtype=ld)
    lx = np.empty((S, I, 2), dtype=ld)
    with np.errstate(invalid="ignore"):
        v = lq
        for s in range(S):
            # (a chromosome's first site: the prediction is q whatever came before)
            lpred[s] = lq if start[s] else np.logaddexp(v + ldiag[s], v[:, ::-1] + loff[s])
            v = lpred[s] + le[s]
            v = v - v.max(axis=1, keepdims=True)
        w = np.zeros((I, 2), dtype=ld)
        for s in range(S - 1, -1, -1):
            lx[s] = lpred[s] + w
            u = le[s] + w
            w = np.logaddexp(ldiag[s] + u, loff[s][:, ::-1] + u[:, ::-1])
            w = np.zeros((I, 2), dtype=ld) if start[s] else w - w.max(axis=1, keepdims=True)
        lz = np.logaddexp(lx[..., 0], lx[..., 1])
        w0, w1 = np.exp(lx[..., 0] - lz), np.exp(lx[..., 1] - lz)
    out = _site_part(w0, w1, p, freq, levels, ld)
    out["w0"] = np.ascontiguousarray(w0.T).astype(np.float64)
    out["cavity"] = np.ascontiguousarray(w1.T).astype(np.float64)
    return out


def spread(got, want):
    """Per field the largest |got - want| over the entry's scale: for the cavity c itself (the
    call returns c, so relative to c is what a double of it can hold at either end; the precision
    of 1 - c shows in the sums, which use that weight); for the sums the sum of the absolute values
    of the entry's terms (want's).  Every entry of `want` must be finite."""
    out = {"cavity": float(np.max(np.abs(got["cavity"] - want["cavity"]) / want["cavity"]))}
    for f in ("ll", "score", "info", "curve"):
        if np.asarray(got[f]).size:
            out[f] = float(np.max(np.abs(got[f] - want[f]) / want["abs_" + f]))
    return out


def gpu_cohort(pkg):
    """The cohort of tests/test_gpu_freqinfo.py, shared with the yardstick-spread measurement of
    tests/test_freqinfo_cpu.py: support_util.gpu_cohort's recipe with I = 70 -- 70 x 5003 (two
    blocks of individuals in the site reduce, the second one ragged; the sites ragged against every
    block size), three chromosomes, missing cells, random indF, alpha = 1e-3 for the first five
    individuals and random for the rest -- with freq = "r" data, evaluated at a frequency vector
    that is NOT the truth, 0.8 truth + 0.05, so that the scores are far from 0.
    Returns (simulated data, normalised log likelihoods, indF, alpha, freq [S])."""
    I, S = 70, 5003
    d = pkg.simulate.simulate(I, S, seed=41, n_chrom=3, indF="r", alpha="r", freq="r", missing_rate=0.03)
    rng = np.random.default_rng(42)
    F, A = rng.uniform(0.02, 0.95, I), rng.uniform(0.01, 2.0, I)
    A[:5] = 1e-3
    F[:5] = rng.uniform(0.3, 0.9, 5)
    return d, pkg.simulate.normalise_log_gl(d.gl), F, A, 0.8 * d.freq + 0.05


# eight levels, 0 and 1 among them
LEVELS = (0.0, 0.01, 0.05, 0.2, 0.5, 0.8, 0.95, 1.0)

# The spread of the two yardsticks on gpu_cohort at LEVELS, per field, in the measure of spread():
# as tests/test_freqinfo_cpu.py measures and prints it (float64 scaled linear space against
# longdouble log space).  The GPU tolerance is 16 x these, the margin tests/test_gpu_support.py
# gives two correct restatements: the device rescales and orders its products unlike either.
SPREAD = {"cavity": 2.46e-12, "ll": 3.95e-15, "score": 2.13e-15, "info": 5.61e-15, "curve": 7.08e-12}
TOL = {k: 16 * v for k, v in SPREAD.items()}
