"""The yardstick of the tract-bounds tests (nghmm_tract_bounds, include/nghmm.h), in numpy, twice:

(A) float64 on sample_util.forward_filter with the conditional
        c_t = P(z_t = 1 | z_{t+1} = 1, y_1..t)        (support_util.support_a's factor):
        ln G(s) = sum_{t = s..c-1} ln c_t,
        ln H(s) = ln P(z_s = 1 | y) + sum_{t = c..s-1} ln c_t - ln P(z_c = 1 | y);
(B) np.longdouble log space with g_t = T_t(1,1) e_t(1) beta_t(1) / beta_{t-1}(1)
        (support_util.support_b's vectors):
        ln H(s) = sum_{t = c+1..s} ln g_t,
        ln G(s) = ln P(z_s = 1 | y) + sum_{t = s+1..c} ln g_t - ln P(z_c = 1 | y).

Both carry exact zeros (-inf; 0/0 counts as 0) and form P(z_s = 0 | y) directly.  Anchors, limits
and quantile sites are made of either form by the same code below.  tests/test_bounds_cpu.py checks
both against enumeration before tests/test_gpu_bounds.py uses B."""
import numpy as np

import sample_util as su
import support_util as sup

NO_ANCHOR = 2 ** 64 - 1
LEVELS = (0.975, 0.5, 0.025)
# three logged quantities enter a reach (support_util.LOG_TOL: 16 x the yardsticks' spread)
TIE = 3 * sup.LOG_TOL


def _fix(x):
    return np.where(np.isnan(x), -np.inf, x)


class FormA:
    def __init__(self, eprob, pos, F, alpha):
        eprob = np.asarray(eprob, dtype=np.float64)
        I = eprob.shape[0]
        F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
        alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
        f = su.forward_filter(eprob, pos, F, alpha)
        post = sup.posterior2(f, eprob, pos, F, alpha)
        nxt = np.r_[np.asarray(pos, dtype=np.float64)[1:], np.inf]
        c = su.coancestry(alpha, nxt)
        q1 = F[:, None]
        num = f[..., 1] * ((1 - c) * q1 + c)
        den = num + f[..., 0] * (1 - c) * q1
        with np.errstate(invalid="ignore", divide="ignore"):
            self.lcond = sup._log0(num / den)          # [I][S]
        self.p0 = np.where(np.isnan(post[..., 0]), 1.0, post[..., 0])
        self.lp1 = sup._log0(post[..., 1])
        self.p1 = np.where(np.isnan(post[..., 1]), 0.0, post[..., 1])

    def ln_g(self, i, lo, c):
        """ln G(s), s = lo..c"""
        t = self.lcond[i, lo:c]
        return np.r_[np.cumsum(t[::-1])[::-1], 0.0]

    def ln_h(self, i, c, hi):
        """ln H(s), s = c..hi"""
        t = np.r_[0.0, np.cumsum(self.lcond[i, c:hi])]
        with np.errstate(invalid="ignore"):
            return _fix(self.lp1[i, c:hi + 1] + t - self.lp1[i, c])


class FormB:
    def __init__(self, eprob, pos, F, alpha):
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
            loff = np.log((1 - c)[..., None] * q[:, None, :])
            ldiag = np.log((1 - c)[..., None] * q[:, None, :] + c[..., None])
        lf = np.empty((I, S, 2), dtype=ld)
        lb = np.empty((I, S, 2), dtype=ld)
        with np.errstate(invalid="ignore"):
            v = lq
            for s in range(S):
                v = np.logaddexp(v + ldiag[:, s], v[:, ::-1] + loff[:, s]) + eprob[:, s]
                lf[:, s] = v
            w = np.zeros((I, 2), dtype=ld)
            for s in range(S - 1, -1, -1):
                lb[:, s] = w
                u = eprob[:, s] + w
                w = np.logaddexp(ldiag[:, s] + u, loff[:, s, ::-1] + u[:, ::-1])
            lz = np.logaddexp(lf[:, -1, 0], lf[:, -1, 1])
            lpost = lf + lb - lz[:, None, None]
            lpost = np.where(np.isnan(lpost), np.array([0.0, -np.inf], dtype=ld), lpost)
            lg = np.full((I, S), -np.inf, dtype=ld)      # (site 0 has no factor)
            lg[:, 1:] = _fix(ldiag[:, 1:, 1] + eprob[:, 1:, 1] + lb[:, 1:, 1] - lb[:, :-1, 1])
        self.lg = lg
        self.lp1 = lpost[..., 1]
        self.p0 = np.exp(lpost[..., 0]).astype(np.float64)
        self.p1 = np.exp(lpost[..., 1]).astype(np.float64)

    def ln_g(self, i, lo, c):
        t = self.lg[i, lo + 1:c + 1]
        suf = np.r_[np.cumsum(t[::-1])[::-1], np.longdouble(0)]
        with np.errstate(invalid="ignore"):
            return _fix(self.lp1[i, lo:c + 1] + suf - self.lp1[i, c]).astype(np.float64)

    def ln_h(self, i, c, hi):
        return np.r_[np.longdouble(0), np.cumsum(self.lg[i, c + 1:hi + 1])].astype(np.float64)


def chrom_edges(pos):
    """(first site, last site) of every site's chromosome"""
    pos = np.asarray(pos, dtype=np.float64)
    S = len(pos)
    st = np.flatnonzero(np.isinf(pos) | (np.arange(S) == 0))
    idx = np.searchsorted(st, np.arange(S), side="right") - 1
    first = st[idx]
    last = np.r_[st[1:], S][idx] - 1
    return first, last


def start_of(ln_g, lo, level):
    bad = np.flatnonzero(ln_g < np.log(level))
    return lo + (int(bad[-1]) + 1 if len(bad) else 0)


def end_of(ln_h, c, level):
    bad = np.flatnonzero(ln_h < np.log(level))
    return c + (int(bad[0]) - 1 if len(bad) else len(ln_h) - 1)


def bounds_ref(model, pos, tracts, anchors=None, levels=LEVELS):
    """The whole result of nghmm_tract_bounds from a FormA / FormB: a dict of arrays, with the
    curves ln G / ln H of every record (for answers at other levels) and, for auto anchors, the
    smallest P(z = 0 | y) of the core at any other site (runner_up)."""
    ind, a, b = sup.as_ranges(tracts)
    n, m = len(ind), len(levels)
    first, last = chrom_edges(pos)
    anc = np.empty(n, dtype=np.int64)
    runner = np.full(n, np.inf)
    for k in range(n):
        if anchors is not None and int(anchors[k]) != NO_ANCHOR:
            anc[k] = int(anchors[k])
        else:
            p0 = model.p0[ind[k], a[k]:b[k] + 1]
            j = int(np.argmin(p0))
            anc[k] = a[k] + j
            rest = np.delete(p0, j)
            runner[k] = rest.min() if len(rest) else np.inf
    out = {"anchor": anc, "runner_up": runner,
           "left_limit": first[anc].copy(), "right_limit": last[anc].copy(),
           "post_anchor": model.p1[ind, anc],
           "log_reach_left": np.zeros(n), "log_reach_right": np.zeros(n),
           "start": np.empty((n, m), dtype=np.int64), "end": np.empty((n, m), dtype=np.int64),
           "ln_g": [], "ln_h": []}
    for k in range(n):
        if k > 0 and ind[k - 1] == ind[k]:
            out["left_limit"][k] = max(out["left_limit"][k], anc[k - 1])
        if k + 1 < n and ind[k + 1] == ind[k]:
            out["right_limit"][k] = min(out["right_limit"][k], anc[k + 1])
    for k in range(n):
        i, c, lo, hi = ind[k], anc[k], out["left_limit"][k], out["right_limit"][k]
        if not out["post_anchor"][k] > 0:
            g, h = np.full(c - lo + 1, -np.inf), np.full(hi - c + 1, -np.inf)
            out["start"][k], out["end"][k] = c, c
        else:
            g, h = model.ln_g(i, lo, c), model.ln_h(i, c, hi)
            for j, p in enumerate(levels):
                out["start"][k, j] = start_of(g, lo, p)
                out["end"][k, j] = end_of(h, c, p)
        out["log_reach_left"][k], out["log_reach_right"][k] = g[0], h[-1]
        out["ln_g"].append(g)
        out["ln_h"].append(h)
    return out


def enumerate_curves(eprob, pos, F, alpha, i, c):
    """Brute force over all 2^S paths (S <= 12): ln G(s), s = 0..c and ln H(s), s = c..S-1 of
    individual i and anchor c, not cut at chromosome edges; and P(z_s = 0 | y) [S]."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    assert S <= 12
    Fi = float(np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))[i])
    ai = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))[i:i + 1]
    eprob = eprob[i:i + 1]
    cc = su.coancestry(ai, pos)[0]
    z = (np.arange(2 ** S)[:, None] >> np.arange(S)[None, :]) & 1
    e = np.exp(eprob[0])
    q = np.array([1 - Fi, Fi])
    p = q[z[:, 0]] * e[0, z[:, 0]]
    for s in range(1, S):
        T = (1 - cc[s]) * q[z[:, s]] + np.where(z[:, s - 1] == z[:, s], cc[s], 0.0)
        p = p * T * e[s, z[:, s]]
    Z = p.sum()
    pc = p[z[:, c] == 1].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.array([np.log(p[z[:, s:c + 1].all(axis=1)].sum() / pc) for s in range(c + 1)])
        h = np.array([np.log(p[z[:, c:s + 1].all(axis=1)].sum() / pc) for s in range(c, S)])
    p0 = np.array([p[z[:, s] == 0].sum() / Z for s in range(S)])
    return _fix(g), _fix(h), p0


def compare(a, b):
    """Two bounds_ref results of the same records: sites that differ (count, of), and the largest
    difference of the reach logarithms and of post_anchor where both are finite."""
    diff = int((a["start"] != b["start"]).sum() + (a["end"] != b["end"]).sum())
    worst = 0.0
    for f in ("log_reach_left", "log_reach_right"):
        fin = np.isfinite(a[f]) & np.isfinite(b[f])
        assert np.array_equal(np.isfinite(a[f]), np.isfinite(b[f]))
        if fin.any():
            worst = max(worst, float(np.max(np.abs(a[f][fin] - b[f][fin]))))
    post = float(np.max(np.abs(a["post_anchor"] - b["post_anchor"]))) if len(a["anchor"]) else 0.0
    return {"sites_differ": diff, "sites": 2 * a["start"].size, "log_reach": worst, "post_anchor": post,
            "anchors_differ": int((a["anchor"] != b["anchor"]).sum())}
