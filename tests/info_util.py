"""The yardstick of the observed-information tests (nghmm_obs_info, include/nghmm.h).

ref_info: an independent 50-digit evaluation with mpmath, written from the definition -- a plain
forward recursion for l_i(F, alpha) = log(q prod_s M_s 1), M_s = (c_s I + (1 - c_s) 1 q^T) diag(e_s),
c_s = exp(-alpha d_s) (0 at a chromosome start), q = (1 - F, F), NO jets; its derivatives are
mpmath.diff of orders (1,0), (0,1), (2,0), (1,1), (0,2).  (mpf has an unbounded exponent: the
recursion needs no rescaling.)

jet_info_np: the device's recursion restated in binary64 numpy -- the forward ROW VECTOR v = q
prod M with its five derivative companions, advanced by the product rule with the closed-form
derivatives of a site operator, rescaled every 8 sites by the exponent of the value component,
closed as l = log Z, g = Z_x / Z, h_xy = Z_xy / Z - g_x g_y.  tests/test_info_cpu.py holds the
two to each other, which guards the reference and the algebra against each other.

Tolerances of a record against the reference (check_records), from the project's per-call contract
of 1e-9 relative for fast against exact mode and 1e-12 for log-likelihoods:
  lkl       |l - L| <= 1e-12 |L|
  gradient  |g_k - G_k| <= 1e-9 (|G_k| + |H_kk| x_k)   (what a 1e-9 relative shift of x_k causes)
  Hessian   |h_kl - H_kl| <= 1e-9 max(|H_kl|, sqrt(|H_kk H_ll|))
`scale` multiplies all three bounds (the CPU test demands 1e-3 of the gradient and Hessian
bounds of the binary64 restatement)."""
import numpy as np

FIELDS = ("lkl", "g_F", "g_A", "h_FF", "h_FA", "h_AA")
INFO_DTYPE = np.dtype([(f, np.float64) for f in FIELDS])
POINTS = ((0.1, 0.5), (0.02, 3.0), (0.6, 0.01))


def ref_info(le, pos, F, alpha, dps=50):
    """One individual: le [S][2] log emissions, pos [S] distances (inf: a chromosome start),
    the point (F, alpha) -> the six fields as floats, evaluated with `dps` digits."""
    import mpmath as mp
    with mp.workdps(dps):
        e0 = [mp.exp(mp.mpf(float(x))) for x in le[:, 0]]
        e1 = [mp.exp(mp.mpf(float(x))) for x in le[:, 1]]
        d = [None if np.isinf(x) else mp.mpf(float(x)) for x in pos]
        S = len(d)

        def ell(f, a):
            q0, q1 = 1 - f, f
            v0, v1 = q0, q1
            for s in range(S):
                if d[s] is None:
                    t = v0 + v1
                    v0, v1 = t * q0 * e0[s], t * q1 * e1[s]
                else:
                    c = mp.exp(-a * d[s])
                    t = (1 - c) * (v0 + v1)
                    v0, v1 = (c * v0 + t * q0) * e0[s], (c * v1 + t * q1) * e1[s]
            return mp.log(v0 + v1)

        x = (mp.mpf(float(F)), mp.mpf(float(alpha)))
        out = [ell(*x)] + [mp.diff(ell, x, n) for n in ((1, 0), (0, 1), (2, 0), (1, 1), (0, 2))]
        return tuple(float(v) for v in out)


def ref_records(le, pos, F, alpha, dps=50):
    """ref_info for every individual: le [I][S][2], F / alpha [I] -> structured array [I]."""
    I = le.shape[0]
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    A = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    out = np.zeros(I, dtype=INFO_DTYPE)
    for i in range(I):
        out[i] = ref_info(le[i], pos, F[i], A[i], dps)
    return out


def jet_info_np(le, pos, F, alpha, renorm=8):
    """The jet recursion in binary64, vectorised over individuals: le [I][S][2], F / alpha [I]."""
    le = np.asarray(le, dtype=np.float64)
    I, S, _ = le.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,)).copy()
    A = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)).copy()
    q = np.stack([1 - F, F], axis=1)
    dq = np.stack([-np.ones(I), np.ones(I)], axis=1)
    z = np.zeros((I, 2))
    v, vF, vA, vFF, vFA, vAA = q.copy(), dq.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    base = np.zeros(I)
    ex = np.zeros(I)
    for s in range(S):
        base += le[:, s, 0]
        e = np.stack([np.ones(I), np.exp(le[:, s, 1] - le[:, s, 0])], axis=1)
        if np.isinf(pos[s]):
            c = c1 = c2 = np.zeros(I)
        else:
            c = np.exp(-A * pos[s])
            c1 = -pos[s] * c
            c2 = pos[s] * pos[s] * c
        a = np.ones(I) if np.isinf(pos[s]) else -np.expm1(-A * pos[s])

        def app(x, gamma, beta):          # x (gamma I + 1 beta^T) diag(e)
            return (gamma[:, None] * x + x.sum(axis=1)[:, None] * beta) * e

        def anti(x, k):                   # k x (I - 1 q^T) diag(e), from the small terms:
            w = x[:, 1] * q[:, 0] - x[:, 0] * q[:, 1]   # x (I - 1 q^T) = w (-1, +1)
            return (k * w)[:, None] * dq * e

        zero = np.zeros(I)
        M = (c, a[:, None] * q)
        MF = (zero, a[:, None] * dq)
        MFA = (zero, -c1[:, None] * dq)
        nv = app(v, *M)
        nF = app(vF, *M) + app(v, *MF)
        nA = app(vA, *M) + anti(v, c1)
        nFF = app(vFF, *M) + 2 * app(vF, *MF)
        nFA = app(vFA, *M) + anti(vF, c1) + app(vA, *MF) + app(v, *MFA)
        nAA = app(vAA, *M) + 2 * anti(vA, c1) + anti(v, c2)
        v, vF, vA, vFF, vFA, vAA = nv, nF, nA, nFF, nFA, nAA
        if s % renorm == renorm - 1 or s == S - 1:
            _, k = np.frexp(v.max(axis=1))
            sc = np.ldexp(1.0, -k)[:, None]
            v, vF, vA, vFF, vFA, vAA = v * sc, vF * sc, vA * sc, vFF * sc, vFA * sc, vAA * sc
            ex += k
    Z, ZF, ZA, ZFF, ZFA, ZAA = (x.sum(axis=1) for x in (v, vF, vA, vFF, vFA, vAA))
    out = np.zeros(I, dtype=INFO_DTYPE)
    out["lkl"] = base + (np.log(Z) + ex * np.log(2.0))
    out["g_F"], out["g_A"] = ZF / Z, ZA / Z
    out["h_FF"] = ZFF / Z - out["g_F"] ** 2
    out["h_FA"] = ZFA / Z - out["g_F"] * out["g_A"]
    out["h_AA"] = ZAA / Z - out["g_A"] ** 2
    return out


def bounds(ref, F, alpha):
    """The absolute bound of every field of every record (see the module's docstring)."""
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), ref.shape)
    A = np.broadcast_to(np.asarray(alpha, dtype=np.float64), ref.shape)
    b = np.zeros(ref.shape, dtype=INFO_DTYPE)
    b["lkl"] = 1e-12 * np.abs(ref["lkl"])
    b["g_F"] = 1e-9 * (np.abs(ref["g_F"]) + np.abs(ref["h_FF"]) * F)
    b["g_A"] = 1e-9 * (np.abs(ref["g_A"]) + np.abs(ref["h_AA"]) * A)
    gm = np.sqrt(np.abs(ref["h_FF"] * ref["h_AA"]))
    b["h_FF"] = 1e-9 * np.abs(ref["h_FF"])
    b["h_AA"] = 1e-9 * np.abs(ref["h_AA"])
    b["h_FA"] = 1e-9 * np.maximum(np.abs(ref["h_FA"]), gm)
    return b


def worst_ratios(got, ref, F, alpha):
    """{field: largest |got - ref| / bound over the records}."""
    b = bounds(ref, F, alpha)
    return {f: float(np.max(np.abs(got[f] - ref[f]) / b[f])) for f in FIELDS}


def check_records(got, ref, F, alpha, scale=None, label=""):
    """Every field of every record within scale[field] (default 1) of its bound; prints the worst
    ratio per field first."""
    w = worst_ratios(got, ref, F, alpha)
    print(f"\n  {label}: worst |error| / bound per field: " + ", ".join(f"{f} {w[f]:.3g}" for f in FIELDS))
    b = bounds(ref, F, alpha)
    for f in FIELDS:
        sc = 1.0 if scale is None else scale[f]
        err = np.abs(got[f] - ref[f])
        bad = np.flatnonzero(~(err <= sc * b[f]))
        assert bad.size == 0, (label, f, int(bad[0]), float(got[f][bad[0]]), float(ref[f][bad[0]]),
                               float(b[f][bad[0]]) * sc)
    return w


def random_case(seed, n_ind, n_sites, n_chrom=3):
    """Random log emissions [I][S][2], distances with n_chrom chromosomes."""
    rng = np.random.default_rng(seed)
    e0 = rng.uniform(0.05, 1.0, (n_ind, n_sites))
    e1 = e0 * np.exp(rng.normal(0.0, 0.7, (n_ind, n_sites)))
    pos = rng.uniform(0.001, 0.5, n_sites)
    pos[0] = np.inf
    for k in range(1, n_chrom):
        pos[n_sites * k // n_chrom] = np.inf
    return np.log(np.stack([e0, e1], axis=-1)), pos
