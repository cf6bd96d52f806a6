"""The yardstick of the sampled-path tests (nghmm_sample_paths, include/nghmm.h), in numpy:
Philox4x32-10 twice (vectorised uint64 arithmetic, plain Python ints), the forward filter in
linear space normalised at every site, the sequential backward draw of the header's definition
from the same uniforms, and path statistics by run-length encoding.  tests/test_sample_cpu.py
checks it against enumeration before tests/test_gpu_sample.py uses it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox_py(key, ctr):
    """Philox4x32-10 on Python ints: key (k0, k1), counter (c0, c1, c2, c3) -> four words."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_np(k0, k1, c0, c1, c2, c3):
    """The same on broadcastable arrays (values < 2^32 held in uint64)."""
    k0, k1, c0, c1, c2, c3 = [np.asarray(v, dtype=np.uint64) for v in (k0, k1, c0, c1, c2, c3)]
    m = np.uint64(MASK)
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> sh) ^ c1 ^ k0
        n2 = (p0 >> sh) ^ c3 ^ k1
        c1 = p1 & m
        c3 = p0 & m
        c0, c2 = n0, n2
        k0 = (k0 + np.uint64(W0)) & m
        k1 = (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def uniforms(seed, draws, n_ind, n_sites, site0=0):
    """u [len(draws)][I][S] of the header's definition; site0 = global index of the first site."""
    seed = int(seed) & (2 ** 64 - 1)
    g = np.arange(site0, site0 + n_sites, dtype=np.uint64)
    pair = g >> np.uint64(1)
    d = np.asarray(list(draws), dtype=np.uint64)[:, None, None]
    i = np.arange(n_ind, dtype=np.uint64)[None, :, None]
    x0, x1, x2, x3 = philox_np(seed & MASK, seed >> 32, (pair & np.uint64(MASK))[None, None, :],
                               (pair >> np.uint64(32))[None, None, :], i, d)
    odd = (g & np.uint64(1)).astype(bool)[None, None, :]
    lo = np.where(odd, x2, x0)
    hi = np.where(odd, x3, x1)
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def emissions_np(gl, freq):
    """log emissions [I][S][2] from log likelihoods gl [S][I][3] and freq [S] (calc_emission,
    shared/HMM.cpp:144-154, with calc_HWE at F = 0 and F = 1)."""
    f = np.asarray(freq, dtype=np.float64)[:, None]
    p = np.exp(gl)
    e0 = p[..., 0] * (1 - f) ** 2 + p[..., 1] * 2 * f * (1 - f) + p[..., 2] * f * f
    e1 = p[..., 0] * (1 - f) + p[..., 2] * f
    with np.errstate(divide="ignore"):
        return np.log(np.stack([e0.T, e1.T], axis=-1))


def coancestry(alpha, pos):
    """c [I][S] = exp(-alpha_i d_s), 0 at chromosome starts (d = +inf)."""
    pos = np.asarray(pos, dtype=np.float64)
    d = np.where(np.isinf(pos), 0.0, pos)
    c = np.exp(-np.asarray(alpha, dtype=np.float64)[:, None] * d[None, :])
    c[:, np.isinf(pos)] = 0.0
    return c


def forward_filter(eprob, pos, F, alpha, a_in=None):
    """a [I][S][2], a_s(k) ~ P(z_s = k, y_1..s), normalised to sum 1 at every site.  a_in [I][2]:
    the vector at the site in front of the first (default: the initial distribution (1 - F, F))."""
    eprob = np.asarray(eprob, dtype=np.float64)
    I, S, _ = eprob.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    q = np.stack([1 - F, F], axis=1)
    e = np.exp(eprob - eprob.max(axis=2, keepdims=True))
    c = coancestry(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)), pos)
    a = np.empty((I, S, 2))
    v = q.copy() if a_in is None else np.asarray(a_in, dtype=np.float64) / np.sum(a_in, axis=1, keepdims=True)
    for s in range(S):
        cs = c[:, s, None]
        v = (cs * v + (1 - cs) * v.sum(axis=1, keepdims=True) * q) * e[:, s]
        v = v / v.sum(axis=1, keepdims=True)
        a[:, s] = v
    return a


def thresholds(a, pos, F, alpha, d_after=None):
    """(s0, t0, s1, t1), each [I][S]: z_s = 1 iff u * s_l < t_l with l = z_{s+1}; n_k = a_s(k)
    T_{s+1}(k, l), s_l = n0 + n1, t_l = n1.  At the last site (d_after None) and in front of a
    chromosome start T does not depend on k: both l give (a(0) + a(1), a(1)).  d_after: the
    distance of the site that follows the last one (a shard that is not the chain's last)."""
    I, S, _ = a.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,))
    nxt = np.r_[np.asarray(pos, dtype=np.float64)[1:], np.inf if d_after is None else d_after]
    c = coancestry(alpha, nxt)
    free = np.isinf(nxt)[None, :]
    q0, q1 = (1 - F)[:, None], F[:, None]
    A0 = np.where(free, 1.0, (1 - c) * q0)
    A1 = np.where(free, 1.0, (1 - c) * q1)
    cc = np.where(free, 0.0, c)
    a0, a1 = a[..., 0], a[..., 1]
    n00, n10 = a0 * (A0 + cc), a1 * A0
    n01, n11 = a0 * A1, a1 * (A1 + cc)
    return n00 + n10, n10, n01 + n11, n11


def cond_probs(thr):
    """p [I][S][2]: P(z_s = 1 | z_{s+1} = l, data) = n1 / (n0 + n1); NaN where n0 = n1 = 0 (a
    state z_{s+1} = l that the data exclude: u * 0 < 0 is false whatever the rounding)."""
    s0, t0, s1, t1 = thr
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([t0 / s0, t1 / s1], axis=-1)


def backward_draw(thr, u, state_after=None):
    """paths [R][I][S] uint8 from u [R][I][S], site by site from the last to the first.
    state_after [R][I]: z of the site that follows the last one (None: there is none)."""
    s0, t0, s1, t1 = thr
    z0 = u * s0[None] < t0[None]
    z1 = u * s1[None] < t1[None]
    R, I, S = u.shape
    out = np.empty((R, I, S), dtype=np.uint8)
    z = np.zeros((R, I), dtype=bool) if state_after is None else np.asarray(state_after).astype(bool)
    for s in range(S - 1, -1, -1):
        z = np.where(z, z1[:, :, s], z0[:, :, s])
        out[:, :, s] = z
    return out


def min_margin(thr, u):
    """The smallest |u - n1 / (n0 + n1)| over (draw, individual, site, l)."""
    p = cond_probs(thr)
    return float(min(np.nanmin(np.abs(u - p[None, ..., 0])), np.nanmin(np.abs(u - p[None, ..., 1]))))


def posterior(a, eprob, pos, F, alpha):
    """Unsnapped P(z_s = 1 | data) [I][S] from the filter a and a normalised backward pass."""
    I, S, _ = a.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), (I,))
    q = np.stack([1 - F, F], axis=1)
    e = np.exp(eprob - eprob.max(axis=2, keepdims=True))
    c = coancestry(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (I,)), pos)
    post = np.empty((I, S))
    w = np.ones((I, 2))
    for s in range(S - 1, -1, -1):
        x = a[:, s] * w
        post[:, s] = x[:, 1] / x.sum(axis=1)
        cs = c[:, s, None]
        uu = e[:, s] * w
        w = cs * uu + (1 - cs) * (q * uu).sum(axis=1, keepdims=True)
        w = w / w.sum(axis=1, keepdims=True)
    return post


STATS_DTYPE = np.dtype([("ibd_sites", np.uint64), ("n_tracts", np.uint64),
                        ("longest_sites", np.uint64), ("ibd_mb", np.float64)])


def path_stats(paths, pos):
    """Records [...][I] of paths [...][I][S] by run-length encoding: runs of 1 cut at chromosome
    starts (pos = +inf); ibd_mb = the sum over runs of the distances from first to last site."""
    paths = np.asarray(paths)
    pos = np.asarray(pos, dtype=np.float64)
    S = paths.shape[-1]
    cs = np.isinf(pos)
    cs[0] = True
    flat = paths.reshape(-1, S).astype(bool)
    out = np.zeros(len(flat), dtype=STATS_DTYPE)
    for k, x in enumerate(flat):
        prev = np.r_[False, x[:-1]]
        nxt = np.r_[x[1:], False]
        starts = np.flatnonzero(x & (~prev | cs))
        ends = np.flatnonzero(x & (~nxt | np.r_[cs[1:], True]))
        lens = ends - starts + 1
        cont = x & prev & ~cs                       # sites that continue a run
        out[k] = (x.sum(), len(starts), lens.max() if len(lens) else 0,
                  float(np.sum(np.where(cont, np.where(cs, 0.0, pos), 0.0))))
    return out.reshape(paths.shape[:-1])


def calibration_case(pkg):
    """The cohort of the statistical test, shared by its calibration on the restatement
    (tests/test_sample_cpu.py) and its run on the device (tests/test_gpu_sample.py): 20 x 5000,
    three chromosomes, missing cells, random indF / alpha, one frequency.  Returns (simulated data,
    normalised log likelihoods, indF, alpha, freq, draws, seed)."""
    I, S = 20, 5000
    d = pkg.simulate.simulate(I, S, seed=19, n_chrom=3, indF="r", alpha="r", missing_rate=0.03)
    rng = np.random.default_rng(20)
    return (d, pkg.simulate.normalise_log_gl(d.gl), rng.uniform(0.02, 0.95, I),
            rng.uniform(0.01, 2.0, I), 0.15, 256, 77)
