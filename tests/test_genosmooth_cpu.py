"""The smoothed genotype posteriors without a GPU: the two numpy yardsticks of
tests/genosmooth_util.py against enumeration over all paths (likelihoods and called genotypes),
against each other on the cohort of tests/test_gpu_genosmooth.py (the figure that test's tolerance
is made of), Fisher's identity with freq_info's score, the EM update of the frequency, a dead
cell, the share of near-tied cells on the cohort, and the two helpers of the binding.

Tolerances: against enumeration rtol 1e-12 (2^10 paths of 10 factors each in np.longdouble on one
side, a forward-backward in float64 or longdouble on the other: far below); for identities between
sums 64 eps times the sum of the absolute values of the terms on both sides."""
import numpy as np
import pytest

import freqinfo_util as fu
import genosmooth_util as gu

EPS = float(np.finfo(np.float64).eps)
YARDSTICKS = (("A", gu.geno_smooth_a), ("B", gu.geno_smooth_b))


def _enumerate(p_i, pos, F, alpha, freq):
    """One individual, all 2^S paths, np.longdouble: per site the joint posterior J[z][g] / B of
    the site's state and genotype, [S][2][3], and the cavity weights [S][2] (the posterior of the
    site's state with the site's own data left out)."""
    ld = np.longdouble
    S = len(pos)
    z = (np.arange(1 << S)[:, None] >> np.arange(S)[None, :]) & 1           # [paths][S]
    q = np.array([1 - F, F], dtype=ld)
    f = np.asarray(freq, dtype=np.float64).astype(ld)
    om = 1 - f
    p = np.asarray(p_i).astype(ld)
    h = np.stack([np.stack([om * om, 2 * f * om, f * f], axis=1),
                  np.stack([om, 0 * f, f], axis=1)], axis=1)                # [S][2][3]
    e = (h * p[:, None, :]).sum(axis=2)                                     # [S][2]
    prior = np.ones(1 << S, dtype=ld)
    for s in range(S):
        if s == 0 or np.isinf(pos[s]):
            prior = prior * q[z[:, s]]
        else:
            c = np.exp(-ld(alpha) * ld(pos[s]))
            prior = prior * ((1 - c) * q[z[:, s]] + c * (z[:, s] == z[:, s - 1]))
    em = np.stack([e[s][z[:, s]] for s in range(S)], axis=1)                # [paths][S]
    J = np.zeros((S, 2, 3), dtype=ld)
    cav = np.zeros((S, 2), dtype=ld)
    for s in range(S):
        rest = prior * np.prod(np.delete(em, s, axis=1), axis=1)
        for k in range(2):
            wk = rest[z[:, s] == k].sum()
            cav[s, k] = wk
            J[s, k] = wk * h[s, k] * p[s]
        cav[s] /= cav[s].sum()
        J[s] /= J[s].sum()
    return J, cav


def _small_case(called):
    rng = np.random.default_rng(11)
    I, S = 3, 9
    p = rng.dirichlet(np.ones(3), size=(S, I))
    if called:
        g = rng.integers(0, 4, size=(S, I))            # 3: missing
        p = np.where((g == 3)[..., None], 1.0 / 3, np.eye(3)[np.minimum(g, 2)])
    pos = rng.uniform(0.01, 0.6, S)
    pos[0] = pos[5] = np.inf
    freq = rng.uniform(0.1, 0.6, S)
    return p, pos, np.array([0.3, 0.6, 0.85]), np.array([0.4, 1.5, 0.05]), freq


@pytest.mark.parametrize("called", [False, True], ids=["likelihoods", "called"])
def test_closed_form_equals_enumeration(called):
    """3 x 9 with a chromosome start inside: post, the site sums and the region sums of both
    yardsticks against the enumeration over all 512 paths; called genotypes give posteriors that
    are one-hot EXACTLY, missing cells lie strictly inside (0, 1)."""
    p, pos, F, A, freq = _small_case(called)
    S, I = p.shape[:2]
    regs = np.array([(0, 4), (4, 9)])
    J = np.empty((S, I, 2, 3), dtype=np.longdouble)
    cav = np.empty((S, I, 2), dtype=np.longdouble)
    for i in range(I):
        J[:, i], cav[:, i] = _enumerate(p[:, i], pos, F[i], A[i], freq)
    P = J.sum(axis=2)
    hp = cav[..., 0] * (2 * freq * (1 - freq))[:, None]
    want = {"post": P, "n0": P[..., 0].sum(1), "n1": P[..., 1].sum(1), "n2": P[..., 2].sum(1),
            "het_prior": hp.sum(1), "ibd": J[:, :, 1].sum(axis=(1, 2)), "alt_ibd": J[:, :, 1, 2].sum(1),
            "het": np.array([P[a:b, :, 1].sum(0) for a, b in regs]).T,
            "r_het_prior": np.array([hp[a:b].sum(0) for a, b in regs]).T,
            "non_ibd": np.array([J[a:b, :, 0].sum(axis=(0, 2)) for a, b in regs]).T,
            "dosage": np.array([(P[a:b, :, 1] + 2 * P[a:b, :, 2]).sum(0) for a, b in regs]).T}
    for name, fn in YARDSTICKS:
        got = fn(p, pos, F, A, freq, regs)
        for k, w in want.items():
            np.testing.assert_allclose(got[k], np.asarray(w, dtype=np.float64), rtol=1e-12, atol=1e-300,
                                       err_msg=f"{name} {k}")
        assert np.array_equal(got["call"], np.argmax(np.asarray(P, dtype=np.float64), axis=2)), name
        if called:
            hot = p.max(axis=2) == 1.0
            assert hot.sum() > 10 and (~hot).sum() > 3
            assert np.array_equal(got["post"][hot], p[hot]), name          # exactly one-hot
            assert np.array_equal(got["call"][hot], np.argmax(p[hot], axis=1)), name
            inner = got["post"][~hot]
            assert (inner[:, [0, 2]] > 0).all() and (inner < 1).all(), name


@pytest.fixture(scope="module")
def cohort_ab(pkg):
    d, gl, F, A, freq = fu.gpu_cohort(pkg)
    p = np.exp(gl)
    regs = pkg.chromosome_regions(d.pos_dist_mb)
    return (d, p, F, A, freq, gu.geno_smooth_a(p, d.pos_dist_mb, F, A, freq, regs),
            gu.geno_smooth_b(p, d.pos_dist_mb, F, A, freq, regs))


def test_yardstick_spread_on_the_gpu_cohort(cohort_ab):
    """|A - B| on the cohort of the GPU test, per field, in the measure of genosmooth_util.spread
    (printed; genosmooth_util.SPREAD quotes it, the GPU tolerance is 16 x it).  Every entry is
    finite in both."""
    d, p, F, A, freq, a, b = cohort_ab
    for r in (a, b):
        for f in ("post",) + gu.SITE_FIELDS + tuple(gu._key(f) for f in gu.REGION_FIELDS):
            assert np.isfinite(r[f]).all(), f
    s = gu.spread(a, b)
    print("\n  spread |A - B| / scale: " + ", ".join(f"{k} {v:.3e}" for k, v in s.items()))
    assert set(s) == set(gu.SPREAD)
    # what the GPU test quotes is what is measured here (within a factor of two: libm versions)
    for k, v in s.items():
        assert v <= 2 * gu.SPREAD[k], (k, v, gu.SPREAD[k])
        assert gu.SPREAD[k] <= 4 * v, (k, v, gu.SPREAD[k])


def test_near_ties_are_rare_on_the_gpu_cohort(cohort_ab):
    """The share of the cohort's cells whose two largest posteriors lie within the post tolerance
    of each other -- the only cells the GPU test's call comparison may leave out -- is below 0.1 %;
    elsewhere the two yardsticks call the same genotype."""
    d, p, F, A, freq, a, b = cohort_ab
    tie = gu.near_ties(b["post"], gu.TOL["post"])
    print(f"\n  near ties: {tie.sum()} of {tie.size} cells")
    assert tie.mean() < 1e-3
    assert np.array_equal(a["call"][~tie], b["call"][~tie])
    assert set(np.unique(b["call"])) == {0, 1, 2}


def test_fisher_identity_and_em_freq(pkg, cohort_ab):
    """(a) in B: score f (1 - f) = (n1 + 2 n2 - alt_ibd) - f (2 I - ibd) per site, freq_info_b's
    score on one side and the site sums on the other; geno_em_freq is the quotient, and
    em_freq - freq is the score in frequency units."""
    d, p, F, A, freq, a, b = cohort_ab
    I = d.n_ind
    fi = fu.freq_info_b(p, d.pos_dist_mb, F, A, freq)
    v = freq * (1 - freq)
    lhs = fi["score"] * v
    rhs = (b["n1"] + 2 * b["n2"] - b["alt_ibd"]) - freq * (2 * I - b["ibd"])
    tol = 64 * EPS * (fi["abs_score"] * v + b["abs_n1"] + 2 * b["abs_n2"] + b["abs_alt_ibd"]
                      + freq * (2 * I + b["abs_ibd"]))
    err = np.abs(lhs - rhs)
    print(f"\n  largest |score f (1 - f) - site sums| {err.max():.2e} at a scale of {np.abs(lhs).max():.1f}")
    assert (err <= tol).all() and np.abs(fi["score"]).max() > 1
    sites = np.zeros(d.n_sites, dtype=pkg.GENO_SITE_STAT_DTYPE)
    for f in gu.SITE_FIELDS:
        sites[f] = b[f]
    em = pkg.geno_em_freq(sites, I)
    assert em.shape == (d.n_sites,) and (em > 0).all() and (em < 1).all()
    np.testing.assert_array_equal(em, (b["n1"] + 2 * b["n2"] - b["alt_ibd"]) / (2 * I - b["ibd"]))
    den = 2 * I - b["ibd"]
    assert (np.abs((em - freq) * den - lhs) <= tol + 4 * EPS * den).all()
    # so the update moves the way the score points, wherever the score is not rounding
    clear = np.abs(lhs) > 2 * tol
    assert clear.mean() > 0.9 and np.array_equal(np.sign(em - freq)[clear], np.sign(fi["score"])[clear])


def test_a_dead_cell_is_nan_exactly_there():
    """A called genotype that a frequency of 0 or 1 excludes: NaN in post and 3 in call at that
    cell, NaN in the site's and the region's sums (not het_prior), nothing else."""
    p, pos, F, A, freq = _small_case(True)
    S, I = p.shape[:2]
    s = 5                                              # a chromosome of its own: the walks stay defined
    pos[s] = pos[s + 1] = np.inf
    freq[s] = 0.0
    p[s] = np.eye(3)[[0, 2, 1]]                        # individuals 1 and 2 are excluded
    regs = np.array([(0, 5), (5, 9)])
    for name, fn in YARDSTICKS:
        got = fn(p, pos, F, A, freq, regs)
        dead = np.zeros((S, I), dtype=bool)
        dead[s, 1:] = True
        assert np.array_equal(np.isnan(got["post"]).any(axis=2), dead), name
        assert np.array_equal(np.isnan(got["post"]).all(axis=2), dead), name
        assert np.array_equal(got["call"] == 3, dead), name
        assert np.array_equal(got["post"][s, 0], [1.0, 0.0, 0.0]), name
        for f in gu.SITE_FIELDS:
            assert np.array_equal(np.isnan(got[f]), (np.arange(S) == s) & (f != "het_prior")), (name, f)
        # at a frequency of 0 every term of the site's het_prior is 0: the measure asks for 0 exactly
        assert got["het_prior"][s] == 0 and got["abs_het_prior"][s] == 0
        assert gu.spread({"het_prior": got["het_prior"]}, got)["het_prior"] == 0
        assert gu.spread({"het_prior": got["het_prior"] + 1e-300}, got)["het_prior"] == np.inf
        for f in gu.REGION_FIELDS:
            want = np.zeros((I, 2), dtype=bool)
            want[1:, 1] = f != "het_prior"
            assert np.array_equal(np.isnan(got[gu._key(f)]), want), (name, f)


def test_helpers(pkg):
    sites = np.zeros(3, dtype=pkg.GENO_SITE_STAT_DTYPE)
    sites["n1"], sites["n2"], sites["alt_ibd"], sites["ibd"] = [2, 1, 0], [1, 0, 0], [0.5, 0, 0], [1, 0.5, 4]
    em = pkg.geno_em_freq(sites, 2)
    np.testing.assert_array_equal(em[:2], [3.5 / 3, 1 / 3.5])
    assert np.isnan(em[2])                             # 2 I - ibd = 0
    reg = np.zeros((2, 2), dtype=pkg.GENO_REGION_STAT_DTYPE)
    reg["het"], reg["non_ibd"] = [[1, 2], [0, 3]], [[4, 0], [0, 6]]
    out = pkg.het_outside_ibd(reg)
    assert out.shape == (2, 2)
    np.testing.assert_array_equal(out[[0, 1], [0, 1]], [0.25, 0.5])
    assert np.isnan(out[0, 1]) and np.isnan(out[1, 0])
    assert pkg.GENO_SITE_STAT_DTYPE.names == gu.SITE_FIELDS and pkg.GENO_SITE_STAT_DTYPE.itemsize == 48
    assert pkg.GENO_REGION_STAT_DTYPE.names == gu.REGION_FIELDS and pkg.GENO_REGION_STAT_DTYPE.itemsize == 32
