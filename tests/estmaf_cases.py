"""Inputs for est_maf (the allele-frequency step) chosen by the test, not by an E-step.

cases(I, S, seed) returns site-major natural-log likelihoods [S][I][3], normalised as
simulate.normalise_log_gl leaves them, IBD posteriors [S][I] and one family label per site.
One call mixes every family over its sites (site s takes recipe s mod len(RECIPES)), so that a
single launch sees them side by side: neighbouring sites share a wave in the four-sites-per-wave
kernels and a scan workgroup in the resuming ones.  Pure numpy, fixed seeds, no GPU.

The families, and what each is for:
  sim_d2 / sim_d5 / sim_d20   sequencing-like likelihoods at mean depth 2, 5, 20; the true
                    frequency cycles through FREQS, whose far values make a site's odds leave the
                    first interpolation interval (every site starts at 0.01)
  all_missing       every cell uninformative
  one_first / one_edge_m1 / one_edge / one_last   all missing but ONE informative individual, at
                    index 0, at full_slots * BLOCK - 1 (the last slot the kernel reads without a
                    mask), at that index + 1 (the first masked one) and at I - 1
  mono_ref / mono_alt   every individual confidently homozygous: the frequency creeps to 0 like
                    1/k (the 101-pass cap) / the odds grow without bound
  sharp / flat      likelihood differences of several hundred log units / of a few thousandths
  post_snapped / post_half / post_tiny   posteriors exactly 0 or 1 (what check_interv leaves);
                    half of them snapped; 1e-300 and 1e-17
  one_minus_eps / one_minus_eps_sharp / one_minus_eps_mono   posteriors 1 - eps, eps from 2^-53
                    to 1e-9, never 1: the reference's doubles cancel in 2(1-f)f - 2(1-f)f F
  called / called_het1 / called_snapped   called genotypes as dense one-hot likelihoods
                    (0 / -1e15); het1 puts called heterozygotes at posterior exactly 1 (every
                    linear weight of the cell vanishes: the log-space route), snapped all of them
"""
import numpy as np

FREQS = (1e-4, 0.01, 0.05, 0.2, 0.5, 0.8, 0.99, 0.9999)
MISSING_LOG = -1e15      # the reference's stand-in for log 0 (called genotypes)

# the GPU test's cohort sizes: both ends of every size class of the frequency step's dispatch
SIZES = (1, 2, 3, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025,
         1536, 1537, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 7168, 7169,
         8192, 8193, 9000)
N_SITES = 301            # 7 x 43 recipes: five scan workgroups of 64, two workgroups of 256
SEED = 20240917


def size_class(I):
    """(NI, BLOCK, full_slots) of the register kernel that holds I individuals per site (the
    dispatch of fast_estmaf without the four-sites-per-wave kernels), full_slots being the slots
    per lane that the kernel reads unmasked; None above 8192 (streaming kernel)."""
    table = ((64, 1, 64, 0), (128, 2, 64, 1), (256, 4, 64, 2), (512, 8, 64, 4), (768, 12, 64, 8),
             (1024, 16, 64, 12), (1536, 12, 128, 0), (2048, 16, 128, 8), (3072, 12, 256, 0),
             (4096, 16, 256, 8), (5120, 10, 512, 0), (6144, 12, 512, 0), (7168, 14, 512, 0),
             (8192, 16, 512, 8))
    for top, ni, block, full in table:
        if I <= top:
            return ni, block, full
    return None


def edge_index(I):
    """Index of the last individual in an unmasked slot (full_slots * BLOCK - 1), clamped into
    the cohort; where the class has no unmasked slot, the last lane of the first wave."""
    sc = size_class(I)
    e = (sc[2] * sc[1] - 1) if sc and sc[2] else 63
    return max(0, min(e, I - 1))


def _normalise(gl):
    # simulate.normalise_log_gl, restated (the generator imports nothing from the package)
    m = gl.max(axis=-1, keepdims=True)
    return gl - (m + np.log(np.exp(gl - m).sum(axis=-1, keepdims=True)))


def _sim_gl(rng, I, depth, freq, err=0.01):
    """Unnormalised log GLs of I individuals at one site: genotypes in Hardy-Weinberg
    proportions, Poisson(depth) reads, binomial alternative reads with error err."""
    geno = rng.binomial(2, freq, I)
    n = rng.poisson(depth, I)
    p_alt = np.array([err, 0.5, 1 - err])
    k = rng.binomial(n, p_alt[geno])
    gl = k[:, None] * np.log(p_alt)[None, :] + (n - k)[:, None] * np.log1p(-p_alt)[None, :]
    return gl, geno


def _one_informative(I, at, which):
    gl = np.zeros((I, 3))
    gl[at] = ((0.0, -8.0, -16.0), (-8.0, 0.0, -8.0), (-16.0, -8.0, 0.0))[which]
    return gl


def _called(rng, I, freq):
    _, geno = _sim_gl(rng, I, 20, freq)
    gl = np.full((I, 3), MISSING_LOG)
    gl[np.arange(I), geno] = 0.0
    miss = rng.random(I) < 0.05          # an uncalled cell is uniform
    gl[miss] = 0.0
    return gl, np.where(miss, -1, geno)


def _one_minus_eps(rng, I):
    eps = np.array([2.0 ** -53, 1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9])
    post = 1.0 - eps[rng.integers(0, len(eps), I)]
    assert np.all(post < 1.0)
    return post


# (label, likelihoods, posteriors): the likelihood makers take (rng, I, round) and return [I][3]
# unnormalised logs (and, for called sites, the genotypes); `round` is s // len(RECIPES) and makes
# the repeats of a recipe differ in their frequency
def _recipes():
    R = []

    def uniform(rng, I, aux):
        return rng.random(I)

    def snapped(rng, I, aux):
        return (rng.random(I) < 0.3).astype(np.float64)

    def half(rng, I, aux):
        return np.where(rng.random(I) < 0.5, (rng.random(I) < 0.3).astype(np.float64),
                        rng.random(I))

    def tiny(rng, I, aux):
        return np.where(rng.random(I) < 0.5, 1e-300, 1e-17)

    def skew(rng, I, aux):               # most individuals not IBD, a few nearly so
        return rng.beta(0.3, 1.5, I)

    def ome(rng, I, aux):
        return _one_minus_eps(rng, I)

    def het1(rng, I, geno):              # called heterozygotes at posterior exactly 1
        post = rng.random(I)
        hets = np.flatnonzero(geno == 1)
        if len(hets):
            post[hets[:max(1, len(hets) // 2)]] = 1.0
        else:                            # no heterozygote drawn: the site still needs one
            post[0] = 1.0
        return post

    def sim(depth, j0):
        return lambda rng, I, rnd: _sim_gl(rng, I, depth, FREQS[(j0 + rnd) % len(FREQS)])[0]

    # every depth meets every frequency within len(FREQS) rounds; three recipes per depth start
    # at different frequencies so that six rounds suffice
    for depth, name in ((2, "sim_d2"), (5, "sim_d5"), (20, "sim_d20")):
        R.append((name, sim(depth, 0), uniform))
        R.append((name, sim(depth, 3), skew))
        R.append((name, sim(depth, 6), half))
    R.append(("all_missing", lambda rng, I, rnd: np.zeros((I, 3)), uniform))
    R.append(("one_first", lambda rng, I, rnd: _one_informative(I, 0, rnd % 3), uniform))
    R.append(("one_edge_m1", lambda rng, I, rnd: _one_informative(I, edge_index(I), rnd % 3), uniform))
    R.append(("one_edge", lambda rng, I, rnd: _one_informative(I, min(edge_index(I) + 1, I - 1), rnd % 3),
              uniform))
    R.append(("one_last", lambda rng, I, rnd: _one_informative(I, I - 1, rnd % 3), uniform))
    mono = np.array([0.0, 20 * np.log(0.5 / 0.99), 20 * np.log(0.01 / 0.99)])
    weak = mono / 20                     # one read each: the frequency creeps, 1/k, into the cap
    R.append(("mono_ref", lambda rng, I, rnd: np.tile(mono, (I, 1)), uniform))
    R.append(("mono_ref", lambda rng, I, rnd: np.tile(weak, (I, 1)), snapped))
    R.append(("mono_alt", lambda rng, I, rnd: np.tile(mono[::-1], (I, 1)), uniform))
    R.append(("mono_alt", lambda rng, I, rnd: np.tile(weak[::-1], (I, 1)), snapped))
    R.append(("sharp", lambda rng, I, rnd: 3.5 * _sim_gl(rng, I, 20, FREQS[(2 + rnd) % 8])[0], uniform))
    R.append(("sharp", lambda rng, I, rnd: 3.5 * _sim_gl(rng, I, 20, FREQS[(5 + rnd) % 8])[0], half))
    R.append(("flat", lambda rng, I, rnd: 1e-3 * _sim_gl(rng, I, 2, FREQS[(3 + rnd) % 8])[0], uniform))
    R.append(("flat", lambda rng, I, rnd: 1e-3 * _sim_gl(rng, I, 2, FREQS[(4 + rnd) % 8])[0], skew))
    for name, post in (("post_snapped", snapped), ("post_half", half), ("post_tiny", tiny)):
        R.append((name, sim(5, 1), post))
        R.append((name, sim(20, 4), post))
        R.append((name, sim(2, 6), post))
    R.append(("one_minus_eps", sim(5, 0), ome))
    R.append(("one_minus_eps", sim(20, 3), ome))
    R.append(("one_minus_eps", sim(2, 5), ome))
    R.append(("one_minus_eps_sharp", lambda rng, I, rnd: 3.5 * _sim_gl(rng, I, 20, FREQS[(3 + rnd) % 8])[0],
              ome))
    R.append(("one_minus_eps_mono", lambda rng, I, rnd: np.tile(mono, (I, 1)), ome))
    R.append(("one_minus_eps_mono", lambda rng, I, rnd: np.tile(mono[::-1], (I, 1)), ome))

    def called(j0):
        return lambda rng, I, rnd: _called(rng, I, FREQS[(j0 + rnd) % len(FREQS)])

    R.append(("called", called(2), uniform))
    R.append(("called", called(5), skew))
    R.append(("called_het1", called(3), het1))
    R.append(("called_het1", called(4), het1))
    R.append(("called_snapped", called(3), snapped))
    R.append(("called_snapped", called(6), snapped))
    # neighbours in the list are neighbours in a wave: interleave instead of grouping by family
    order = np.random.default_rng(7).permutation(len(R))
    return [R[k] for k in order]


RECIPES = _recipes()
FAMILIES = tuple(sorted({r[0] for r in RECIPES}))
ONE_MINUS_EPS = tuple(f for f in FAMILIES if f.startswith("one_minus_eps"))


def cases(I, S=N_SITES, seed=SEED):
    """(gl [S][I][3] normalised natural logs, post [S][I], labels [S] of str)."""
    gl = np.empty((S, I, 3))
    post = np.empty((S, I))
    labels = []
    for s in range(S):
        label, make_gl, make_post = RECIPES[s % len(RECIPES)]
        rng = np.random.default_rng([seed, I, s])
        g = make_gl(rng, I, s // len(RECIPES))
        aux = None
        if isinstance(g, tuple):
            g, aux = g
        if label == "called_het1" and not np.any(aux == 1):
            g[0] = (MISSING_LOG, 0.0, MISSING_LOG)       # (tiny cohorts: make the heterozygote)
            aux[0] = 1
        gl[s] = g
        post[s] = make_post(rng, I, aux)
        labels.append(label)
    return _normalise(gl), post, np.array(labels)


def log_space_sites(gl, post):
    """Sites with a cell whose linear weights all vanish (exp of both homozygotes' likelihoods
    is 0 and the posterior is exactly 1): est_maf takes the reference-order log-space route."""
    hom0 = (np.exp(gl[..., 0]) == 0) & (np.exp(gl[..., 2]) == 0)
    return np.any(hom0 & (post == 1.0), axis=1)


# families of many equal terms over 101 passes: at 4097 and more individuals the oracle's serial
# double sums were measured 1e-12 ... 3.5e-12 from the anchor there (the GPU within 1e-15 of it),
# so at large cohorts ALL their sites are judged by the anchor
ANCHOR_EVERY_SITE = ("mono_ref", "mono_alt", "post_tiny", "post_snapped", "post_half")


def anchor_sites(labels):
    """The fixed subsample the binary128 anchor is computed on at large cohorts: the first site
    of every recipe (so every family, with each of its likelihood / posterior pairings), and
    every site of the families in ANCHOR_EVERY_SITE."""
    labels = np.asarray(labels)
    pick = set(range(min(len(RECIPES), len(labels))))
    pick |= set(np.flatnonzero(np.isin(labels, ANCHOR_EVERY_SITE)).tolist())
    return np.array(sorted(pick))


EPSILON = 1e-5           # est_maf's stopping threshold (gen_func.hpp:16)


def marginal(deltas, rel=1e-6):
    """Is some pass's stopping decision marginal: |delta| within rel (relative) of EPSILON?"""
    d = np.asarray(deltas)
    return bool(np.any(np.abs(d - EPSILON) <= rel * EPSILON))
