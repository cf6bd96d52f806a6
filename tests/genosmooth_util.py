"""The yardstick of the smoothed-genotype tests (nghmm_geno_smooth, include/nghmm.h), in numpy,
twice: (A) float64 on the weights of freqinfo_util.freq_info_a, (B) np.longdouble on those of
freqinfo_util.freq_info_b.  Both take the two cavity weights (w0, w1) = (1 - c, c) of every cell
from there and restate the closed form of the header:

    J[z][g] = w_z h_z[g] p_g,  h_0 = ((1 - f)^2, 2 f (1 - f), f^2),  h_1 = (1 - f, 0, f)
    B = sum J,  P_g = (J[0][g] + J[1][g]) / B,  pi = (J[1][0] + J[1][2]) / B,
    non = (J[0][0] + J[0][1] + J[0][2]) / B

tests/test_genosmooth_cpu.py checks both against enumeration over all paths before
tests/test_gpu_genosmooth.py uses B.

Every function takes LINEAR likelihoods p [S][I][3], distances pos [S] (+inf: a chromosome start),
F and alpha [I], freq [S] and regions [R][2] (or None), and returns a dict of float64 arrays:
    post [S][I][3], call [S][I] uint8 (3: B = 0 or a NaN posterior)
    n0, n1, n2, het_prior, ibd, alt_ibd [S]            the site sums (over the individuals)
    het, r_het_prior, non_ibd, dosage [I][R]           the region sums (over the region's sites)
    abs_<name>                                         the sum of the absolute values of the terms
    w0, cavity [I][S]                                  the weights used
(r_het_prior: the region records' het_prior, which shares its name with the site records'.)"""
import numpy as np

import freqinfo_util as fu

SITE_FIELDS = ("n0", "n1", "n2", "het_prior", "ibd", "alt_ibd")
REGION_FIELDS = ("het", "het_prior", "non_ibd", "dosage")


def _key(f):
    """The yardstick's name of a region field."""
    return "r_het_prior" if f == "het_prior" else f


def _closed_form(fi, p, freq, regions, dt):
    p = np.asarray(p).astype(dt)
    w0 = np.ascontiguousarray(fi["w0"].T).astype(dt)              # [S][I]
    w1 = np.ascontiguousarray(fi["cavity"].T).astype(dt)
    f = np.asarray(freq, dtype=np.float64).astype(dt)[:, None]
    om = 1 - f
    p0, p1, p2 = p[..., 0], p[..., 1], p[..., 2]
    hh = 2 * f * om
    j00, j01, j02 = w0 * om * om * p0, w0 * hh * p1, w0 * f * f * p2
    j10, j12 = w1 * om * p0, w1 * f * p2
    B = j00 + j01 + j02 + j10 + j12
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.stack([(j00 + j10) / B, j01 / B, (j02 + j12) / B], axis=2)
        pi = (j10 + j12) / B
        non = (j00 + j01 + j02) / B
        alt = j12 / B
    hp = w0 * hh
    out = {"post": P.astype(np.float64), "w0": fi["w0"], "cavity": fi["cavity"]}
    # (argmax takes the first of equal values; a NaN row is overwritten)
    P64 = out["post"]
    call = np.argmax(np.where(np.isnan(P64), -1.0, P64), axis=2).astype(np.uint8)
    call[np.isnan(P64).any(axis=2) | ~(np.asarray(B, dtype=np.float64) > 0)] = 3
    out["call"] = call
    terms = {"n0": P[..., 0], "n1": P[..., 1], "n2": P[..., 2], "het_prior": hp, "ibd": pi, "alt_ibd": alt}
    for k, t in terms.items():
        out[k] = t.sum(axis=1).astype(np.float64)
        out["abs_" + k] = np.abs(t).sum(axis=1).astype(np.float64)
    out["cells"] = {"het": P[..., 1], "r_het_prior": hp, "non_ibd": non, "dosage": P[..., 1] + 2 * P[..., 2]}
    out.update(region_sums(out, regions))
    return out


def region_sums(yard, regions):
    """The region sums [I][R] of a yardstick's cells over another set of regions: a dict of the
    four fields and their abs_ companions."""
    reg = np.zeros((0, 2), dtype=np.int64) if regions is None else np.asarray(regions, dtype=np.int64)
    out = {}
    for k, t in yard["cells"].items():
        I = t.shape[1]
        out[k] = np.array([t[a:b].sum(axis=0) for a, b in reg], dtype=t.dtype).reshape(len(reg), I).T.astype(np.float64)
        out["abs_" + k] = np.array([np.abs(t[a:b]).sum(axis=0) for a, b in reg],
                                   dtype=t.dtype).reshape(len(reg), I).T.astype(np.float64)
    return out


def geno_smooth_a(p, pos, F, alpha, freq, regions=None):
    """Yardstick A: float64, on freq_info_a's weights."""
    return _closed_form(fu.freq_info_a(p, pos, F, alpha, freq), p, freq, regions, np.float64)


def geno_smooth_b(p, pos, F, alpha, freq, regions=None):
    """Yardstick B: np.longdouble, on freq_info_b's weights."""
    return _closed_form(fu.freq_info_b(p, pos, F, alpha, freq), p, freq, regions, np.longdouble)


def as_dict(res):
    """What NgsFHMM.geno_smooth returned, under the yardstick's names."""
    out = {}
    if "post" in res:
        out["post"] = res["post"]
    if "call" in res:
        out["call"] = res["call"]
    if "sites" in res:
        for f in SITE_FIELDS:
            out[f] = res["sites"][f]
    if "regions" in res:
        for f in REGION_FIELDS:
            out[_key(f)] = res["regions"][f]
    return out


def spread(got, want, where=None):
    """Per field the largest |got - want| in its measure: absolute for post, over the sum of the
    absolute values of the entry's terms (want's) for the sums.  Only the fields in both; where:
    {field: mask} restricts a field to the entries to compare (the rest must be tested apart)."""
    out = {}
    for f in ("post",) + SITE_FIELDS + tuple(_key(f) for f in REGION_FIELDS):
        if f not in got or f not in want or not np.asarray(got[f]).size:
            continue
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if f == "post":
            err = np.abs(g - w)
        else:
            # (a sum all of whose terms are 0 -- het_prior at a frequency of 0 or 1 -- has the scale
            # 0: it must be 0 exactly)
            scale = np.asarray(want["abs_" + f])
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.where(scale == 0, np.where(g == w, 0.0, np.inf), np.abs(g - w) / scale)
        if where is not None and f in where:
            err = err[where[f]]
        out[f] = float(np.max(err))
    return out


def near_ties(post, tol):
    """[S][I] bool: the two largest posteriors of the cell lie within tol of each other."""
    top = np.sort(post, axis=2)
    return ~(top[..., 2] - top[..., 1] > tol)


def hand_regions(pos):
    """A hand-made set on the GPU cohort: a region that crosses both a multiple of 2048 and a
    chromosome start, with gaps between the regions and sites in front of the first and behind the
    last that belong to none."""
    starts = [int(s) for s in np.flatnonzero(np.isinf(pos)) if s > 0]
    S = len(pos)
    # the chromosome start nearest to a multiple of 2048, and a region around both
    s = min(starts, key=lambda x: min(abs(x - m) for m in range(2048, S, 2048)))
    m = min(range(2048, S, 2048), key=lambda x: abs(x - s))
    lo, hi = min(s, m) - 37, max(s, m) + 41
    assert 20 < lo and hi < S - 10
    regs = [(11, lo - 5), (lo, hi), (hi + 9, S - 2)]
    assert regs[0][1] - regs[0][0] > 100
    return np.array(regs, dtype=np.int64)


# The spread of the two yardsticks on freqinfo_util.gpu_cohort with chromosome_regions, per field,
# in the measure of spread(): as tests/test_genosmooth_cpu.py measures and prints it.  The GPU
# tolerance is 16 x these, the margin tests/test_gpu_support.py and freqinfo_util.TOL give two
# correct restatements: the device rescales and orders its products unlike either.
SPREAD = {"post": 7.66e-14, "n0": 1.03e-14, "n1": 6.49e-15, "n2": 1.56e-14, "het_prior": 3.29e-15,
          "ibd": 2.65e-15, "alt_ibd": 1.91e-14, "het": 2.57e-13, "r_het_prior": 2.35e-13,
          "non_ibd": 2.38e-13, "dosage": 3.26e-15}
TOL = {k: 16 * v for k, v in SPREAD.items()}
