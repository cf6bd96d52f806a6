"""Mean and covariance of (total length, number) of the long IBD tracts on the device
(nghmm_ibd_long_moments, include/nghmm.h) against brute-force enumeration and against yardstick B of
tests/long_moments_util.py (np.longdouble, the recursion of the header walked through chromosome
starts), which tests/test_long_moments_cpu.py checks against enumeration.

Tolerance.  The two yardsticks A (float64, the chain augmented by the run's first site, raw moments,
nothing subtracted) and B differ on the 20 x 5003 cohort, over all region sets and the thresholds
1, 2, 8, 80, 81, 400, 2000 sites / 0, 0.05, 0.5, 2, 10 Mb, by at most the figures of
long_moments_util.SPREAD (tests/test_long_moments_cpu.py measures and prints them) -- the spread of
two correct restatements, relative to max(|value|, 1).  The tolerance is 16 x the spread per unit and
field, the project's rule and margin; on the long chain it is 16 x what float64 costs recursion B
itself against np.longdouble (SPREAD_LONG).  Nothing in either comes from a device.  The yardstick
runs once on the emissions numpy makes of the likelihoods and the frequency, and is shared by the
tests."""
import ctypes as C
import os

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import count_util as cu
import expect_util as xu
import layout_util
import long_moments_util as mu
import longest_util as lu
import moments_util as mo
import sample_util as su
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# enumeration agrees with both restatements to a few 1e-14 (sums over 2^12 paths of moments up to
# 12^2); the device's emissions reach the host through a logarithm and go back through an
# exponential (1e-16 per site, twelve sites; second moments of at most 144)
ENUM_TOL = 1e-11
MODES = ["fast", "exact"]
UNITS = mu.UNITS
SMALL_SETS = {"whole": [[0, 12]], "chrom": [[0, 7], [7, 12]], "across": [[2, 10]]}


def _mode(pkg, mode):
    return pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT


def _handle(pkg, cohort, mode):
    d, gl, F, A, freq = cohort
    h = pkg.NgsFHMM(d.n_ind, d.n_sites, mode=_mode(pkg, mode))
    h.load(np.ascontiguousarray(gl), np.ascontiguousarray(d.pos_dist_mb))
    h.set_params(F, A, freq)
    h.init_emission()
    return h


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


@pytest.fixture(scope="module")
def handles(pkg, cohort):
    hs = {m: _handle(pkg, cohort, m) for m in MODES}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def cohort_want(pkg, cohort, handles):
    """Yardstick B on the cohort: the region sets for the lane length of the layout the device
    reports (both modes get the same sets), every threshold of COHORT_LEN."""
    d, gl, F, A, freq = cohort
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    T = handles["fast"].layout()[1]
    assert T > 0
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    assert set(sets) >= {"chrom", "win7", "win64", "win2048", "win2049", "edges", "gaps", "whole"}
    cells = lu.cells_b(e, d.pos_dist_mb, F, A)
    want = {(u, tag): mu.records_b(cells, d.pos_dist_mb, bu.COHORT_LEN[u], u, reg)
            for u in UNITS for tag, reg in sets.items()}
    return sets, want, cells


def _check(got, want, tol, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    for f in mu.FIELDS:
        assert np.isfinite(got[f]).all(), (tag, f)
    assert (got["var_a"] >= 0).all() and (got["var_t"] >= 0).all(), tag
    err = mu.rel_err(got, want)
    print(f"  {tag:22s}: error / tolerance " + ", ".join(f"{f} {err[f] / tol[f]:.3g}" for f in mu.FIELDS))
    assert mu.within(got, want, tol), (tag, err)


def _check_abs(got, want, atol, tag):
    worst = max(float(np.abs(got[f] - want[f]).max()) for f in mu.FIELDS)
    print(f"  {tag:22s}: largest |device - enumeration| = {worst:.3e} (tol {atol:.1e})")
    for f in mu.FIELDS:
        assert np.isfinite(got[f]).all() and (np.abs(got[f] - want[f]) <= atol).all(), (tag, f)


@pytest.mark.parametrize("mode", MODES)
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths, both units: the whole data (two chromosomes), the chromosomes,
    a region across the chromosome start and every single-site region, where at L = 1 site and at
    0 Mb mean_t is the posterior p = pi_s(1) and var_t = p (1 - p); an excluded state gives five
    exact zeros."""
    _, pos, F, A, _, gl, freq = xu.small_case()
    I, S = gl.shape[1], gl.shape[0]
    gl = np.where(np.isneginf(gl), -1e15, gl)          # (the reader's likelihood of an excluded genotype)
    one = xu.single_site_regions(S)
    with pkg.NgsFHMM(I, S, mode=_mode(pkg, mode)) as h:
        h.load(np.ascontiguousarray(gl), pos)
        h.set_params(F, A, freq)
        h.init_emission()
        e = h.e_prob
        e = np.where(e < -1e14, -np.inf, e)
        post = xu.terms_b(e, pos, F, A)["ibd"]
        print()
        for unit in UNITS:
            L = bu.SMALL_LEN[unit]
            got = h.ibd_long_moments(L, unit=unit)
            assert got.dtype == pkg.LONG_MOMENT_DTYPE and got.shape == (I, 1, len(L))
            for tag, reg in SMALL_SETS.items():
                _check_abs(h.ibd_long_moments(L, unit=unit, regions=np.array(reg)),
                           mu.enumerate_long_moments(e, pos, F, A, L, unit, reg), ENUM_TOL, f"{unit} {tag}")
            cells = h.ibd_long_moments(L, unit=unit, regions=one)
            _check_abs(cells, mu.enumerate_long_moments(e, pos, F, A, L, unit, one), ENUM_TOL, f"{unit} cells")
            assert np.abs(cells["mean_t"][:, :, 0] - post).max() <= ENUM_TOL
            assert np.abs(cells["var_t"][:, :, 0] - post * (1 - post)).max() <= ENUM_TOL
            for f in mu.FIELDS:
                assert (cells[f][1, 4] == 0.0).all(), (unit, f)


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_yardstick(handles, cohort_want, mode):
    """20 x 5003 against yardstick B within 16 x spread, both units, seven and five thresholds (K = 7
    and 5 in one call) and every threshold alone (K = 1) with the bytes it has in the full call, and
    K = 8: the chromosomes; windows of 7, 64, 2048 and 2049 sites; single sites on both sides of every
    lane-chunk edge; a region across a chromosome start among regions with gaps; the whole data.
    2000 sites exceed every chromosome: five exact zeros.  Means do not increase in k."""
    sets, want, cells = cohort_want
    h = handles[mode]
    print()
    for unit in UNITS:
        tol = mu.TOL[unit]
        L = bu.COHORT_LEN[unit]
        for tag in ("chrom", "win7", "win64", "win2048", "win2049", "edges", "gaps", "whole"):
            got = h.ibd_long_moments(L, unit=unit, regions=sets[tag])
            _check(got, want[unit, tag], tol, f"{unit} {tag}")
            if unit == "sites":
                for f in mu.FIELDS:
                    assert (got[f][:, :, -1] == 0.0).all(), (tag, f)
            for f in ("mean_a", "mean_t"):
                slack = tol[f] * np.maximum(np.abs(want[unit, tag][f][:, :, :-1]), 1.0)
                assert (np.diff(got[f], axis=2) <= 2 * slack).all(), (unit, tag, f)
        for tag in ("chrom", "gaps"):
            full = h.ibd_long_moments(L, unit=unit, regions=sets[tag])
            for k, l in enumerate(L):
                assert h.ibd_long_moments(l, unit=unit, regions=sets[tag]).tobytes() == \
                    np.ascontiguousarray(full[:, :, k:k + 1]).tobytes(), (unit, tag, l)
    # K = 8
    L8 = (1, 2, 8, 40, 80, 81, 400, 2000)
    got = h.ibd_long_moments(L8, regions=sets["chrom"])
    sel = [L8.index(l) for l in bu.COHORT_LEN["sites"]]
    assert got[:, :, sel].tobytes() == h.ibd_long_moments(bu.COHORT_LEN["sites"], regions=sets["chrom"]).tobytes()
    _check(np.ascontiguousarray(got[:, :, sel]), want["sites", "chrom"], mu.TOL["sites"], "sites chrom K = 8")


@pytest.fixture(scope="module")
def ragged(pkg):
    """70 x 301, 3 chromosomes, called genotypes (blocked steps): two waves, the second with 6 lanes;
    S % 4 == 1; parts whose length is no multiple of 8; windows of 7 sites cut runs at their edges."""
    I, S = 70, 301
    d = pkg.simulate.simulate(I, S, seed=5, n_chrom=3, indF=0.4, alpha=0.1)
    return d, I, S


@pytest.mark.parametrize("mode", MODES)
def test_small_ragged_shape(pkg, ragged, mode):
    """The ragged shape against yardstick B on the emissions the device made of the called
    genotypes (excluded states are -inf): the chromosomes, windows of 7 sites, the whole data."""
    d, I, S = ragged
    pos = d.pos_dist_mb
    with pkg.NgsFHMM(I, S, mode=_mode(pkg, mode) | pkg.GENO_PACKED) as h:
        h.load_raw(d.gl, pos, space=0, call_geno=True)
        h.set_params(0.4, 0.1, 0.2)
        h.init_emission()
        e = h.e_prob
        het = e[..., 1] < -1e14
        assert het.sum() > 50
        e = np.where(e < -1e14, -np.inf, e)
        cells = lu.cells_b(e, pos, 0.4, 0.1)
        assert np.isneginf(cells[2][:, ~xu.chrom_start(pos)]).any()         # blocked steps inside chromosomes
        sets = xu.region_sets(S, pos, 0)
        assert len(sets["chrom"]) == 3 and any((b - a) % 8 for a, b in sets["chrom"])
        print()
        for unit, L in (("sites", (1, 2, 5, 40)), ("mb", (0.0, 0.1, 1.0))):
            for tag in ("chrom", "win7", "whole"):
                got = h.ibd_long_moments(L, unit=unit, regions=sets[tag])
                _check(got, mu.records_b(cells, pos, L, unit, sets[tag]), mu.TOL[unit], f"{unit} {tag}")
            one = h.ibd_long_moments(L, unit=unit, regions=xu.single_site_regions(S))
            for f in mu.FIELDS:
                assert (one[f][het] == 0.0).all(), (unit, f)


@pytest.mark.parametrize("mode", MODES)
def test_identities(cohort, handles, cohort_want, mode):
    """Against the device's own calls, each within the sum of the two calls' tolerances.  L = 1 site
    and L = 0 Mb over whole chromosomes (and the whole data): all five fields are ibd_moments'.  Over
    whole chromosomes, every threshold: mean_t is ibd_by_length's tracts, mean_a its length.  On any
    region mean_t and var_t are the mean and variance of ibd_count's distribution at M = 16, at the
    thresholds for which yardstick B puts P(C >= 16) below the tolerance -- which leaves out no
    threshold of COHORT_LEN on windows of 64 sites and on the regions with gaps."""
    sets, want, cells = cohort_want
    h = handles[mode]
    print()
    for unit in UNITS:
        L = bu.COHORT_LEN[unit]
        tol = mu.TOL[unit]
        mine = lambda f, v: tol[f] * np.maximum(np.abs(v), 1.0)
        for tag in ("chrom", "whole"):
            got = h.ibd_long_moments(L[0], unit=unit, regions=sets[tag])[:, :, 0]
            ref = h.ibd_moments(sets[tag], length=unit)
            for f in mu.FIELDS:
                err = np.abs(got[f] - ref[f])
                print(f"  {unit} {tag} {f}: largest |long_moments - ibd_moments| = {err.max():.3e}")
                assert (err <= mine(f, ref[f]) + mo.COHORT_TOL[unit][f]).all(), (unit, tag, f, err.max())
        got = h.ibd_long_moments(L, unit=unit, regions=sets["chrom"])
        bl = h.ibd_by_length(L, unit=unit, regions=sets["chrom"])
        for f, g in (("mean_t", "tracts"), ("mean_a", "length")):
            err = np.abs(got[f] - bl[g])
            print(f"  {unit} chrom {f}: largest |long_moments - ibd_by_length.{g}| = {err.max():.3e}")
            assert (err <= mine(f, bl[g]) + bu.TOL[unit][g]).all(), (unit, f, err.max())
        for tag in ("win64", "gaps"):
            reg = sets[tag]
            top = cu.records_b(cells, cohort[0].pos_dist_mb, L, unit, reg, 16)[..., 16]
            keep = [k for k in range(len(L)) if top[:, :, k].max() < min(tol["mean_t"], tol["var_t"])]
            assert keep == list(range(len(L))), (unit, tag, keep)
            got = h.ibd_long_moments(L, unit=unit, regions=reg)
            p = h.ibd_count(L, unit=unit, regions=reg, max_count=16)
            c = np.arange(17.0)
            mean = (p * c).sum(axis=-1)
            var = (p * (c - mean[..., None]) ** 2).sum(axis=-1)
            # 17 probabilities within count_util's tolerance each, weighted by c and c^2
            cm, cv = cu.TOL[unit] * c.sum(), cu.TOL[unit] * (c ** 2).sum()
            for f, v, other in (("mean_t", mean, cm), ("var_t", var, cv)):
                err = np.abs(got[f] - v)
                print(f"  {unit} {tag} {f}: largest |long_moments - ibd_count| = {err.max():.3e}")
                assert (err <= mine(f, v) + other).all(), (unit, tag, f, err.max())


@pytest.fixture(scope="module")
def long_chain(pkg):
    case = mu.long_case(pkg)
    want = np.load(mu.GOLDEN_LONG)
    assert want.dtype == mu.DTYPE and want.shape == (2, 3, 1, 1)
    return case, want


def test_long_chain(pkg, long_chain):
    """3 x 50 000 on one chromosome, 50 sites and 0.5 Mb, fast mode, against B(np.longdouble) within
    TOL_LONG = 16 x what float64 costs the centred recursion.  (tests/golden holds B(np.longdouble),
    45 s of numpy a unit; tests/test_long_moments_cpu.py recomputes it and holds the file to it, and
    shows that the recursion WITHOUT the offsets misses this tolerance in var_t.)"""
    case, want = long_chain
    print()
    with _handle(pkg, case, "fast") as h:
        for n, unit in enumerate(UNITS):
            got = h.ibd_long_moments(mu.LONG_LEN[unit], unit=unit)
            _check(got, want[n], mu.TOL_LONG[unit], f"long chain {unit}")


@pytest.mark.parametrize("mode", MODES)
def test_against_the_sampler(handles, cohort, mode):
    """sample_paths(400, seed 77, keep all) on the cohort: path_long_moments of the kept paths at
    SAMPLER_LEN, both units, under long_moments_util.sampler_check: means within 5 standard errors
    per individual and for the cohort at every threshold, sample variances within
    5 sqrt((m4 - s^4) / R) at SAMPLER_VAR_LEN (all but 10 Mb: long_moments_util says why)."""
    d = cohort[0]
    h = handles[mode]
    assert mu.SAMPLER_DRAWS == xu.SAMPLER_DRAWS == 400 and xu.SAMPLER_SEED == 77
    _, paths = h.sample_paths(mu.SAMPLER_DRAWS, seed=xu.SAMPLER_SEED, keep=mu.SAMPLER_DRAWS)
    assert paths.shape == (mu.SAMPLER_DRAWS, d.n_ind, d.n_sites)
    print()
    for u in UNITS:
        exact = h.ibd_long_moments(bu.SAMPLER_LEN[u], unit=u)[:, 0]
        A, Cn = mu.path_long_moments(paths, d.pos_dist_mb, u, bu.SAMPLER_LEN[u])
        worst = mu.sampler_check(A, Cn, exact, mu.sampler_var_k(u), u)
        print(f"  device sampler against the moments in {u}: largest |z| = {worst:.2f}")


@pytest.mark.parametrize("mode", MODES)
def test_same_bits_and_nothing_else_moves(pkg, cohort, mode):
    """The same arguments give the same bits; a region's record does not depend on the other
    regions; parameters, posteriors, tracts and the next EM iteration are bit-identical with and
    without the call; ibd_longest and ibd_count, whose scratch the call shares, give the same bytes
    before and after."""
    d = cohort[0]
    regions = pkg.window_regions(d.pos_dist_mb, 777)

    def run(with_call):
        out = {}
        with _handle(pkg, cohort, mode) as h:
            h.iter_EM(1)
            h.viterbi()
            out["before"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ibd_tracts("viterbi"))
            if with_call:
                for unit in UNITS:
                    L = bu.COHORT_LEN[unit]
                    lg, ct = h.ibd_longest(L, unit, regions), h.ibd_count(L, unit, regions, 5)
                    a, b = h.ibd_long_moments(L, unit, regions), h.ibd_long_moments(L, unit, regions)
                    assert a.tobytes() == b.tobytes()
                    assert h.ibd_longest(L, unit, regions).tobytes() == lg.tobytes()
                    assert h.ibd_count(L, unit, regions, 5).tobytes() == ct.tobytes()
                    h.ibd_long_moments(L, unit)
                    assert h.ibd_long_moments(L, unit, regions).tobytes() == a.tobytes()
                    for g in range(len(regions)):
                        assert h.ibd_long_moments(L, unit, regions[g:g + 1]).tobytes() == \
                            np.ascontiguousarray(a[:, g:g + 1]).tobytes()
            out["params"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ibd_tracts("viterbi"))
            h.iter_EM(1)
            out["after"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ind_lkl.copy())
        return out

    a, b = run(False), run(True)
    for k in ("before", "params", "after"):
        for x, y in zip(a[k], b[k]):
            assert x.tobytes() == y.tobytes(), k
    for x, y in zip(b["before"], b["params"]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("fast_c", [1, 2, 3, 4])
def test_same_bytes_across_forced_layouts(pkg, cohort, handles, cohort_want, fast_c):
    """Fast mode under the forced lane layouts of tests/test_gpu_layouts.py (1 to 4 waves per
    individual; the cohort's own layout has 5): the walk is one lane per individual and chromosome
    over site-major planes, so the bytes are the default layout's."""
    sets = cohort_want[0]
    href = handles["fast"]
    with layout_util.handle(pkg, cohort, False, fast_c) as h:
        (C_, T), (C0, T0) = h.layout(), href.layout()
        assert C_ == fast_c and C0 != fast_c and T != T0
        for unit in UNITS:
            for tag in ("chrom", "gaps", "win7"):
                assert h.ibd_long_moments(bu.COHORT_LEN[unit], unit, sets[tag]).tobytes() == \
                    href.ibd_long_moments(bu.COHORT_LEN[unit], unit, sets[tag]).tobytes(), (unit, tag)


def _raw(h, what, lengths, begin, end, stats=True, n=None, k=None, null_len=False, null_begin=False):
    u64 = C.POINTER(C.c_uint64)
    b, e = np.array(begin, dtype=np.uint64), np.array(end, dtype=np.uint64)
    L = np.array(lengths, dtype=np.float64)
    n = len(b) if n is None else n
    k = len(L) if k is None else k
    buf = np.zeros(h.n_ind * max(n, 1) * max(k, 1) * 5)
    rc = h.lib.nghmm_ibd_long_moments(h.handle, what, k,
                                      None if null_len or not len(L) else L.ctypes.data_as(C.POINTER(C.c_double)), n,
                                      None if null_begin or not len(b) else b.ctypes.data_as(u64),
                                      None if not len(e) else e.ctypes.data_as(u64),
                                      C.c_void_p(buf.ctypes.data) if stats else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg):
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=3, n_chrom=2)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, 0, [1], [0], [S])                     # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_long_moments(1)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        assert _raw(h, 0, [1, 5], [0], [S])[0] == 0 and _raw(h, 1, [0, 0.5], [0], [S])[0] == 0
        assert _raw(h, 0, list(range(1, 9)), [0], [S])[0] == 0
        # a whole number of sites beyond any integer type: no window, no long run at all
        far = h.ibd_long_moments((1, 1e30))
        for f in mu.FIELDS:
            assert (far[f][..., 1] == 0.0).all()
        inf, nan = float("inf"), float("nan")
        bad = [
            ((2, [1], [0], [S]), {}),                           # an unknown bit
            ((1 | 4, [1], [0], [S]), {}),
            ((0, [], [0], [S]), {"k": 0}),                      # no thresholds, too many
            ((0, list(range(1, 10)), [0], [S]), {}),
            ((0, [1], [0], [S]), {"null_len": True}),
            ((0, [2, 1], [0], [S]), {}),                        # unsorted, repeated
            ((0, [2, 2], [0], [S]), {}),
            ((1, [0.5, 0.5], [0], [S]), {}),
            ((0, [1, inf], [0], [S]), {}),                      # not finite
            ((1, [nan], [0], [S]), {}),
            ((1, [-0.5, 1], [0], [S]), {}),                     # negative
            ((0, [1.5], [0], [S]), {}),                         # sites: not whole, below 1
            ((0, [0, 1], [0], [S]), {}),
            ((0, [1], [], []), {"n": 0}),                       # n_regions == 0
            ((0, [1], [0], [S]), {"stats": False}),             # a NULL pointer
            ((0, [1], [0], [S]), {"null_begin": True}),
            ((0, [1], [10, 5], [20, 8]), {}),                   # unsorted regions
            ((0, [1], [0, 9], [10, 20]), {}),                   # overlapping
            ((0, [1], [0, 10], [10, 10]), {}),                  # empty
            ((0, [1], [0], [S + 1]), {}),                       # end > S
        ]
        for args, kw in bad:
            rc, msg = _raw(h, *args, **kw)
            assert rc == -10 and msg, (args, kw, rc, msg)
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_long_moments(1, unit="cm")
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_long_moments(1, regions=np.array([[0.0, 5.0]]))
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_long_moments((3, 2))
        assert ei.value.code == -10 and "increasing" in ei.value.message


@pytest.mark.parametrize("mode", MODES)
def test_cli_ibd_long_moments(pkg, tmp_path, mode):
    """ngsF-HMM --ibd_long_moments at 6 x 400, two chromosomes, all parameters fixed (so the binding
    can be put at the run's final parameters exactly): the file parses and matches ibd_long_moments
    to the %.10g printed, in Mb and with --long_moments_sites --long_moments_window 50; without the
    flag the set of output files and their bytes are those of a run without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", mode]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_long_moments", "0,0.5,2"])
    cli_util.run_cli(base + ["--out", w, "--ibd_long_moments", "1,5,40", "--long_moments_sites",
                             "--long_moments_window", 50])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.long.moments"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    with pkg.NgsFHMM(I, S, mode=_mode(pkg, mode)) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        for out, window, unit, L in ((a, 0, "mb", (0, 0.5, 2)), (w, 50, "sites", (1, 5, 40))):
            regions = summary_util.chrom_regions(chrom, window)
            got = h.ibd_long_moments(L, unit=unit, regions=regions)
            sd = pkg.long_moment_sd(got)
            lines = open(out + ".ibd.long.moments").read().split("\n")
            assert lines[0] == "\t".join(["ind", "chr", "first_pos", "last_pos", "n_sites", "min_len", "exp_len",
                                          "sd_len", "exp_tracts", "sd_tracts", "corr"])
            assert lines[-1] == "" and len(lines) == 2 + I * len(regions) * len(L)
            assert len(regions) == (2 if not window else 8)
            n = 1
            for i in range(I):
                for r, (lo, hi) in enumerate(regions):
                    for k, l in enumerate(L):
                        f = lines[n].split("\t")
                        n += 1
                        assert f[:6] == [f"ind{i}", chrom[lo], str(pos[lo]), str(pos[hi - 1]), str(int(hi - lo)),
                                         "%.10g" % l]
                        assert len(f) == 11
                        vals = (got["mean_a"][i, r, k], sd["sd_a"][i, r, k], got["mean_t"][i, r, k],
                                sd["sd_t"][i, r, k], sd["corr"][i, r, k])
                        for text, v in zip(f[6:], vals):
                            if np.isnan(v):
                                assert text == "NA"
                                continue
                            assert text == "%.10g" % float(text)
                            assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[n - 1], v)
