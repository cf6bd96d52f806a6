"""The distribution of the number of long IBD tracts on the device (nghmm_ibd_count,
include/nghmm.h) against brute-force enumeration and against yardstick B of tests/count_util.py
(np.longdouble, the recursion of the header walked through chromosome starts), which
tests/test_count_cpu.py checks against enumeration.

Tolerance.  The two yardsticks A (float64, the chain augmented by count level and the run's first
site: running products, nothing subtracted) and B differ on the 20 x 5003 cohort, over all region
sets, the thresholds 1, 2, 8, 80, 81, 400, 2000 sites / 0, 0.05, 0.5, 2, 10 Mb and 16 count levels,
by at most the figures of count_util.SPREAD (tests/test_count_cpu.py measures and prints them) --
the spread of two correct restatements.  The tolerance is 16 x the spread per unit, the project's
rule and margin; nothing in it comes from a device.  The yardstick runs once on the emissions numpy
makes of the likelihoods and the frequency, and is shared by the tests."""
import ctypes as C
import os

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import count_util as cu
import expect_util as xu
import longest_util as lu
import sample_util as su
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# tests/test_gpu_longest.py's ENUM_TOL and its reason: enumeration agrees with both restatements to
# a few 1e-15; the device's emissions reach the host through a logarithm and go back through an
# exponential (1e-16 per site, twelve sites; probabilities)
ENUM_TOL = 1e-12
MODES = ["fast", "exact"]
UNITS = ("sites", "mb")
M_MAX = 16
SMALL_SETS = {"whole": [[0, 12]], "chrom": [[0, 7], [7, 12]], "across": [[2, 10]]}


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


def _handle(pkg, cohort, mode):
    d, gl, F, A, freq = cohort
    h = pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT)
    h.load(np.ascontiguousarray(gl), np.ascontiguousarray(d.pos_dist_mb))
    h.set_params(F, A, freq)
    h.init_emission()
    return h


@pytest.fixture(scope="module")
def cohort_want(pkg, cohort):
    """Yardstick B on the cohort at M = 16: the region sets for the lane length of the layout the
    device reports (both modes get the same sets)."""
    d, gl, F, A, freq = cohort
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    with _handle(pkg, cohort, "fast") as h:
        T = h.layout()[1]
    assert T > 0
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    assert set(sets) >= {"chrom", "win7", "win64", "win2048", "win2049", "edges", "gaps", "whole"}
    cells = lu.cells_b(e, d.pos_dist_mb, F, A)
    want = {(u, tag): cu.records_b(cells, d.pos_dist_mb, bu.COHORT_LEN[u], u, reg, M_MAX)
            for u in UNITS for tag, reg in sets.items()}
    return sets, want


def _check(got, want, tol, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), tag
    err = np.abs(got - want)
    print(f"  {tag:20s}: largest |device - yardstick| = {err.max():.3e} (tol {tol:.3e})")
    assert (err <= tol).all(), (tag, err.max())


@pytest.mark.parametrize("mode", MODES)
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths at M = 3, both units: the whole data (two chromosomes), the
    chromosomes, a region across the chromosome start and every single-site region, where prob[1]
    at L = 1 site and at 0 Mb is the posterior pi_s(1); an excluded state (exact zeros); one
    threshold alone gives the same bytes; prob[..., :2] at M = 3 against M = 2."""
    _, pos, F, A, _, gl, freq = xu.small_case()
    I, S = gl.shape[1], gl.shape[0]
    gl = np.where(np.isneginf(gl), -1e15, gl)          # (the reader's likelihood of an excluded genotype)
    m = pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT
    one = xu.single_site_regions(S)
    M = 3
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load(np.ascontiguousarray(gl), pos)
        h.set_params(F, A, freq)
        h.init_emission()
        e = h.e_prob
        assert np.isneginf(e[1, 4, 1]) or e[1, 4, 1] < -1e14
        e = np.where(e < -1e14, -np.inf, e)
        post = xu.terms_b(e, pos, F, A)["ibd"]
        print()
        for unit in UNITS:
            L = bu.SMALL_LEN[unit]
            got = h.ibd_count(L, unit=unit, max_count=M)
            assert got.dtype == np.float64 and got.shape == (I, 1, len(L), M + 1)
            assert got.tobytes() == h.ibd_count(L, unit=unit, regions=np.array([[0, S]]), max_count=M).tobytes()
            for tag, reg in SMALL_SETS.items():
                _check(h.ibd_count(L, unit=unit, regions=np.array(reg), max_count=M),
                       cu.enumerate_count(e, pos, F, A, L, unit, reg, M), ENUM_TOL, f"{unit} {tag}")
            cells = h.ibd_count(L, unit=unit, regions=one, max_count=M)
            _check(cells, cu.enumerate_count(e, pos, F, A, L, unit, one, M), ENUM_TOL, f"{unit} cells")
            assert np.abs(cells[:, :, 0, 1] - post).max() <= ENUM_TOL
            assert (cells[..., 2:] == 0.0).all()                      # one site: at most one run
            assert (cells[1, 4, :, 1:] == 0.0).all() and (cells[1, 4, :, 0] == 1.0).all()
            for k, l in enumerate(L):      # one threshold alone is the same record
                assert h.ibd_count(l, unit=unit, max_count=M).tobytes() == \
                    np.ascontiguousarray(got[:, :, k:k + 1]).tobytes()
            for tag, reg in SMALL_SETS.items():
                a3 = h.ibd_count(L, unit=unit, regions=np.array(reg), max_count=3)
                a2 = h.ibd_count(L, unit=unit, regions=np.array(reg), max_count=2)
                same = a3[..., :2].tobytes() == a2[..., :2].tobytes()
                err = np.abs(a3[..., :2] - a2[..., :2]).max()
                print(f"  {unit} {tag}: prob[:2] at M = 3 against M = 2: "
                      f"{'the same bytes' if same else f'largest difference {err:.3e}'}")
                assert err <= cu.TOL[unit]


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_yardstick(pkg, cohort, cohort_want, mode):
    """20 x 5003 against yardstick B within 16 x spread at M = 16, both units, seven and five
    thresholds: the chromosomes; windows of 7, 64, 2048 and 2049 sites; single sites on both sides
    of every lane-chunk edge; a region across a chromosome start among regions with gaps; the whole
    data.  The sum over c is within (M + 1) x the tolerance of 1; 2000 sites exceed every
    chromosome: prob[0] == 1 exactly."""
    sets, want = cohort_want
    with _handle(pkg, cohort, mode) as h:
        print()
        for unit in UNITS:
            tol = cu.TOL[unit]
            for tag in ("chrom", "win7", "win64", "win2048", "win2049", "edges", "gaps", "whole"):
                got = h.ibd_count(bu.COHORT_LEN[unit], unit=unit, regions=sets[tag], max_count=M_MAX)
                _check(got, want[unit, tag], tol, f"{unit} {tag}")
                assert (got >= 0).all()
                one = np.abs(got.sum(axis=-1) - 1).max()
                print(f"  {unit} {tag}: largest |sum - 1| = {one:.3e}")
                assert one <= (M_MAX + 1) * tol
                if unit == "sites":
                    assert (got[:, :, -1, 0] == 1.0).all() and (got[:, :, -1, 1:] == 0.0).all()


@pytest.mark.parametrize("mode", MODES)
def test_two_waves_the_second_ragged(pkg, mode):
    """gpu_cohort at 70 x 700: two waves of individuals, the second with 6 lanes; the chromosomes
    and windows of 64 sites at M = 4 against yardstick B."""
    coh = sup.gpu_cohort(pkg, 70, 700)
    d, gl, F, A, freq = coh
    pos = d.pos_dist_mb
    cells = lu.cells_b(su.emissions_np(gl, np.full(d.n_sites, freq)), pos, F, A)
    with _handle(pkg, coh, mode) as h:
        sets = xu.region_sets(d.n_sites, pos, h.layout()[1] or xu.SPREAD_LANE_SITES)
        print()
        for unit in UNITS:
            for tag in ("chrom", "win64"):
                got = h.ibd_count(bu.COHORT_LEN[unit], unit=unit, regions=sets[tag], max_count=4)
                _check(got, cu.records_b(cells, pos, bu.COHORT_LEN[unit], unit, sets[tag], 4), cu.TOL[unit],
                       f"{unit} {tag}")


@pytest.mark.parametrize("mode", MODES)
def test_identities(pkg, cohort, cohort_want, mode):
    """Against the device's own calls.  M = 1 is ibd_longest (within the two tolerances; the bytes
    are expected and which is printed).  Over whole chromosomes mean_lower is at most
    ibd_by_length's expected number of tracts, always, and equal to it on the (individual,
    chromosome) records that yardstick B says have P(C >= 16) <= 1e-13 -- every record at 400 sites
    and at least 90 % at 80 and 81 (tests/test_count_cpu.py establishes that on the yardstick);
    thresholds of at most 8 sites are left out of the equality.  Every prob[c] >= 0 and the tail
    sum over j >= c is non-increasing in k."""
    sets, want = cohort_want
    d = cohort[0]
    with _handle(pkg, cohort, mode) as h:
        print()
        for unit in UNITS:
            L = bu.COHORT_LEN[unit]
            tol = cu.TOL[unit]
            for tag in ("whole", "chrom", "win64", "gaps", "edges"):
                reg = sets[tag]
                c1 = h.ibd_count(L, unit=unit, regions=reg, max_count=1)
                lg = h.ibd_longest(L, unit=unit, regions=reg)
                same = c1[..., 0].tobytes() == lg["p_none"].tobytes() and c1[..., 1].tobytes() == lg["p_any"].tobytes()
                err = max(np.abs(c1[..., 0] - lg["p_none"]).max(), np.abs(c1[..., 1] - lg["p_any"]).max())
                print(f"  {unit} {tag}: M = 1 against ibd_longest: "
                      f"{'the same bytes' if same else f'largest difference {err:.3e}'}")
                assert np.abs(c1[..., 0] - lg["p_none"]).max() <= tol + lu.TOL[unit]["p_none"]
                assert np.abs(c1[..., 1] - lg["p_any"]).max() <= tol + lu.TOL[unit]["p_any"]
                got = h.ibd_count(L, unit=unit, regions=reg, max_count=M_MAX)
                assert (got >= 0).all()
                tail = np.cumsum(got[..., ::-1], axis=-1)[..., ::-1][..., 1:]      # P(C_k >= c), c = 1 .. M
                assert (np.diff(tail, axis=2) <= (M_MAX + 1) * tol).all(), (unit, tag)
            got = h.ibd_count(L, unit=unit, regions=sets["chrom"], max_count=M_MAX)
            mean = pkg.count_summary(got)["mean_lower"]
            tr = h.ibd_by_length(L, unit=unit, regions=sets["chrom"])["tracts"]
            both = tol + bu.TOL[unit]["tracts"]
            assert (mean <= tr + both).all(), (unit, (mean - tr).max())
            sel = want[unit, "chrom"][..., M_MAX] <= 1e-13                        # by the yardstick
            for k, l in enumerate(L):
                if unit == "sites" and l <= 8:
                    continue
                share = sel[:, :, k].mean()
                err = np.abs(mean - tr)[:, :, k][sel[:, :, k]]
                print(f"  {unit} L = {l}: {100 * share:.0f} % of {sel[:, :, k].size} records qualify; "
                      f"largest |mean_lower - tracts| = {err.max() if err.size else 0.0:.3e} (tol {both:.3e})")
                if unit == "sites" and l in (80, 81):
                    assert share >= 0.9
                if unit == "sites" and l == 400:
                    assert share == 1.0
                assert (err <= both).all(), (unit, l, err.max())


@pytest.mark.parametrize("mode", MODES)
def test_against_the_sampler(pkg, cohort, mode):
    """sample_paths(400, seed 77, keep all) on the cohort: path_count of the kept paths at
    SAMPLER_LEN, both units, against prob at M = 4 under count_util.sampler_check: every threshold,
    every probability, every individual."""
    d = cohort[0]
    with _handle(pkg, cohort, mode) as h:
        _, paths = h.sample_paths(xu.SAMPLER_DRAWS, seed=xu.SAMPLER_SEED, keep=xu.SAMPLER_DRAWS)
        exact = {u: h.ibd_count(bu.SAMPLER_LEN[u], unit=u, max_count=4)[:, 0] for u in UNITS}
    assert xu.SAMPLER_DRAWS == 400 and xu.SAMPLER_SEED == 77
    assert paths.shape == (xu.SAMPLER_DRAWS, d.n_ind, d.n_sites)
    print()
    for u in UNITS:
        counts = cu.path_count(paths, d.pos_dist_mb, u, bu.SAMPLER_LEN[u])
        worst = cu.sampler_check(counts, exact[u], bu.SAMPLER_LEN[u], u)
        print(f"  device sampler against prob in {u}: largest |z| = {worst:.2f}")


@pytest.mark.parametrize("mode", MODES)
def test_packed_called_genotypes(pkg, mode):
    """8 x 300 called genotypes as 2-bit codes: everything finite; a one-site region on a called
    heterozygote (the IBD state is excluded) has prob[0] == 1."""
    I, S = 8, 300
    d = pkg.simulate.simulate(I, S, seed=5, n_chrom=2, indF=0.4, alpha=0.1)
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | pkg.GENO_PACKED
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=True)
        h.set_params(0.4, 0.1, 0.2)
        h.init_emission()
        het = h.e_prob[..., 1] < -1e14
        assert het.sum() > 50
        for unit, L in (("sites", (1, 2, 5, 40)), ("mb", (0.0, 0.1, 1.0))):
            one = h.ibd_count(L, unit=unit, regions=xu.single_site_regions(S), max_count=3)
            whole = h.ibd_count(L, unit=unit, max_count=3)
            assert np.isfinite(one).all() and np.isfinite(whole).all(), unit
            assert (one[het][..., 0] == 1.0).all() and (one[het][..., 1:] == 0.0).all()
            assert (one[~het][:, 0, 1] > 0.0).any()
            np.testing.assert_allclose(whole.sum(axis=-1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", MODES)
def test_same_bits_and_nothing_else_moves(pkg, cohort, mode):
    """The same arguments give the same bits; a region's record does not depend on the other
    regions; parameters, posteriors, tracts and the next EM iteration are bit-identical with and
    without the call; ibd_longest, whose plane scratch the call shares, gives the same bytes before
    and after."""
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
                    lg = h.ibd_longest(L, unit, regions)
                    a, b = h.ibd_count(L, unit, regions, 5), h.ibd_count(L, unit, regions, 5)
                    assert a.tobytes() == b.tobytes()
                    assert h.ibd_longest(L, unit, regions).tobytes() == lg.tobytes()
                    h.ibd_count(L, unit, max_count=16)
                    assert h.ibd_count(L, unit, regions, 5).tobytes() == a.tobytes()
                    # a region's record does not depend on which other regions are asked for
                    assert h.ibd_count(L, unit, regions[2:3], 5).tobytes() == \
                        np.ascontiguousarray(a[:, 2:3]).tobytes()
                    assert h.ibd_longest(L, unit, regions).tobytes() == lg.tobytes()
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


def _raw(h, what, lengths, begin, end, m=4, prob=True, n=None, k=None, null_len=False, null_begin=False):
    u64 = C.POINTER(C.c_uint64)
    b, e = np.array(begin, dtype=np.uint64), np.array(end, dtype=np.uint64)
    L = np.array(lengths, dtype=np.float64)
    n = len(b) if n is None else n
    k = len(L) if k is None else k
    buf = np.zeros(h.n_ind * max(n, 1) * max(k, 1) * (min(max(m, 1), 32) + 1))
    rc = h.lib.nghmm_ibd_count(h.handle, what, k,
                               None if null_len or not len(L) else L.ctypes.data_as(C.POINTER(C.c_double)), m, n,
                               None if null_begin or not len(b) else b.ctypes.data_as(u64),
                               None if not len(e) else e.ctypes.data_as(u64),
                               buf.ctypes.data_as(C.POINTER(C.c_double)) if prob else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg):
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=3, n_chrom=2)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, 0, [1], [0], [S])                     # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_count(1)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        assert _raw(h, 0, [1, 5], [0], [S])[0] == 0 and _raw(h, 1, [0, 0.5], [0], [S])[0] == 0
        assert _raw(h, 0, list(range(1, 9)), [0], [S])[0] == 0
        assert _raw(h, 0, [1], [0], [S], m=1)[0] == 0 and _raw(h, 0, [1], [0], [S], m=16)[0] == 0
        # a whole number of sites beyond any integer type: no window, no long run at all
        far = h.ibd_count((1, 1e30))
        assert (far[..., 1, 0] == 1.0).all() and (far[..., 1, 1:] == 0.0).all()
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
            ((0, [1], [0], [S]), {"prob": False}),              # a NULL pointer
            ((0, [1], [0], [S]), {"null_begin": True}),
            ((0, [1], [10, 5], [20, 8]), {}),                   # unsorted regions
            ((0, [1], [0, 9], [10, 20]), {}),                   # overlapping
            ((0, [1], [0, 10], [10, 10]), {}),                  # empty
            ((0, [1], [0], [S + 1]), {}),                       # end > S
            ((0, [1], [0], [S]), {"m": 0}),                     # n_counts outside 1..16
            ((0, [1], [0], [S]), {"m": 17}),
        ]
        for args, kw in bad:
            rc, msg = _raw(h, *args, **kw)
            assert rc == -10 and msg, (args, kw, rc, msg)
        assert "n_counts" in _raw(h, 0, [1], [0], [S], m=17)[1]
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_count(1, unit="cm")
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_count(1, regions=np.array([[0.0, 5.0]]))
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_count(1, max_count=0)
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_count(1, max_count=2.5)
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_count((3, 2))
        assert ei.value.code == -10 and "increasing" in ei.value.message


@pytest.mark.parametrize("mode", MODES)
def test_cli_ibd_count(pkg, tmp_path, mode):
    """ngsF-HMM --ibd_count at 6 x 400, two chromosomes, all parameters fixed (so the binding can be
    put at the run's final parameters exactly): the file parses and matches ibd_count to the %.10g
    printed, in Mb and with --count_sites --count_window 50 --count_max 3; without the flag the set
    of output files and their bytes are those of a run without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", mode]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_count", "0,0.5,2"])
    cli_util.run_cli(base + ["--out", w, "--ibd_count", "1,5,40", "--count_sites", "--count_window", 50,
                             "--count_max", 3])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.count"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        for out, window, unit, L, M in ((a, 0, "mb", (0, 0.5, 2), 8), (w, 50, "sites", (1, 5, 40), 3)):
            regions = summary_util.chrom_regions(chrom, window)
            got = h.ibd_count(L, unit=unit, regions=regions, max_count=M)
            lines = open(out + ".ibd.count").read().split("\n")
            assert lines[0] == "\t".join(["ind", "chr", "first_pos", "last_pos", "n_sites", "min_len"] +
                                         [f"p_{c}" for c in range(M)] + [f"p_ge_{M}"])
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
                        assert len(f) == 6 + M + 1
                        for text, v in zip(f[6:], got[i, r, k]):
                            assert text == "%.10g" % float(text)
                            assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[n - 1], v)
