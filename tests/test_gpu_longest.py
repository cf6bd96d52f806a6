"""The distribution of the longest IBD tract on the device (nghmm_ibd_longest /
nghmm_chain_ibd_longest, include/nghmm.h) against brute-force enumeration and against yardstick B
of tests/longest_util.py (np.longdouble, the recursion of the header walked through chromosome
starts), which tests/test_longest_cpu.py checks against enumeration.

Tolerance.  The two yardsticks A (float64, the chain augmented by the run's first site: running
products, nothing subtracted) and B differ on the 20 x 5003 cohort, over all region sets and the
thresholds 1, 2, 8, 80, 81, 400, 2000 sites / 0, 0.05, 0.5, 2, 10 Mb, by at most the figures of
longest_util.SPREAD (tests/test_longest_cpu.py measures and prints them) -- the spread of two
correct restatements.  The tolerance is 16 x the spread per unit and field, the project's rule and
margin; nothing in it comes from a device.  The yardstick runs once on the emissions numpy makes
of the likelihoods and the frequency, and is shared by the tests."""
import ctypes as C
import os

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import expect_util as xu
import longest_util as lu
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# Enumeration over 2^12 paths in float64 agrees with both restatements to 5e-16
# (tests/test_longest_cpu.py); the device's emissions reach the host through a logarithm and go
# back through an exponential (1e-16 per site, twelve sites; probabilities): 1e-12, as
# tests/test_gpu_bylength.py.
ENUM_TOL = 1e-12
MODES = ["fast", "exact"]
UNITS = ("sites", "mb")


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


def _handle(pkg, cohort, mode, sites=None):
    d, gl, F, A, freq = cohort
    lo, hi = sites or (0, d.n_sites)
    h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT)
    h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
    h.set_params(F, A, freq)
    h.init_emission()
    return h


@pytest.fixture(scope="module")
def cohort_want(pkg, cohort):
    """Yardstick B on the cohort: the region sets for the lane length of the layout the device
    reports (both modes get the same sets), yardstick B's cells, and the per-site posterior of the
    IBD state."""
    import sample_util as su
    d, gl, F, A, freq = cohort
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    with _handle(pkg, cohort, "fast") as h:
        T = h.layout()[1]
    assert T > 0
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    cells = lu.cells_b(e, d.pos_dist_mb, F, A)
    want = {(u, tag): lu.records_b(cells, d.pos_dist_mb, bu.COHORT_LEN[u], u, reg)
            for u in UNITS for tag, reg in sets.items()}
    return sets, want, np.asarray(cells[0][..., 1], dtype=np.float64)


def _check(got, want, tol, tag):
    for f in lu.FIELDS:
        assert np.isfinite(got[f]).all(), (tag, f)
        err = np.abs(got[f] - want[f])
        t = tol[f] if isinstance(tol, dict) else tol
        print(f"  {tag:16s} {f:7s}: largest |device - yardstick| = {err.max():.3e} (tol {t:.3e})")
        assert (err <= t).all(), (tag, f, err.max())


@pytest.mark.parametrize("mode", MODES)
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths, both units: the whole data (two chromosomes) and every
    single-site region, where p_any at L = 1 site and at 0 Mb is the posterior pi_s(1); a missing
    cell, an excluded state (exact zeros); one threshold alone gives the same bytes."""
    _, pos, F, A, _, gl, freq = xu.small_case()
    I, S = gl.shape[1], gl.shape[0]
    gl = np.where(np.isneginf(gl), -1e15, gl)          # (the reader's likelihood of an excluded genotype)
    m = pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT
    one = xu.single_site_regions(S)
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
            got = h.ibd_longest(L, unit=unit)
            assert got.dtype == pkg.LONGEST_DTYPE and got.shape == (I, 1, len(L))
            _check(got, lu.enumerate_longest(e, pos, F, A, L, unit, [[0, S]]), ENUM_TOL, f"{unit} whole")
            assert got.tobytes() == h.ibd_longest(L, unit=unit, regions=np.array([[0, S]])).tobytes()
            for tag, reg in (("chrom", [[0, 7], [7, S]]), ("across", [[2, 10]]), ("inside", [[1, 6], [8, 11]])):
                _check(h.ibd_longest(L, unit=unit, regions=np.array(reg)),
                       lu.enumerate_longest(e, pos, F, A, L, unit, reg), ENUM_TOL, f"{unit} {tag}")
            cells = h.ibd_longest(L, unit=unit, regions=one)
            _check(cells, lu.enumerate_longest(e, pos, F, A, L, unit, one), ENUM_TOL, f"{unit} cells")
            assert np.abs(cells["p_any"][..., 0] - post).max() <= ENUM_TOL
            assert (cells["p_any"][1, 4] == 0.0).all()
            for k, l in enumerate(L):      # one threshold alone is the same record
                assert h.ibd_longest(l, unit=unit).tobytes() == got[:, :, k:k + 1].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_yardstick(pkg, cohort, cohort_want, mode):
    """20 x 5003 against yardstick B within 16 x spread, both units, seven and five thresholds
    (2000 sites exceed every chromosome: p_any exactly 0): the chromosomes; windows of 7, 64, 2048
    and 2049 sites; single sites on both sides of every lane-chunk edge; a region across a
    chromosome start among regions with gaps; the whole data.  p_any + p_none = 1 within the two
    tolerances."""
    sets, want, _ = cohort_want
    with _handle(pkg, cohort, mode) as h:
        print()
        for unit in UNITS:
            tol = lu.TOL[unit]
            for tag, reg in sets.items():
                got = h.ibd_longest(bu.COHORT_LEN[unit], unit=unit, regions=reg)
                _check(got, want[unit, tag], tol, f"{unit} {tag}")
                if unit == "sites":
                    assert (got["p_any"][..., -1] == 0).all()
                one = np.abs(got["p_any"] + got["p_none"] - 1).max()
                print(f"  {unit} {tag}: largest |p_any + p_none - 1| = {one:.3e}")
                assert one <= tol["p_any"] + tol["p_none"]


@pytest.mark.parametrize("mode", MODES)
def test_identities(pkg, cohort, mode):
    """Against the device's own calls: at L = 1 site p_none is exp(log_p_non) of tract_support on
    the region as a range; over whole chromosomes p_any is at most ibd_by_length's expected number
    of tracts (Markov's inequality; inside a chromosome the two count different things -- a run is
    cut at the region's edges, a tract belongs with its whole length to the region it begins in --
    and neither bounds the other); p_any is non-increasing in k; longest_classes sums to 1."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    with _handle(pkg, cohort, mode) as h:
        sets = xu.region_sets(S, pos, h.layout()[1] or xu.SPREAD_LANE_SITES)
        print()
        for tag in ("whole", "chrom", "win64", "gaps", "edges"):
            reg = sets[tag]
            for unit in UNITS:
                L = bu.COHORT_LEN[unit]
                tol = lu.TOL[unit]
                got = h.ibd_longest(L, unit=unit, regions=reg)
                if tag in ("whole", "chrom"):      # (whole chromosomes: a run is a tract)
                    tr = h.ibd_by_length(L, unit=unit, regions=reg)["tracts"]
                    assert (got["p_any"] <= tr + tol["p_any"] + bu.TOL[unit]["tracts"]).all(), (unit, tag)
                assert (np.diff(got["p_any"], axis=-1) <= 2 * tol["p_any"]).all(), (unit, tag)
                assert (got["p_any"] >= 0).all() and (got["p_none"] >= 0).all()
                cls = pkg.longest_classes(got)
                assert np.abs(cls.sum(axis=-1) - 1).max() <= tol["p_any"] + tol["p_none"]
                assert (cls >= -2 * tol["p_any"]).all()
            got = h.ibd_longest(1, regions=reg)
            rng = np.array([(i, a, b - a) for i in range(d.n_ind) for a, b in reg], dtype=np.int64)
            non = np.exp(h.tract_support(rng)["log_p_non"]).reshape(d.n_ind, len(reg))
            err = np.abs(got["p_none"][:, :, 0] - non).max()
            print(f"  {tag:6s} p_none at 1 site against tract_support's exp(log_p_non): {err:.3e}")
            assert err <= lu.TOL["sites"]["p_none"] + sup.LOG_TOL, (tag, err)


@pytest.mark.parametrize("mode", MODES)
def test_packed_called_genotypes(pkg, mode):
    """8 x 300 called genotypes as 2-bit codes: everything finite; a one-site region on a called
    heterozygote (the IBD state is excluded) has p_any == 0."""
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
            one = h.ibd_longest(L, unit=unit, regions=xu.single_site_regions(S))
            whole = h.ibd_longest(L, unit=unit)
            for f in lu.FIELDS:
                assert np.isfinite(one[f]).all() and np.isfinite(whole[f]).all(), (unit, f)
            assert (one["p_any"][het] == 0.0).all() and (one["p_any"][~het][:, 0] > 0.0).any()
            assert np.abs(one["p_none"][het] - 1.0).max() <= 1e-12      # (pi_s(0), propagated)
            np.testing.assert_allclose(whole["p_any"] + whole["p_none"], 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", MODES)
def test_same_bits_and_nothing_else_moves(pkg, cohort, mode):
    """The same arguments give the same bits; a region's record does not depend on the other
    regions -- nor on whether the thresholds have lanes of their own (NGHMM_LONGEST_SPLIT, read
    at every call); parameters, posteriors, tracts and the next EM iteration are bit-identical
    with and without the call."""
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
                    a, b = h.ibd_longest(L, unit, regions), h.ibd_longest(L, unit, regions)
                    assert a.tobytes() == b.tobytes()
                    h.ibd_longest(L, unit)
                    assert h.ibd_longest(L, unit, regions).tobytes() == a.tobytes()
                    # a region's record does not depend on which other regions are asked for
                    assert h.ibd_longest(L, unit, regions[2:3]).tobytes() == a[:, 2:3].tobytes()
                    for split in ("0", "1"):      # the K thresholds as a loop, as lanes of their own
                        os.environ["NGHMM_LONGEST_SPLIT"] = split
                        try:
                            assert h.ibd_longest(L, unit, regions).tobytes() == a.tobytes(), split
                        finally:
                            del os.environ["NGHMM_LONGEST_SPLIT"]
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


@pytest.mark.parametrize("mode", MODES)
def test_against_the_sampler(pkg, cohort, mode):
    """sample_paths(400, seed 77) on the cohort: the draws' longest_sites >= L (and, from the kept
    paths, the longest run in Mb) against p_any of the whole data under
    longest_util.sampler_check at SAMPLER_LEN: every threshold, every individual
    (tests/test_longest_cpu.py checks the condition on the restatement of the sampler)."""
    d = cohort[0]
    with _handle(pkg, cohort, mode) as h:
        stats, paths = h.sample_paths(xu.SAMPLER_DRAWS, seed=xu.SAMPLER_SEED, keep=xu.SAMPLER_DRAWS)
        exact = {u: h.ibd_longest(bu.SAMPLER_LEN[u], unit=u)["p_any"][:, 0] for u in UNITS}
    assert paths.shape == (xu.SAMPLER_DRAWS, d.n_ind, d.n_sites)
    longest = {"sites": np.where(stats["longest_sites"] > 0, stats["longest_sites"].astype(np.float64), -1.0),
               "mb": lu.path_longest(paths, d.pos_dist_mb, "mb")}
    assert np.array_equal(longest["sites"], lu.path_longest(paths, d.pos_dist_mb, "sites"))
    print()
    for u in UNITS:
        worst = lu.sampler_check(longest[u], exact[u], bu.SAMPLER_LEN[u], u)
        print(f"  device sampler against p_any in {u}: largest |z| = {worst:.2f}")


def test_chain_against_one_handle(pkg, cohort, cohort_want):
    """The same data on 1 handle and as 2 and 3 site shards with uneven cuts -- one inside a
    confident tract of the alpha = 1e-3 individuals, one at a chromosome start, and a middle shard
    of 47 sites under a threshold of 80: the chain returns the single handle's bytes, both units."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    post = cohort_want[2]
    starts = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    inside = [s for s in range(1100, 1400) if (post[:5, s - 40:s + 40] >= 0.9).all(axis=1).any()]
    assert inside, "a cut inside a confident tract of an alpha = 1e-3 individual"
    cut = inside[len(inside) // 2]
    assert cut not in starts and cut < starts[0]
    names = ("whole", "chrom", "win2048", "gaps", "win7", "edges")
    with _handle(pkg, cohort, "fast") as whole:
        sets = xu.region_sets(S, pos, whole.layout()[1])
        want = {(k, u): whole.ibd_longest(bu.COHORT_LEN[u], u, sets[k]) for k in names for u in UNITS}
    for cuts in ([0, cut, S], [0, cut, starts[1], S], [0, cut, cut + 47, S]):
        hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
        try:
            ch = pkg.Chain(hs)
            for (k, u), w in want.items():
                got = ch.ibd_longest(bu.COHORT_LEN[u], u, sets[k])
                assert got.shape == w.shape
                assert got.tobytes() == w.tobytes(), (cuts, k, u, np.abs(got["p_any"] - w["p_any"]).max())
            os.environ["NGHMM_LONGEST_SPLIT"] = "0"      # ... and with the thresholds as a loop in a lane
            try:
                for u in UNITS:
                    assert ch.ibd_longest(bu.COHORT_LEN[u], u, sets["gaps"]).tobytes() == want["gaps", u].tobytes()
            finally:
                del os.environ["NGHMM_LONGEST_SPLIT"]
        finally:
            for h in hs:
                h.close()


def _raw(h, what, lengths, begin, end, stats=True, n=None, k=None, null_len=False, null_begin=False):
    u64 = C.POINTER(C.c_uint64)
    b, e = np.array(begin, dtype=np.uint64), np.array(end, dtype=np.uint64)
    L = np.array(lengths, dtype=np.float64)
    n = len(b) if n is None else n
    k = len(L) if k is None else k
    buf = C.create_string_buffer(16 * h.n_ind * max(n, 1) * max(k, 1))
    rc = h.lib.nghmm_ibd_longest(h.handle, what, k,
                                 None if null_len or not len(L) else L.ctypes.data_as(C.POINTER(C.c_double)), n,
                                 None if null_begin or not len(b) else b.ctypes.data_as(u64),
                                 None if not len(e) else e.ctypes.data_as(u64),
                                 C.cast(buf, C.c_void_p) if stats else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg):
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=3, n_chrom=2)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, 0, [1], [0], [S])                     # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_longest(1)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        assert _raw(h, 0, [1, 5], [0], [S])[0] == 0 and _raw(h, 1, [0, 0.5], [0], [S])[0] == 0
        assert _raw(h, 0, list(range(1, 9)), [0], [S])[0] == 0
        # a whole number of sites beyond any integer type: no window, p_any exactly 0 (and
        # ibd_by_length's tracts likewise)
        assert (h.ibd_longest((1, 1e30))["p_any"][..., 1] == 0).all()
        assert (h.ibd_by_length((1, 1e30))["tracts"][..., 1] == 0).all()
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
            h.ibd_longest(1, unit="cm")
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_longest(1, regions=np.array([[0.0, 5.0]]))
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_longest((3, 2))
        assert ei.value.code == -10 and "increasing" in ei.value.message
        # a chain that was not set up
        with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as g:
            g.load(gl, d.pos_dist_mb)
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            b, e = np.array([0], dtype=np.uint64), np.array([S], dtype=np.uint64)
            L = np.array([1.0])
            buf = C.create_string_buffer(16 * I)
            u64 = C.POINTER(C.c_uint64)
            rc = h.lib.nghmm_chain_ibd_longest(arr, 2, 0, 1, L.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                               b.ctypes.data_as(u64), e.ctypes.data_as(u64),
                                               C.cast(buf, C.c_void_p))
            assert rc == -10 and "nghmm_chain_setup" in h.lib.nghmm_last_error().decode()


def test_longest_classes(pkg, cohort):
    """longest_classes on the device's records per chromosome: K + 1 classes that add up to 1 and
    are non-negative within the tolerance; the last threshold (2000 sites) has no mass."""
    L = np.asarray(bu.COHORT_LEN["sites"], dtype=np.float64)
    with _handle(pkg, cohort, "fast") as h:
        got = h.ibd_longest(L, regions=pkg.chromosome_regions(cohort[0].pos_dist_mb))
    cls = pkg.longest_classes(got)
    tol = lu.TOL["sites"]
    assert cls.shape == got.shape[:-1] + (len(L) + 1,)
    assert np.abs(cls.sum(axis=-1) - 1).max() <= tol["p_any"] + tol["p_none"]
    assert (cls >= -2 * tol["p_any"]).all() and (cls[..., -1] == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_cli_ibd_longest(pkg, tmp_path, mode):
    """ngsF-HMM --ibd_longest at 6 x 400, two chromosomes, all parameters fixed (so the binding can
    be put at the run's final parameters exactly): the file parses and matches ibd_longest to the
    %.10g printed, in Mb and with --longest_sites --longest_window 50; without the flag the set of
    output files and their bytes are those of a run without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", mode]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_longest", "0,0.5,2"])
    cli_util.run_cli(base + ["--out", w, "--ibd_longest", "1,5,40", "--longest_sites", "--longest_window", 50])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.longest"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        for out, window, unit, L in ((a, 0, "mb", (0, 0.5, 2)), (w, 50, "sites", (1, 5, 40))):
            regions = summary_util.chrom_regions(chrom, window)
            got = h.ibd_longest(L, unit=unit, regions=regions)
            lines = open(out + ".ibd.longest").read().split("\n")
            assert lines[0] == "ind\tchr\tfirst_pos\tlast_pos\tn_sites\tmin_len\tp_any\tp_none"
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
                        for text, v in zip(f[6:], (got["p_any"][i, r, k], got["p_none"][i, r, k])):
                            assert text == "%.10g" % float(text)
                            assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[n - 1], v)
