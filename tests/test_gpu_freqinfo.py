"""The per-site likelihood in the allele frequency on the device (nghmm_freq_info /
nghmm_chain_freq_info, include/nghmm.h) against yardstick B of tests/freqinfo_util.py (log space,
np.longdouble), which tests/test_freqinfo_cpu.py checks against enumeration and whole-chain
likelihoods.

Tolerance: 16 x the spread of the two yardsticks on this cohort, per field and in the measure of
freqinfo_util.spread -- |device - B| over the sum of the absolute values of the entry's terms (the
cavity: over c itself) -- as tests/test_freqinfo_cpu.py measures it (freqinfo_util.SPREAD): cavity
3.9e-11, ll 6.3e-14, score 3.4e-14, info 9.0e-14, curve 1.1e-10.  Every entry must be finite and
every site is compared."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cli_util
import freqinfo_util as fu
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

SUMS = ("ll", "score", "info")


@pytest.fixture(scope="module")
def cohort(pkg):
    return fu.gpu_cohort(pkg)


@pytest.fixture(scope="module")
def yardstick(cohort):
    """B on the cohort at its eight levels: computed once, shared, left unchanged."""
    d, gl, F, A, freq = cohort
    return fu.freq_info_b(np.exp(gl), d.pos_dist_mb, F, A, freq, fu.LEVELS)


def _handle(pkg, cohort, mode, called=None, F=None, A=None, freq=None, sites=None):
    d, gl, F0, A0, freq0 = cohort
    lo, hi = sites or (0, d.n_sites)
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | (pkg.GENO_PACKED if called == "packed" else 0)
    h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=m)
    pos = np.ascontiguousarray(d.pos_dist_mb[lo:hi])
    if called:
        h.load_raw(np.ascontiguousarray(d.gl[lo:hi]), pos, space=0, call_geno=True)
    else:
        h.load(np.ascontiguousarray(gl[lo:hi]), pos)
    h.set_params(F0 if F is None else F, A0 if A is None else A, (freq0 if freq is None else freq)[lo:hi])
    h.init_emission()
    return h


def _as_dict(res):
    stats, curve, cav = res
    return {"cavity": cav, "ll": stats["ll"], "score": stats["score"], "info": stats["info"], "curve": curve}


def _bytes(res):
    return tuple(np.ascontiguousarray(x).tobytes() for x in res)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_fields_match_the_yardstick(pkg, cohort, yardstick, mode):
    d, gl, F, A, freq = cohort
    pos, S = d.pos_dist_mb, d.n_sites
    assert len(fu.LEVELS) == 8 and 0.0 in fu.LEVELS and 1.0 in fu.LEVELS
    with _handle(pkg, cohort, mode) as h:
        if mode == "fast":
            # sites on both sides of every lane-chunk boundary, a chromosome start inside a lane-chunk
            T = h.layout()[1]
            bounds = np.arange(T, S, T)
            assert len(bounds) > 10 and bounds[-1] < S and bounds[0] - 1 >= 0
            starts = np.flatnonzero(np.isinf(pos))
            assert any(s > 0 and s % T != 0 for s in starts)
        stats, curve, cav = h.freq_info(fu.LEVELS, cavity=True)
        assert stats.dtype == pkg.FREQ_STAT_DTYPE and stats.shape == (S,)
        assert curve.shape == (S, 8) and cav.shape == (d.n_ind, S)
        assert np.array_equal(stats["freq"], freq)
        got = _as_dict((stats, curve, cav))
        for f in fu.FIELDS:
            assert np.isfinite(got[f]).all() and np.isfinite(yardstick[f]).all(), f
        err = fu.spread(got, yardstick)
        print()
        for f in fu.FIELDS:
            print(f"  {mode:5s} {f:6s}: largest |device - B| / scale = {err[f]:.3e} (tol {fu.TOL[f]:.3e})")
        for f in fu.FIELDS:
            assert err[f] <= fu.TOL[f], (mode, f, err[f])
        # the standard errors: 1 / sqrt(info) where info > 0
        se = pkg.freq_std_errors(stats)
        ok = stats["info"] > 0
        assert ok.mean() > 0.9 and np.array_equal(np.isnan(se), ~ok)
        np.testing.assert_allclose(se[ok], 1 / np.sqrt(stats["info"][ok]), rtol=1e-15)


def test_curve_equals_whole_chain_likelihood_differences(pkg, cohort):
    """The identity through code the feature does not touch: one entry of freq replaced, the sum
    of the forward log-likelihoods (nghmm_lkl_batch) minus the same at the original frequencies is
    curve[s][k], within 2 x 1e-12 x sum_i |lkl_i| -- the project's own per-call bound on fast-mode
    log-likelihoods (README, parity paragraph)."""
    d, gl, F, A, freq = cohort
    pos, S, I = d.pos_dist_mb, d.n_sites, d.n_ind
    levels = (0.05, 0.9)
    ind = np.arange(I)
    with _handle(pkg, cohort, "fast") as h:
        T = h.layout()[1]
        cs = int([s for s in np.flatnonzero(np.isinf(pos)) if s > 0][0])
        sites = [0, S - 1, cs, 7 * T - 1, 7 * T, 2 * T + T // 2 + 1]
        assert len(set(sites)) == 6 and all(0 <= s < S for s in sites)
        stats, curve = h.freq_info(levels)
        base = h.lkl(ind, F, A)
        bound = 2 * 1e-12 * np.abs(base).sum()
        print(f"\n  bound {bound:.2e}")
        for s in sites:
            for k, x in enumerate(levels):
                fr = freq.copy()
                fr[s] = x
                h.set_params(freq=fr)
                h.init_emission()                     # (nghmm_lkl_batch reads the current EMISSIONS)
                diff = float((h.lkl(ind, F, A) - base).sum())
                print(f"  site {s:4d} level {x}: curve {curve[s, k]: .9f}, whole chain {diff: .9f}, "
                      f"difference {abs(diff - curve[s, k]):.2e}")
                assert abs(diff - curve[s, k]) <= bound, (s, x)
        assert np.abs(curve[sites]).max() > 0.5


def test_packed_called_genotypes(pkg, cohort):
    """Called genotypes as 2-bit codes, levels 0 and 1: an individual whose genotype the level
    excludes makes the entry -inf, exactly where the yardstick has it; nothing is NaN; at a
    frequency inside (0, 1) no bracket is 0, so stats has neither -inf nor NaN."""
    d, gl, F, A, freq = cohort
    levels = (0.0, 1.0)
    with _handle(pkg, cohort, "fast", called="packed") as h:
        p = np.exp(h.gl)
        assert (p == 0).mean() > 0.5 and p.max() <= 1.0          # the restatement carries the exact zeros
        want = fu.freq_info_b(p, d.pos_dist_mb, F, A, freq, levels)
        stats, curve, cav = h.freq_info(levels, cavity=True)
        got = _as_dict((stats, curve, cav))
        inf = np.isneginf(want["curve"])
        assert inf.mean() > 0.5 and (~inf).sum() > 20
        assert not np.isnan(curve).any() and np.array_equal(np.isneginf(curve), inf)
        for f in SUMS:
            assert np.isfinite(want[f]).all() and np.isfinite(got[f]).all(), f
            err = np.abs(got[f] - want[f]) / want["abs_" + f]
            assert err.max() <= fu.TOL[f], (f, err.max())
        err = np.abs(curve[~inf] - want["curve"][~inf]) / want["abs_curve"][~inf]
        assert err.max() <= fu.TOL["curve"], err.max()
        # a called heterozygote excludes IBD whatever the other sites say: c stays a probability
        assert np.isfinite(cav).all() and cav.min() >= 0.0 and cav.max() <= 1.0


def test_a_bracket_that_is_zero_at_the_current_frequency(pkg, cohort):
    """Packed called genotypes with the frequency of three sites set to 0 or 1: an individual
    whose genotype that frequency excludes has the bracket 0 there, so ll = -inf and score, info
    and the site's curve are NaN -- exactly where yardstick B has them, and nothing else is -inf
    or NaN in stats.  Each of the three sites is a chromosome of its own (the individual's
    likelihood on that chromosome is 0, which leaves every other chromosome defined); the cavity
    stays a probability everywhere."""
    import dataclasses
    d, gl, F, A, freq = cohort
    levels = (0.0, 0.3, 1.0)
    sites, values = (300, 2100, 4000), (0.0, 1.0, 0.0)
    pos, fr = d.pos_dist_mb.copy(), freq.copy()
    for s, x in zip(sites, values):
        pos[s] = pos[s + 1] = np.inf
        fr[s] = x
    d2 = dataclasses.replace(d, pos_dist_mb=pos)
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST | pkg.GENO_PACKED) as h:
        h.load_raw(np.ascontiguousarray(d2.gl), pos, space=0, call_geno=True)
        h.set_params(F, A, fr)
        want = fu.freq_info_b(np.exp(h.gl), pos, F, A, fr, levels)
        other = fu.freq_info_a(np.exp(h.gl), pos, F, A, fr)
        stats, curve, cav = h.freq_info(levels, cavity=True)
    dead = np.isneginf(want["ll"])
    assert dead.sum() >= 2 and set(np.flatnonzero(dead)) <= set(sites)
    assert np.array_equal(np.isneginf(stats["ll"]), dead) and not np.isnan(stats["ll"]).any()
    for f in ("score", "info"):
        assert np.array_equal(np.isnan(stats[f]), dead), f
        assert np.isfinite(stats[f][~dead]).all() and np.isnan(want[f][dead]).all(), f
    assert np.array_equal(np.isnan(curve), np.isnan(want["curve"]))
    assert np.array_equal(np.isnan(curve), np.repeat(dead[:, None], len(levels), axis=1))
    assert np.array_equal(np.isneginf(curve), np.isneginf(want["curve"]))
    assert np.isfinite(cav).all() and cav.min() >= 0.0 and cav.max() <= 1.0
    live = ~dead
    for f in SUMS:
        err = np.abs(stats[f][live] - want[f][live]) / want["abs_" + f][live]
        assert err.max() <= fu.TOL[f], (f, err.max())
    fin = np.isfinite(want["curve"])
    err = np.abs(curve[fin] - want["curve"][fin]) / want["abs_curve"][fin]
    assert err.max() <= fu.TOL["curve"], err.max()
    # the cavity: called genotypes drive c down to 1e-14, where the yardsticks themselves differ far
    # more, relative to c, than on likelihoods: 16 x THEIR spread on these cells (A against B), the
    # rule freqinfo_util.TOL is made by
    assert want["cavity"].min() > 0 and cav.min() > 0
    tol = 16 * np.max(np.abs(other["cavity"] - want["cavity"]) / want["cavity"])
    err = np.max(np.abs(cav - want["cavity"]) / want["cavity"])
    print(f"\n  cavity: largest |device - B| / c = {err:.3e} (tol {tol:.3e}, smallest c {want['cavity'].min():.1e})")
    assert err <= tol


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_nothing_else_moves_and_the_same_bytes(pkg, cohort, mode):
    d = cohort[0]
    lv = np.array(fu.LEVELS[:3])
    with _handle(pkg, cohort, mode) as a, _handle(pkg, cohort, mode) as b:
        for h in (a, b):
            h.estep()
            h.viterbi()
        state = lambda h: (h.indF.tobytes(), h.alpha.tobytes(), h.freq.tobytes(), h.marg_prob.tobytes(),
                           h.ibd_tracts("viterbi").tobytes(), h.e_prob.tobytes())
        before = state(a)
        r1 = a.freq_info(lv, cavity=True)
        assert state(a) == before
        assert _bytes(a.freq_info(lv, cavity=True)) == _bytes(r1)
        # whichever outputs are asked for
        assert _bytes(a.freq_info(lv)) == _bytes(r1[:2])
        assert a.freq_info()[0].tobytes() == r1[0].tobytes()
        L, S, I = a.lib, d.n_sites, d.n_ind
        cav = np.zeros((I, S))
        assert L.nghmm_freq_info(a.handle, 0, None, None, None, cav.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert cav.tobytes() == r1[2].tobytes()
        curve = np.zeros((S, 3))
        assert L.nghmm_freq_info(a.handle, 3, lv.ctypes.data_as(C.POINTER(C.c_double)), None,
                                 curve.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
        assert curve.tobytes() == r1[1].tobytes()
        # a level's column does not depend on the other levels
        assert a.freq_info(lv[1:2])[1].tobytes() == np.ascontiguousarray(r1[1][:, 1:2]).tobytes()
        assert state(a) == before
        for h in (a, b):
            h.iter_EM()
        for f in ("indF", "alpha", "freq", "marg_prob", "ind_lkl"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_results_follow_the_current_parameters(pkg, cohort):
    """After set_params (and init_emission, which every call needs after new frequencies) the call
    answers for the new parameters: within the tolerance of yardstick B there, far from the old
    answer, and the bytes of a fresh handle at those parameters; the posteriors stay the old
    E-step's."""
    d, gl, F, A, freq = cohort
    rng = np.random.default_rng(7)
    F2, A2 = rng.uniform(0.05, 0.9, d.n_ind), rng.uniform(0.02, 1.5, d.n_ind)
    freq2 = np.clip(freq + rng.uniform(-0.04, 0.04, d.n_sites), 0.01, 0.99)
    lv = fu.LEVELS[:2]
    want = fu.freq_info_b(np.exp(gl), d.pos_dist_mb, F2, A2, freq2, lv)
    with _handle(pkg, cohort, "fast") as h:
        h.estep()
        marg = h.marg_prob.copy()
        old = h.freq_info(lv, cavity=True)
        h.set_params(F2, A2, freq2)
        h.init_emission()
        new = h.freq_info(lv, cavity=True)
        assert np.array_equal(new[0]["freq"], freq2)
        assert np.abs(new[0]["score"] - old[0]["score"]).max() > 1.0
        assert np.abs(new[2] - old[2]).max() > 1e-2
        assert h.marg_prob.tobytes() == marg.tobytes()       # still the old E-step's
    err = fu.spread(_as_dict(new), want)
    print("\n  " + ", ".join(f"{f} {err[f]:.2e}" for f in fu.FIELDS))
    for f in fu.FIELDS:
        assert err[f] <= fu.TOL[f], (f, err[f])
    with _handle(pkg, cohort, "fast", F=F2, A=A2, freq=freq2) as g:
        assert _bytes(g.freq_info(lv, cavity=True)) == _bytes(new)


CUTS = ([0, 1877, 5003], [0, 1877, 3500, 5003])      # an odd site; both inside a chromosome


def _chain(pkg, cohort, cuts):
    return [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("cuts", CUTS, ids=["two", "three"])
def test_chains_match_the_yardstick(pkg, cohort, yardstick, cuts):
    """Chains of 2 and 3 site shards: every field within the tolerance of yardstick B, the same
    bytes on a second call, and the records carry the global order (freq is the whole vector)."""
    d, gl, F, A, freq = cohort
    starts = [int(s) for s in np.flatnonzero(np.isinf(d.pos_dist_mb))]
    assert cuts[-1] == d.n_sites and cuts[1] % 2 == 1
    assert all(abs(c - s) > 50 for c in cuts[1:-1] for s in starts)
    hs = _chain(pkg, cohort, cuts)
    try:
        got = pkg.Chain(hs).freq_info(fu.LEVELS, cavity=True)
        assert _bytes(pkg.Chain(hs).freq_info(fu.LEVELS, cavity=True)) == _bytes(got)
    finally:
        for h in hs:
            h.close()
    assert np.array_equal(got[0]["freq"], freq)
    err = fu.spread(_as_dict(got), yardstick)
    for f in fu.FIELDS:
        assert err[f] <= fu.TOL[f], (cuts, f, err[f])


def test_chains_equal_the_single_handle(pkg, cohort):
    """Chains of 2 and 3 site shards, cut at an odd site and inside a chromosome: the bytes of the
    single handle (the walks are site-by-site vector recursions that a shard continues bit for
    bit)."""
    d, gl, F, A, freq = cohort
    with _handle(pkg, cohort, "fast") as whole:
        want = whole.freq_info(fu.LEVELS, cavity=True)
    w = _as_dict(want)
    same = []
    print()
    for cuts in CUTS:
        hs = _chain(pkg, cohort, cuts)
        try:
            got = pkg.Chain(hs).freq_info(fu.LEVELS, cavity=True)
        finally:
            for h in hs:
                h.close()
        g = _as_dict(got)
        print(f"  cuts {cuts}: largest |chain - single|: "
              + ", ".join(f"{f} {np.abs(g[f] - w[f]).max():.2e}" for f in fu.FIELDS))
        same.append(_bytes(got) == _bytes(want))
    assert all(same), same


def test_argument_errors(pkg, cohort):
    d = cohort[0]
    S, I = d.n_sites, d.n_ind
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    stats = np.zeros(S, dtype=pkg.FREQ_STAT_DTYPE)
    curve = np.zeros((S, 9))
    sp = C.c_void_p(stats.ctypes.data)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        with pytest.raises(pkg.NgsFHMMError) as ei:          # no data loaded
            h.freq_info()
        assert ei.value.code == -10 and "no data" in ei.value.message
    with _handle(pkg, cohort, "fast") as h:
        L = h.lib
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.freq_info(np.linspace(0.1, 0.9, 9))
        assert ei.value.code == -10 and "n_levels = 9" in ei.value.message
        for bad in (-0.1, 1.5, math.nan):
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.freq_info((0.5, bad))
            assert ei.value.code == -10 and "levels[1]" in ei.value.message, (bad, ei.value.message)
        assert L.nghmm_freq_info(h.handle, 0, None, None, None, None) == -10     # all outputs NULL
        assert b"all NULL" in L.nghmm_last_error()
        lv = np.array([0.5])
        assert L.nghmm_freq_info(h.handle, 1, dp(lv), sp, None, None) == -10     # levels without a curve
        assert b"curve" in L.nghmm_last_error()
        assert L.nghmm_freq_info(h.handle, 0, None, sp, dp(curve), None) == -10  # a curve without levels
        assert b"curve" in L.nghmm_last_error()
        assert L.nghmm_freq_info(None, 0, None, sp, None, None) == -10
        assert L.nghmm_chain_freq_info(None, 1, 0, None, sp, None, None) == -10
        assert L.nghmm_freq_info(h.handle, 0, None, sp, None, None) == 0
        # two handles that nghmm_chain_setup has not seen
        with _handle(pkg, cohort, "fast") as g:
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            assert L.nghmm_chain_freq_info(arr, 2, 0, None, sp, None, None) == -10
            assert b"nghmm_chain_setup" in L.nghmm_last_error()


def _g10(v):
    return "NA" if v != v else "-inf" if v == -math.inf else "%.10g" % v


def test_cli_freq_info(pkg, tmp_path):
    """ngsF-HMM --freq_info on a chain of two with all parameters fixed (so the binding can be put
    at the run's final parameters exactly): the header and every line of PREFIX.freq.info are the
    text made from Chain.freq_info; the other output files are those of a run without the flag."""
    I, S = 12, 3001
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast", "--n_gpus", 2,
            "--devices", "0,0", "--ibd_bed"]
    plain, a, b = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "b")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--freq_info"])
    cli_util.run_cli(base + ["--out", b, "--freq_info", "--freq_levels", "0,0.25,1"])
    for ext in (".indF", ".ibd", ".geno", ".ibd.bed"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
        assert open(plain + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("a.")) == \
        sorted(["a" + f[5:] for f in os.listdir(tmp_path) if f.startswith("plain.")] + ["a.freq.info"])
    # the same through the binding: a chain cut where the host cuts (multiples of 16 sites)
    cut = S // 2 // 16 * 16
    hs = []
    try:
        for lo, hi in ((0, cut), (cut, S)):
            h = pkg.NgsFHMM(I, hi - lo, mode=pkg.MODE_FAST)
            hs.append(h)
            h.load_raw(np.ascontiguousarray(d.gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]), space=0)
            h.set_params(0.6, 0.05, 0.1)
            h.init_emission()
        ch = pkg.Chain(hs)
        ch.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        ch.viterbi()
        res = {"a": ch.freq_info((0.0,)), "b": ch.freq_info((0.0, 0.25, 1.0))}
    finally:
        for h in hs:
            h.close()
    for tag, prefix, levels in (("a", a, (0.0,)), ("b", b, (0.0, 0.25, 1.0))):
        stats, curve = res[tag]
        se = pkg.freq_std_errors(stats)
        want = ["\t".join(["chr", "pos", "freq", "se", "ll", "score", "info"] + ["dll_%g" % x for x in levels])]
        for s in range(S):
            want.append("\t".join([f"chr{int(d.chrom[s])}", str(int(d.pos[s]))] +
                                  [_g10(float(v)) for v in (stats["freq"][s], se[s], stats["ll"][s],
                                                            stats["score"][s], stats["info"][s])] +
                                  [_g10(float(v)) for v in curve[s]]))
        got = open(prefix + ".freq.info").read().split("\n")
        assert got[-1] == "" and len(got) == S + 2
        assert got[0] == want[0]
        assert got[1:-1] == want[1:], tag
