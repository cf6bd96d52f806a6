"""Exact posterior means and covariances of (IBD sites or Mb, number of tracts) on the device
(nghmm_ibd_moments / nghmm_chain_ibd_moments, include/nghmm.h) against brute-force enumeration and
against yardstick B of tests/moments_util.py (uncentred jets in np.longdouble), which
tests/test_moments_cpu.py checks against enumeration.

Tolerance.  The two yardsticks A (float64, centred per site) and B differ by at most
(tests/test_moments_cpu.py measures and prints the figures; moments_util.COHORT_SPREAD /
CONFIDENT_SPREAD hold them)
    20 x 5003 cohort, all region sets   sites: mean_a 1.8e-11, mean_t 5.4e-13, var_a 8.2e-10,
                                               cov_at 1.9e-12, var_t 3.3e-13
                                        mb:    mean_a 1.5e-12, var_a 9.0e-12, cov_at 2.2e-13
    4 x 20011 confident chain           sites: mean_a 6.2e-11, mean_t 1.5e-13, var_a 6.6e-10,
                                               cov_at 8.4e-13, var_t 5.0e-15
                                        mb:    mean_a 5.0e-14, var_a 2.1e-15, cov_at 2.4e-15
-- the spread of two correct restatements.  The tolerance is 16 x the spread per field, the
project's rule and margin (expect_util.REGION_TOL: the device groups and rescales its products
unlike either restatement); nothing in it comes from a device.  The yardstick runs once per cohort
on the emissions numpy makes of the likelihoods and the frequency, and is shared by the tests."""
import ctypes as C
import os

import numpy as np
import pytest

import cli_util
import expect_util as xu
import moments_util as mu
import sample_util as su
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# Enumeration over 2^12 paths in float64 agrees with both restatements to 2e-14
# (tests/test_moments_cpu.py); the device's emissions reach the host through a logarithm and go
# back through an exponential (1e-16 per site, twelve sites; variances of the order of 1): 1e-12,
# as tests/test_gpu_expect.py.
ENUM_TOL = 1e-12
MODES = ["fast", "exact"]


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


@pytest.fixture(scope="module")
def cohort_want(pkg, cohort):
    """Yardstick B on the cohort: {length: {set: [I][R]}} over the region sets for the lane length
    of the layout the device reports for it (both modes get the same sets)."""
    d, gl, F, A, freq = cohort
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    with _handle(pkg, cohort, "fast") as h:
        T = h.layout()[1]
    assert T > 0
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    out = {}
    for L in mu.LENGTHS:
        b = mu.moments_b(e, d.pos_dist_mb, F, A, list(sets.values()), L)
        out[L] = dict(zip(sets, b))
    return sets, out


def _handle(pkg, cohort, mode, sites=None):
    d, gl, F, A, freq = cohort
    lo, hi = sites or (0, d.n_sites)
    h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT)
    h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
    h.set_params(F, A, freq)
    h.init_emission()
    return h


def _check(got, want, tol, tag):
    for f in mu.FIELDS:
        assert np.isfinite(got[f]).all(), (tag, f)
        err = np.abs(got[f] - want[f])
        t = tol[f] if isinstance(tol, dict) else tol
        print(f"  {tag:16s} {f:7s}: largest |device - yardstick| = {err.max():.3e} (tol {t:.3e})")
        assert (err <= t).all(), (tag, f, err.max())


@pytest.mark.parametrize("mode", MODES)
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths, both lengths: the whole data, the chromosomes, [3, 9) with
    the chromosome start inside, every single site; a missing cell, an excluded state."""
    _, pos, F, A, _, gl, freq = xu.small_case()
    I, S = gl.shape[1], gl.shape[0]
    gl = np.where(np.isneginf(gl), -1e15, gl)          # (the reader's likelihood of an excluded genotype)
    m = pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load(np.ascontiguousarray(gl), pos)
        h.set_params(F, A, freq)
        h.init_emission()
        e = h.e_prob
        assert np.isneginf(e[1, 4, 1]) or e[1, 4, 1] < -1e14
        print()
        for L in mu.LENGTHS:
            for name, reg in mu.small_regions().items():
                got = h.ibd_moments(reg, length=L)
                assert got.dtype == pkg.MOMENT_REGION_DTYPE and got.shape == (I, len(reg))
                _check(got, mu.enumerate_moments(e, pos, F, A, reg, L), ENUM_TOL, f"{L} {name}")
                if name == "cells":
                    assert got["var_a"][1, 4] == 0.0 and got["var_t"][1, 4] == 0.0 and got["mean_a"][1, 4] == 0.0
            whole = h.ibd_moments(None, length=L)
            assert whole.tobytes() == h.ibd_moments(np.array([[0, S]]), length=L).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_yardstick(pkg, cohort, cohort_want, mode):
    """20 x 5003 against yardstick B within 16 x spread, both lengths: the chromosomes; windows of
    7, 64, 2048 and 2049 sites; single sites on both sides of every lane-chunk edge; a region across
    a chromosome start among regions with gaps; the whole data."""
    d = cohort[0]
    pos = d.pos_dist_mb
    sets, want = cohort_want
    with _handle(pkg, cohort, mode) as h:
        T = int(sets["edges"][1, 1])                  # (the lane length the sets were made for)
        assert mode != "fast" or h.layout()[1] == T
        cs = int([x for x in np.flatnonzero(np.isinf(pos)) if x > 0][0])
        assert ((sets["gaps"][:, 0] < cs) & (sets["gaps"][:, 1] > cs)).any()
        bounds = np.arange(T, d.n_sites, T)
        assert np.isin(bounds, sets["edges"][:, 0]).all() and np.isin(bounds - 1, sets["edges"][:, 0]).all()
        assert len(bounds) > 10
        print()
        for L in mu.LENGTHS:
            for tag, reg in sets.items():
                got = h.ibd_moments(reg, length=L)
                _check(got, want[L][tag], mu.COHORT_TOL[L], f"{L} {tag}")
                assert (got["var_a"] >= 0).all() and (got["var_t"] >= 0).all()


@pytest.fixture(scope="module")
def confident(pkg):
    gl, pos, F, A, freq, regs = mu.confident_case(pkg)
    e = su.emissions_np(gl, np.full(gl.shape[0], freq))
    want = {L: dict(zip(regs, mu.moments_b(e, pos, F, A, list(regs.values()), L))) for L in mu.LENGTHS}
    return gl, pos, F, A, freq, regs, want


@pytest.mark.parametrize("mode", MODES)
def test_accuracy_on_a_confident_chain(pkg, confident, mode):
    """4 x 20011, two chromosomes, tracts of 400 sites known almost surely: thousands of IBD sites
    with a variance of tens.  The whole data and one interior region against yardstick B at 16 x
    spread -- the test an uncentred float64 jet fails (eps E[A]^2 / Var: 1e-8 relative here)."""
    gl, pos, F, A, freq, regs, want = confident
    S, I = gl.shape[0], gl.shape[1]
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) as h:
        h.load(gl, pos)
        h.set_params(F, A, freq)
        h.init_emission()
        print()
        for L in mu.LENGTHS:
            for tag, reg in regs.items():
                _check(h.ibd_moments(reg, length=L), want[L][tag], mu.CONFIDENT_TOL[L], f"{L} {tag}")


@pytest.mark.parametrize("mode", MODES)
def test_identities(pkg, cohort, mode):
    """The means are ibd_expect's; chromosome variances and covariances add up to the whole
    data's; a one-site region has var_a = pi (1 - pi); variances >= 0 and Cauchy-Schwarz."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    with _handle(pkg, cohort, mode) as h:
        sets = xu.region_sets(S, pos, h.layout()[1] or mu.SPREAD_LANE_SITES)
        print()
        for tag in ("whole", "chrom", "win64", "gaps", "edges"):
            ex = h.ibd_expect(sets[tag], sites=False)[0]
            for L, fa in (("sites", "ibd"), ("mb", "ibd_mb")):
                got = h.ibd_moments(sets[tag], length=L)
                tol = mu.COHORT_TOL[L]
                for f, g in (("mean_a", fa), ("mean_t", "starts")):
                    err = np.abs(got[f] - ex[g]).max()
                    print(f"  {L:5s} {tag:6s} {f} against ibd_expect's {g}: {err:.3e} (tol {xu.REGION_TOL[g]:.3e})")
                    assert err <= xu.REGION_TOL[g]
                assert (got["var_a"] >= 0).all() and (got["var_t"] >= 0).all()
                # what errors of the three fields within their tolerances move the two sides by
                slack = tol["cov_at"] * (2 * np.abs(got["cov_at"]) + tol["cov_at"]) + \
                    tol["var_a"] * got["var_t"] + tol["var_t"] * got["var_a"]
                assert (got["cov_at"] ** 2 <= got["var_a"] * got["var_t"] * (1 + 1e-9) + slack).all(), (L, tag)
                if tag == "edges" and L == "sites":
                    pi = ex["ibd"]
                    err = np.abs(got["var_a"] - pi * (1 - pi)).max()
                    print(f"  one-site regions: var_a against pi (1 - pi): {err:.3e}")
                    assert err <= tol["var_a"] + 2 * xu.REGION_TOL["ibd"]
        for L in mu.LENGTHS:
            whole, chrom = h.ibd_moments(sets["whole"], length=L), h.ibd_moments(sets["chrom"], length=L)
            assert len(sets["chrom"]) == 3
            for f in mu.FIELDS:
                err = np.abs(chrom[f].sum(axis=1) - whole[f][:, 0]).max()
                print(f"  {L:5s} chromosomes add up to the whole, {f}: {err:.3e}")
                assert err <= 4 * mu.COHORT_TOL[L][f]      # (three records and the whole, each within tol)


@pytest.mark.parametrize("mode", MODES)
def test_packed_called_genotypes(pkg, mode):
    """8 x 300 called genotypes as 2-bit codes: everything finite; a one-site region on a called
    heterozygote (the IBD state is excluded) has mean and variance exactly 0."""
    I, S = 8, 300
    d = pkg.simulate.simulate(I, S, seed=5, n_chrom=2, indF=0.4, alpha=0.1)
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | pkg.GENO_PACKED
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=True)
        h.set_params(0.4, 0.1, 0.2)
        h.init_emission()
        e = h.e_prob
        het = e[..., 1] < -1e14
        assert het.sum() > 50
        for L in mu.LENGTHS:
            one = h.ibd_moments(xu.single_site_regions(S), length=L)
            for f in mu.FIELDS:
                assert np.isfinite(one[f]).all(), (L, f)
            assert (one["var_a"][het] == 0.0).all() and (one["var_t"][het] == 0.0).all()
            assert (one["mean_a"][het] == 0.0).all() and (one["cov_at"][het] == 0.0).all()
            assert (one["var_a"][~het] > 0.0).any()
            whole = h.ibd_moments(None, length=L)
            for f in mu.FIELDS:
                assert np.isfinite(whole[f]).all(), (L, f)
            np.testing.assert_allclose(whole["mean_a"][:, 0], one["mean_a"].sum(axis=1), rtol=1e-12)


def test_same_bits_and_nothing_else_moves(pkg, cohort):
    d = cohort[0]
    regions = pkg.window_regions(d.pos_dist_mb, 777)

    def run(with_call):
        out = {}
        with _handle(pkg, cohort, "fast") as h:
            h.iter_EM(1)
            h.viterbi()
            out["before"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ibd_tracts("viterbi"))
            if with_call:
                for L in mu.LENGTHS:
                    a, b = h.ibd_moments(regions, length=L), h.ibd_moments(regions, length=L)
                    assert a.tobytes() == b.tobytes()
                    h.ibd_moments(None, length=L)
                    assert h.ibd_moments(regions, length=L).tobytes() == a.tobytes()
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


def test_against_the_sampler(pkg, cohort):
    """sample_paths(400, seed) on the cohort under moments_util.sampler_check: the sample
    variances of ibd_sites, n_tracts and ibd_mb per individual and of the cohort totals, and the
    sample covariance of (ibd_sites, n_tracts), within 5 standard errors of the exact values
    (tests/test_moments_cpu.py checks the condition on the restatement of the sampler)."""
    with _handle(pkg, cohort, "fast") as h:
        stats, _ = h.sample_paths(mu.SAMPLER_DRAWS, seed=mu.SAMPLER_SEED)
        sites, mb = h.ibd_moments(None)[:, 0], h.ibd_moments(None, length="mb")[:, 0]
    worst = mu.sampler_check(stats, sites, mb)
    print(f"\n  device sampler against the exact variances: largest |z| = {worst:.2f}")


def test_chain_against_one_handle(pkg, cohort):
    """The same data on 1 handle and as 3 site shards with uneven cuts, one inside a region and
    one at a chromosome start: within the tolerance of the single handle, both lengths."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    starts = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    cuts = [0, 1203, starts[1], S]
    assert cuts[1] not in starts and cuts[1] < cuts[2]
    names = ("whole", "chrom", "win2048", "gaps", "win7", "edges")
    with _handle(pkg, cohort, "fast") as whole:
        sets = xu.region_sets(S, pos, whole.layout()[1])
        want = {(k, L): whole.ibd_moments(sets[k], length=L) for k in names for L in mu.LENGTHS}
    assert ((sets["win2048"][:, 0] < cuts[1]) & (sets["win2048"][:, 1] > cuts[1])).any()
    hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        ch = pkg.Chain(hs)
        print()
        for (k, L), w in want.items():
            got = ch.ibd_moments(sets[k], length=L)
            assert got.shape == w.shape
            _check(got, w, mu.COHORT_TOL[L], f"{L} {k}")
        a, b = ch.ibd_moments(sets["chrom"]), ch.ibd_moments(sets["chrom"])
        assert a.tobytes() == b.tobytes()
    finally:
        for h in hs:
            h.close()


def _raw(h, what, begin, end, regions=True, n=None, null_begin=False, null_end=False):
    u64 = C.POINTER(C.c_uint64)
    b, e = np.array(begin, dtype=np.uint64), np.array(end, dtype=np.uint64)
    n = len(b) if n is None else n
    rbuf = C.create_string_buffer(40 * h.n_ind * max(n, 1))
    rc = h.lib.nghmm_ibd_moments(h.handle, what, n, None if null_begin or not len(b) else b.ctypes.data_as(u64),
                                 None if null_end or not len(e) else e.ctypes.data_as(u64),
                                 C.cast(rbuf, C.c_void_p) if regions else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg):
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=3, n_chrom=2)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, 0, [0], [S])                          # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_moments(None)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        assert _raw(h, 0, [0], [S])[0] == 0 and _raw(h, 1, [0], [S])[0] == 0
        bad = [
            ((2, [0], [S]), {}),                                # an unknown bit
            ((1 | 4, [0], [S]), {}),
            ((0, [], []), {"n": 0}),                            # n_regions == 0
            ((0, [0], [S]), {"regions": False}),                # a NULL pointer
            ((0, [0], [S]), {"null_begin": True}),
            ((0, [0], [S]), {"null_end": True}),
            ((0, [10, 5], [20, 8]), {}),                        # unsorted
            ((0, [0, 9], [10, 20]), {}),                        # overlapping
            ((0, [0, 10], [10, 10]), {}),                       # empty
            ((0, [0], [S + 1]), {}),                            # end > S
        ]
        for args, kw in bad:
            rc, msg = _raw(h, *args, **kw)
            assert rc == -10 and msg, (args, kw, rc, msg)
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_moments(np.array([[10, 20], [5, 8]]))
        assert ei.value.code == -10 and ei.value.message
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_moments(np.array([[0.0, 5.0]]))
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_moments(None, length="cm")
        assert _raw(h, 0, [0, 10], [10, S])[0] == 0             # touching regions do not overlap
        # a chain that was not set up
        with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as g:
            g.load(gl, d.pos_dist_mb)
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            b, e = np.array([0], dtype=np.uint64), np.array([S], dtype=np.uint64)
            rbuf = C.create_string_buffer(40 * I)
            u64 = C.POINTER(C.c_uint64)
            rc = h.lib.nghmm_chain_ibd_moments(arr, 2, 0, 1, b.ctypes.data_as(u64), e.ctypes.data_as(u64),
                                               C.cast(rbuf, C.c_void_p))
            assert rc == -10 and "nghmm_chain_setup" in h.lib.nghmm_last_error().decode()


def test_moment_sd(pkg, cohort):
    """moment_sd on hand-made records (the NaN rules) and on the device's."""
    rec = np.zeros((1, 3), dtype=pkg.MOMENT_REGION_DTYPE)
    rec["mean_a"], rec["mean_t"] = [[12.0, 3.0, 5.0]], [[3.0, 0.0, 2.0]]
    rec["var_a"], rec["var_t"], rec["cov_at"] = [[4.0, 1.0, 9.0]], [[0.25, 0.0, 1.0]], [[0.5, 0.0, -1.5]]
    sd = pkg.moment_sd(rec)
    assert np.array_equal(sd["sd_a"], [[2.0, 1.0, 3.0]]) and np.array_equal(sd["sd_t"], [[0.5, 0.0, 1.0]])
    assert np.array_equal(sd["corr"], [[0.5, np.nan, -0.5]], equal_nan=True)
    assert np.array_equal(sd["tract_length"], [[4.0, np.nan, 2.5]], equal_nan=True)
    want = [[np.sqrt(4.0 - 4.0 + 4.0) / 3.0, np.nan, np.sqrt(9.0 + 7.5 + 6.25) / 2.0]]
    np.testing.assert_allclose(sd["tract_length_sd"], want, rtol=1e-15, equal_nan=True)
    with _handle(pkg, cohort, "fast") as h:
        got = h.ibd_moments(pkg.chromosome_regions(cohort[0].pos_dist_mb))
    sd = pkg.moment_sd(got)
    ok = (got["var_a"] > 0) & (got["var_t"] > 0)
    assert ok.any() and (np.abs(sd["corr"][ok]) <= 1 + 1e-9).all() and np.isnan(sd["corr"][~ok]).all()
    assert (sd["tract_length_sd"][got["mean_t"] > 0] >= 0).all()


def test_cli_ibd_moments(pkg, tmp_path):
    """ngsF-HMM --ibd_moments at 6 x 400, two chromosomes, all parameters fixed (so the binding can
    be put at the run's final parameters exactly): the file parses and matches ibd_moments /
    moment_sd to the %.10g printed; with --moments_window 50 the windows restart per chromosome;
    without the flag the set of output files and their bytes are those of a run without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast"]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_moments"])
    cli_util.run_cli(base + ["--out", w, "--ibd_moments", "--moments_window", 50])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.moments"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        for out, window in ((a, 0), (w, 50)):
            regions = summary_util.chrom_regions(chrom, window)
            ns, mb = h.ibd_moments(regions), h.ibd_moments(regions, length="mb")
            sn, sm = pkg.moment_sd(ns), pkg.moment_sd(mb)
            lines = open(out + ".ibd.moments").read().split("\n")
            assert lines[0] == "ind\tchr\tfirst_pos\tlast_pos\tn_sites\texp_ibd_sites\tsd_ibd_sites\texp_tracts\t" \
                               "sd_tracts\tcorr_sites_tracts\texp_ibd_mb\tsd_ibd_mb\tcorr_mb_tracts"
            assert lines[-1] == "" and len(lines) == 2 + I * len(regions)
            assert len(regions) == (2 if not window else 8)
            k = 1
            for i in range(I):
                for r, (lo, hi) in enumerate(regions):
                    f = lines[k].split("\t")
                    k += 1
                    assert f[:5] == [f"ind{i}", chrom[lo], str(pos[lo]), str(pos[hi - 1]), str(int(hi - lo))]
                    want = (ns["mean_a"][i, r], sn["sd_a"][i, r], ns["mean_t"][i, r], sn["sd_t"][i, r],
                            sn["corr"][i, r], mb["mean_a"][i, r], sm["sd_a"][i, r], sm["corr"][i, r])
                    for text, v in zip(f[5:], want):
                        if np.isnan(v):
                            assert text == "NA"
                            continue
                        assert text == "%.10g" % float(text)
                        assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[k - 1], v)
