"""Exact expectations over IBD paths on the device (nghmm_ibd_expect / nghmm_chain_ibd_expect,
include/nghmm.h) against brute-force enumeration and against yardstick B of tests/expect_util.py
(log space, np.longdouble), which tests/test_expect_cpu.py checks against enumeration.

Tolerance.  The two yardsticks A and B differ on the 20 x 5003 cohort by at most
(tests/test_expect_cpu.py measures and prints the figures; expect_util.REGION_SPREAD / SITE_SPREAD
hold them)
    regions: ibd 1.09e-11, starts 9.3e-14, switches 9.8e-14, ibd_mb 1.02e-12, entropy 6.2e-13,
             log_p_path 2.4e-12;   sites: on 5.3e-14, off 5.6e-14, ibd 1.2e-13, entropy 2.7e-13
over all region sets -- the spread of two correct restatements.  The tolerance is 16 x the spread
per field, support_util's rule and margin (the device groups and rescales its products unlike
either restatement); nothing in it comes from a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cli_util
import expect_util as xu
import genosmooth_util as gu
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# Enumeration over 2^12 paths in float64 agrees with two independent restatements to 2e-13
# (tests/test_expect_cpu.py); the device's emissions reach the host through a logarithm and go
# back through an exponential (1e-16 per site, twelve sites): 1e-12 bounds both with a margin of 4.
ENUM_TOL = 1e-12


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


def _handle(pkg, cohort, mode, called=None, sites=None):
    d, gl, F, A, freq = cohort
    lo, hi = sites or (0, d.n_sites)
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | (pkg.GENO_PACKED if called == "packed" else 0)
    h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=m)
    pos = np.ascontiguousarray(d.pos_dist_mb[lo:hi])
    if called:
        h.load_raw(np.ascontiguousarray(d.gl[lo:hi]), pos, space=0, call_geno=True)
    else:
        h.load(np.ascontiguousarray(gl[lo:hi]), pos)
    h.set_params(F, A, freq)
    h.init_emission()
    return h


def _check_regions(got, want, tol, tag):
    for f in xu.REGION_FIELDS:
        assert not np.isnan(got[f]).any(), (tag, f)
        inf = np.isneginf(want[f])
        assert np.array_equal(np.isneginf(got[f]), inf), (tag, f, "-inf exactly where the yardstick has it")
        err = np.abs(got[f][~inf] - want[f][~inf])
        t = tol[f] if isinstance(tol, dict) else tol
        print(f"  {tag:9s} {f:10s}: largest |device - yardstick| = {err.max() if err.size else 0:.3e} (tol {t:.3e})")
        assert (err <= t).all(), (tag, f, err.max())


def _check_sites(got, want, tol, tag):
    for f in xu.SITE_FIELDS:
        assert np.isfinite(got[f]).all(), (tag, f)
        err = np.abs(got[f] - want[f])
        t = tol[f] if isinstance(tol, dict) else tol
        print(f"  {tag:9s} site {f:7s}: largest |device - yardstick| = {err.max():.3e} (tol {t:.3e})")
        assert (err <= t).all(), (tag, f, err.max())


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths: single-site regions give every cell's terms, the whole data
    the identities (E[n_tracts], E[ibd_sites], E[ibd_mb], E[switches], H, ln P(path | y)); two
    chromosomes, a missing cell, a cell whose IBD state is excluded."""
    _, pos, F, A, _, gl, freq = xu.small_case()
    I, S = gl.shape[1], gl.shape[0]
    gl = np.where(np.isneginf(gl), -1e15, gl)          # (the reader's likelihood of an excluded genotype)
    m = pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load(np.ascontiguousarray(gl), pos)
        h.set_params(F, A, freq)
        h.init_emission()
        path = h.viterbi()
        e = h.e_prob
        assert np.isneginf(e[1, 4, 1]) or e[1, 4, 1] < -1e14
        tot, want = xu.enumerate_expect(e, pos, F, A, path)
        assert not np.isnan(want["lp"]).any()           # (the decode avoids the excluded state)
        one, whole = xu.single_site_regions(S), np.array([[0, S]])
        print()
        reg, sites = h.ibd_expect(one, viterbi=True)
        assert reg.dtype == pkg.EXPECT_REGION_DTYPE and reg.shape == (I, S)
        assert sites.dtype == pkg.EXPECT_SITE_DTYPE and sites.shape == (S,)
        _check_regions(reg, xu.region_records(want, one), ENUM_TOL, "cells")
        _check_sites(sites, xu.site_records(want), ENUM_TOL, "cells")
        assert reg["ibd"][1, 4] == 0.0 and reg["starts"][1, 4] == 0.0
        regw, _ = h.ibd_expect(None, viterbi=True)
        for f, k in (("starts", "n_tracts"), ("ibd", "ibd_sites"), ("ibd_mb", "ibd_mb"),
                     ("switches", "switches"), ("entropy", "entropy"), ("log_p_path", "log_p_path")):
            err = np.abs(regw[f][:, 0] - tot[k])
            print(f"  whole     {f:10s}: largest |device - enumeration| = {err.max():.3e}")
            assert (err <= ENUM_TOL).all(), (f, err.max())
        assert (h.ibd_expect(None)[0]["log_p_path"] == 0).all()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_parity_with_the_yardstick(pkg, cohort, mode):
    """20 x 5003 against yardstick B within 16 x spread: the chromosomes; windows of 7, 64, 2048
    and 2049 sites; single sites on both sides of every lane-chunk boundary; a region across a
    chromosome start among regions with gaps; the whole data; with the Viterbi term."""
    d = cohort[0]
    pos = d.pos_dist_mb
    with _handle(pkg, cohort, mode) as h:
        T = h.layout()[1] or xu.SPREAD_LANE_SITES
        path = h.viterbi()
        want = xu.terms_b(h.e_prob, pos, h.indF, h.alpha, path)
        sets = xu.region_sets(d.n_sites, pos, T)
        cs = int([x for x in np.flatnonzero(np.isinf(pos)) if x > 0][0])
        assert ((sets["gaps"][:, 0] < cs) & (sets["gaps"][:, 1] > cs)).any()
        if mode == "fast":
            bounds = np.arange(T, d.n_sites, T)
            assert np.isin(bounds, sets["edges"][:, 0]).all() and np.isin(bounds - 1, sets["edges"][:, 0]).all()
            assert len(bounds) > 10
        print()
        wsites = xu.site_records(want)
        for tag, reg in sets.items():
            got, sites = h.ibd_expect(reg, viterbi=True)
            _check_regions(got, xu.region_records(want, reg), xu.REGION_TOL, tag)
            assert (got["entropy"] >= 0).all() and (got["log_p_path"] <= 0).all()
        _check_sites(sites, wsites, xu.SITE_TOL, "all")
        whole = h.ibd_expect(None)[0]
        n_sites, n_mb = pkg.expect_tract_length(whole)
        assert np.isfinite(n_sites).all() and (n_mb > 0).all()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_packed_called_genotypes(pkg, mode):
    """8 x 300 called genotypes as 2-bit codes: at every called heterozygote the IBD state is
    excluded and ibd of the single-site region is exactly 0.0; no NaN anywhere; entropy >= 0."""
    I, S = 8, 300
    d = pkg.simulate.simulate(I, S, seed=5, n_chrom=2, indF=0.4, alpha=0.1)
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | pkg.GENO_PACKED
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=True)
        h.set_params(0.4, 0.1, 0.2)
        h.init_emission()
        h.viterbi()
        e = h.e_prob
        het = e[..., 1] < -1e14                     # (-inf in fast mode, the reader's -1e15 in exact mode)
        assert het.sum() > 50 and not (e[..., 0] < -1e14).any()
        reg, sites = h.ibd_expect(xu.single_site_regions(S), viterbi=True)
        assert (reg["ibd"][het] == 0.0).all() and (reg["starts"][het] == 0.0).all()
        assert (reg["ibd"][~het] > 0.0).any()
        for f in xu.REGION_FIELDS:
            assert not np.isnan(reg[f]).any(), f
        for f in xu.SITE_FIELDS:
            assert np.isfinite(sites[f]).all(), f
        assert (reg["entropy"] >= 0).all() and (sites["entropy"] >= 0).all()
        assert np.isfinite(reg["log_p_path"]).all()     # (the decode avoids excluded states)
        whole, _ = h.ibd_expect(None, sites=False, viterbi=True)
        np.testing.assert_allclose(whole["ibd"][:, 0], reg["ibd"].sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(whole["log_p_path"][:, 0], reg["log_p_path"].sum(axis=1), rtol=1e-12)


def test_same_bits_and_nothing_else_moves(pkg, cohort):
    d = cohort[0]
    regions = pkg.window_regions(d.pos_dist_mb, 777)
    none = np.zeros((0, 2), dtype=np.int64)

    def run(with_call):
        out = {}
        with _handle(pkg, cohort, "fast") as h:
            h.iter_EM(1)
            h.viterbi()
            out["before"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ibd_tracts("viterbi"))
            if with_call:
                a, b = h.ibd_expect(regions, viterbi=True), h.ibd_expect(regions, viterbi=True)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                # regions alone, sites alone and both: the same bytes for what they share
                r_only = h.ibd_expect(regions, sites=False, viterbi=True)
                s_only = h.ibd_expect(none, viterbi=True)
                assert r_only[1] is None and s_only[0] is None
                assert r_only[0].tobytes() == a[0].tobytes() and s_only[1].tobytes() == a[1].tobytes()
                # a region's record does not depend on the other regions of the call
                few = h.ibd_expect(regions[3:5], sites=False, viterbi=True)[0]
                assert few.tobytes() == np.ascontiguousarray(a[0][:, 3:5]).tobytes()
                # ... nor, but for log_p_path, on the Viterbi term
                plain = h.ibd_expect(regions)
                for f in xu.REGION_FIELDS[:-1]:
                    assert plain[0][f].tobytes() == a[0][f].tobytes(), f
                assert plain[1].tobytes() == a[1].tobytes() and not plain[0]["log_p_path"].any()
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


def test_cross_checks_against_existing_calls(pkg, cohort):
    """sites["ibd"] against geno_smooth's ibd and single-site regions["ibd"] against
    tract_support's post_min on one-site ranges, at the tolerances those features' tests use."""
    d = cohort[0]
    S, I = d.n_sites, d.n_ind
    with _handle(pkg, cohort, "fast") as h:
        _, sites = h.ibd_expect(np.zeros((0, 2), dtype=np.int64))
        gs = h.geno_smooth(None)["sites"]["ibd"]
        err = np.abs(sites["ibd"] - gs) / np.abs(gs)          # (genosmooth_util.spread's measure)
        print(f"\n  sites ibd against geno_smooth: {err.max():.3e} (tol {gu.TOL['ibd']:.3e})")
        assert err.max() <= gu.TOL["ibd"]
        lo = 1000
        one = np.stack([np.arange(lo, lo + 600), np.arange(lo, lo + 600) + 1], axis=1)
        reg, _ = h.ibd_expect(one, sites=False)
        for i in (0, 7, 19):
            sc = h.tract_support(np.array([(i, s, 1) for s in range(lo, lo + 600)], dtype=np.int64))
            err = np.abs(reg["ibd"][i] - sc["post_min"])
            print(f"  regions ibd against tract_support, individual {i}: {err.max():.3e} (tol {sup.POST_TOL:.3e})")
            assert err.max() <= sup.POST_TOL


def test_against_the_sampler(pkg, cohort):
    """sample_paths(400, seed) on the cohort: the cohort totals of the draw means of n_tracts,
    ibd_sites and ibd_mb within 5 standard errors (from the draws) of the exact totals, the same
    per individual whose draws vary, at most 5 of 20 individuals without variance per statistic
    (expect_util.sampler_check; tests/test_expect_cpu.py checks the condition on the restatement)."""
    with _handle(pkg, cohort, "fast") as h:
        stats, _ = h.sample_paths(xu.SAMPLER_DRAWS, seed=xu.SAMPLER_SEED)
        exact = h.ibd_expect(None, sites=False)[0][:, 0]
    worst = xu.sampler_check(stats, exact)
    print(f"\n  device sampler against the exact means: largest |z| = {worst:.2f}")


def test_chain_against_one_handle(pkg, cohort):
    """The same data on 1 handle and as 3 site shards, cuts inside a chromosome and inside a
    region: regions and sites within 16 x spread of the single handle, sites of full length, the
    Viterbi term correct across a cut."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    cuts = [0, 1203, 3907, S]
    starts = np.flatnonzero(np.isinf(pos))
    assert not np.isin(cuts[1:-1], starts).any()
    with _handle(pkg, cohort, "fast") as whole:
        wpath = whole.viterbi()
        sets = xu.region_sets(S, pos, whole.layout()[1])
        want = {k: whole.ibd_expect(sets[k], viterbi=True) for k in ("whole", "chrom", "win2048", "gaps", "win7")}
    hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        ch = pkg.Chain(hs)
        with pytest.raises(pkg.NgsFHMMError) as ei:       # no decode yet
            ch.ibd_expect(None, viterbi=True)
        assert ei.value.code == -10 and "Viterbi" in ei.value.message
        assert np.array_equal(ch.viterbi(), wpath)
        across = [int(((wpath[:, c - 1] == 1) & (wpath[:, c] == 1)).sum()) for c in cuts[1:-1]]
        print(f"\n  decoded IBD runs across the cuts {cuts[1:-1]}: {across} individuals")
        for k, (wreg, wsites) in want.items():
            inside = [((sets[k][:, 0] < c) & (sets[k][:, 1] > c)).any() for c in cuts[1:-1]]
            assert all(inside) or k in ("gaps", "win7")
            reg, sites = ch.ibd_expect(sets[k], viterbi=True)
            assert sites.shape == (S,) and reg.shape == wreg.shape
            _check_regions(reg, wreg, xu.REGION_TOL, k)
            _check_sites(sites, wsites, xu.SITE_TOL, k)
        a, b = ch.ibd_expect(sets["chrom"], viterbi=True), ch.ibd_expect(sets["chrom"], viterbi=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        for h in hs:
            h.close()


def _raw(h, what, begin, end, regions=True, sites=True, n=None):
    u64 = C.POINTER(C.c_uint64)
    b, e = np.array(begin, dtype=np.uint64), np.array(end, dtype=np.uint64)
    n = len(b) if n is None else n
    rbuf = C.create_string_buffer(48 * h.n_ind * max(n, 1))
    sbuf = C.create_string_buffer(32 * h.n_sites)
    rc = h.lib.nghmm_ibd_expect(h.handle, what, n, b.ctypes.data_as(u64) if len(b) else None,
                                e.ctypes.data_as(u64) if len(e) else None,
                                C.cast(rbuf, C.c_void_p) if regions else None,
                                C.cast(sbuf, C.c_void_p) if sites else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg):
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=3, n_chrom=2)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, 0, [0], [S])                          # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_expect(None)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        with pytest.raises(pkg.NgsFHMMError) as ei:             # the Viterbi bit without a decode
            h.ibd_expect(None, viterbi=True)
        assert ei.value.code == -10 and "Viterbi" in ei.value.message
        assert _raw(h, 0, [0], [S])[0] == 0
        h.viterbi()
        assert _raw(h, 1, [0], [S])[0] == 0
        bad = [
            ((2, [0], [S]), {}),                                # an unknown bit
            ((1 | 4, [0], [S]), {}),
            ((0, [10, 5], [20, 8]), {}),                        # unsorted
            ((0, [0, 9], [10, 20]), {}),                        # overlapping
            ((0, [0, 10], [10, 10]), {}),                       # empty
            ((0, [0], [S + 1]), {}),                            # end > S
            ((0, [0], [S]), {"regions": False}),                # NULL mismatch
            ((0, [], []), {"regions": True, "n": 0}),
            ((0, [], []), {"regions": False, "sites": False, "n": 0}),   # all outputs NULL
        ]
        for args, kw in bad:
            rc, msg = _raw(h, *args, **kw)
            assert rc == -10 and msg, (args, kw, rc, msg)
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_expect(np.array([[10, 20], [5, 8]]))
        assert ei.value.code == -10 and ei.value.message
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_expect(np.array([[0.0, 5.0]]))
        assert _raw(h, 0, [0, 10], [10, S])[0] == 0             # touching regions do not overlap
        h.load(gl, d.pos_dist_mb)                               # a reload forgets the decode
        rc, msg = _raw(h, 1, [0], [S])
        assert rc == -10 and "Viterbi" in msg


def test_cli_ibd_expect(pkg, tmp_path):
    """ngsF-HMM --ibd_expect at 6 x 400, two chromosomes, all parameters fixed (so the binding can
    be put at the run's final parameters exactly): both files parse and match ibd_expect to the
    %.10g printed; with --expect_window 50 the windows restart per chromosome; without the flag
    the set of output files and their bytes are those of a run without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast"]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_expect"])
    cli_util.run_cli(base + ["--out", w, "--ibd_expect", "--expect_window", 50])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.expect", ".ibd.breaks"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        h.viterbi()
        for out, window in ((a, 0), (w, 50)):
            regions = summary_util.chrom_regions(chrom, window)
            assert np.array_equal(regions, pkg.window_regions(d.pos_dist_mb, window) if window
                                  else pkg.chromosome_regions(d.pos_dist_mb))
            reg, sites = h.ibd_expect(regions, viterbi=True)
            lines = open(out + ".ibd.expect").read().split("\n")
            assert lines[0] == "ind\tchr\tfirst_pos\tlast_pos\tn_sites\texp_ibd_sites\texp_tracts\t" \
                               "exp_switches\texp_ibd_mb\tentropy\tlog10_p_path"
            assert lines[-1] == "" and len(lines) == 2 + I * len(regions)
            assert len(regions) == (2 if not window else 8)
            k = 1
            for i in range(I):
                for r, (lo, hi) in enumerate(regions):
                    f = lines[k].split("\t")
                    k += 1
                    assert f[:5] == [f"ind{i}", chrom[lo], str(pos[lo]), str(pos[hi - 1]), str(int(hi - lo))]
                    t = reg[i, r]
                    want = (t["ibd"], t["starts"], t["switches"], t["ibd_mb"], t["entropy"],
                            t["log_p_path"] / math.log(10.0))
                    for text, v in zip(f[5:], want):
                        assert text == "%.10g" % float(text)
                        assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[k - 1], v)
            lines = open(out + ".ibd.breaks").read().split("\n")
            assert lines[0] == "chr\tpos\ton\toff\tibd\tentropy" and lines[-1] == "" and len(lines) == 2 + S
            for s in range(S):
                f = lines[1 + s].split("\t")
                assert f[:2] == [chrom[s], str(pos[s])]
                for text, v in zip(f[2:], (sites["on"][s], sites["off"][s], sites["ibd"][s], sites["entropy"][s])):
                    assert text == "%.10g" % float(text)
                    assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[1 + s], v)
