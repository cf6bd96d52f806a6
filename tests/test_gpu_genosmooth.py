"""The smoothed genotype posteriors on the device (nghmm_geno_smooth / nghmm_chain_geno_smooth,
include/nghmm.h) against yardstick B of tests/genosmooth_util.py (np.longdouble on the log-space
weights of freqinfo_util.freq_info_b), which tests/test_genosmooth_cpu.py checks against
enumeration over all paths.

Tolerance: 16 x the spread of the two yardsticks on this cohort, per field and in the measure of
genosmooth_util.spread -- |device - B| absolute for post, over the sum of the absolute values of
the entry's terms for the sums -- as tests/test_genosmooth_cpu.py measures it
(genosmooth_util.SPREAD).  Every entry must be finite and every site and cell is compared."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import cli_util
import freqinfo_util as fu
import genosmooth_util as gu
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

SITE_KEYS = gu.SITE_FIELDS
REGION_KEYS = tuple(gu._key(f) for f in gu.REGION_FIELDS)


@pytest.fixture(scope="module")
def cohort(pkg):
    return fu.gpu_cohort(pkg)


@pytest.fixture(scope="module")
def yardstick(pkg, cohort):
    """B on the cohort with one region per chromosome: computed once, shared, left unchanged."""
    d, gl, F, A, freq = cohort
    return gu.geno_smooth_b(np.exp(gl), d.pos_dist_mb, F, A, freq, pkg.chromosome_regions(d.pos_dist_mb))


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


def _bytes(res):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in res.items()}


def _check(got, want, keys, what, where=None):
    """Every field of keys: finite on both sides and within TOL; prints the figures first."""
    err = gu.spread({k: got[k] for k in keys}, want, where)
    print("\n  " + what + ": " + ", ".join(f"{k} {err[k]:.2e}/{gu.TOL[k]:.2e}" for k in keys))
    for k in keys:
        sel = where[k] if where is not None and k in where else Ellipsis
        assert np.isfinite(np.asarray(got[k])[sel]).all() and np.isfinite(np.asarray(want[k])[sel]).all(), (what, k)
        assert err[k] <= gu.TOL[k], (what, k, err[k], gu.TOL[k])


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_fields_match_the_yardstick(pkg, cohort, yardstick, mode):
    d, gl, F, A, freq = cohort
    pos, S, I = d.pos_dist_mb, d.n_sites, d.n_ind
    chrom = pkg.chromosome_regions(pos)
    assert I > 64 and I % 64 != 0 and S % 2048 != 0 and S > 2 * 2048 and len(chrom) == 3
    with _handle(pkg, cohort, mode) as h:
        res = h.geno_smooth(chrom, sites=True, post=True, call=True)
        assert res["post"].shape == (S, I, 3) and res["call"].shape == (S, I) and res["call"].dtype == np.uint8
        assert res["sites"].dtype == pkg.GENO_SITE_STAT_DTYPE and res["sites"].shape == (S,)
        assert res["regions"].dtype == pkg.GENO_REGION_STAT_DTYPE and res["regions"].shape == (I, 3)
        got = gu.as_dict(res)
        _check(got, yardstick, ("post",) + SITE_KEYS + REGION_KEYS, mode + " chromosomes")
        # the calls: B's on all cells but the near ties
        tie = gu.near_ties(yardstick["post"], gu.TOL["post"])
        assert tie.mean() < 1e-3
        assert np.array_equal(got["call"][~tie], yardstick["call"][~tie])
        assert set(np.unique(got["call"])) <= {0, 1, 2}
        # windows, and a hand-made set: a region across a multiple of 2048 and a chromosome start,
        # gaps between the regions
        hand = gu.hand_regions(pos)
        assert any(a < m < b and a < s < b for a, b in hand for m in (2048, 4096)
                   for s in np.flatnonzero(np.isinf(pos)))
        assert all(hand[k + 1][0] > hand[k][1] for k in range(len(hand) - 1))
        for what, regs in (("windows", pkg.window_regions(pos, 700)), ("hand-made", hand)):
            r2 = h.geno_smooth(regs, sites=False)
            assert set(r2) == {"regions"} and r2["regions"].shape == (I, len(regs))
            _check(gu.as_dict(r2), gu.region_sums(yardstick, regs), REGION_KEYS, f"{mode} {what}")
        # the helpers on the device's records
        out = pkg.het_outside_ibd(res["regions"])
        np.testing.assert_array_equal(out, res["regions"]["het"] / res["regions"]["non_ibd"])
        em = pkg.geno_em_freq(res["sites"], I)
        assert np.isfinite(em).all() and em.min() > 0 and em.max() < 1


def test_fisher_identity_with_freq_info(pkg, cohort, yardstick):
    """(a) through code the feature does not share: freq_info's site pass gives the score, the
    cell pass the site sums; score f (1 - f) = (n1 + 2 n2 - alt_ibd) - f (2 I - ibd) per site,
    within the two sides' own tolerances added."""
    d, gl, F, A, freq = cohort
    I = d.n_ind
    with _handle(pkg, cohort, "fast") as h:
        stats, _ = h.freq_info()
        st = h.geno_smooth()["sites"]
    yfi = fu.freq_info_b(np.exp(gl), d.pos_dist_mb, F, A, freq)
    v = freq * (1 - freq)
    lhs = stats["score"] * v
    rhs = (st["n1"] + 2 * st["n2"] - st["alt_ibd"]) - freq * (2 * I - st["ibd"])
    tol = fu.TOL["score"] * yfi["abs_score"] * v + \
        gu.TOL["n1"] * yardstick["abs_n1"] + 2 * gu.TOL["n2"] * yardstick["abs_n2"] + \
        gu.TOL["alt_ibd"] * yardstick["abs_alt_ibd"] + freq * gu.TOL["ibd"] * yardstick["abs_ibd"]
    err = np.abs(lhs - rhs)
    print(f"\n  largest |score f (1 - f) - site sums| {err.max():.2e} (its tolerance {tol[np.argmax(err)]:.2e}) "
          f"at a scale of {np.abs(lhs).max():.1f}")
    assert np.abs(stats["score"]).max() > 1
    assert (err <= tol).all()


def test_ibd_against_the_estep(pkg, cohort):
    """The smoothed IBD posterior is the E-step's at the same parameters, up to the snap of
    EM.cpp:184 (1e-5 per cell): per site against the sum of marg_prob, per region non_ibd against
    n_sites - post_sum of ibd_summary."""
    d, gl, F, A, freq = cohort
    I = d.n_ind
    regs = pkg.chromosome_regions(d.pos_dist_mb)
    with _handle(pkg, cohort, "fast") as h:
        h.estep()
        marg = h.marg_prob.copy()
        summ, _ = h.ibd_summary(regs, what="posterior", sites=False)
        res = h.geno_smooth(regs)
    err = np.abs(res["sites"]["ibd"] - marg.sum(axis=0))
    print(f"\n  largest |ibd - sum of marg_prob| {err.max():.2e} (allowed {I * 1e-5:.1e})")
    assert err.max() <= I * 1e-5
    n = (regs[:, 1] - regs[:, 0])[None, :]
    err = np.abs(res["regions"]["non_ibd"] - (n - summ["post_sum"]))
    assert (err <= n * 1e-5).all()


def test_packed_called_genotypes(pkg, cohort):
    """Called genotypes as 2-bit codes: post is exactly one-hot at every called cell and call is
    the code; missing cells lie strictly inside (0, 1); the sums are within TOL of B on exp(h.gl)."""
    d, gl, F, A, freq = cohort
    regs = pkg.chromosome_regions(d.pos_dist_mb)
    with _handle(pkg, cohort, "fast", called="packed") as h:
        p = np.exp(h.gl)
        res = h.geno_smooth(regs, post=True, call=True)
    hot = p.max(axis=2) == 1.0
    assert (p[hot].sum(axis=1) == 1.0).all() and hot.mean() > 0.5 and (~hot).sum() > 1000
    assert np.array_equal(res["post"][hot], p[hot])
    assert np.array_equal(res["call"][hot], np.argmax(p[hot], axis=1))
    inner = res["post"][~hot]
    assert (inner > 0).all() and (inner < 1).all()
    want = gu.geno_smooth_b(p, d.pos_dist_mb, F, A, freq, regs)
    _check(gu.as_dict(res), want, SITE_KEYS + REGION_KEYS, "packed")


def test_dead_cells(pkg, cohort):
    """Packed called genotypes with the frequency of three sites set to 0, 1, 0, each site a
    chromosome of its own (the walks stay defined): NaN in post, 3 in call and NaN in the sums
    exactly where yardstick B has them; everything else finite and within TOL."""
    d, gl, F, A, freq = cohort
    sites, values = (300, 2100, 4000), (0.0, 1.0, 0.0)
    pos, fr = d.pos_dist_mb.copy(), freq.copy()
    for s, x in zip(sites, values):
        pos[s] = pos[s + 1] = np.inf
        fr[s] = x
    d2 = dataclasses.replace(d, pos_dist_mb=pos)
    regs = np.array([(0, 250), (250, 2200), (2300, 3900), (3950, 5003)])
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST | pkg.GENO_PACKED) as h:
        h.load_raw(np.ascontiguousarray(d2.gl), pos, space=0, call_geno=True)
        h.set_params(F, A, fr)
        want = gu.geno_smooth_b(np.exp(h.gl), pos, F, A, fr, regs)
        res = h.geno_smooth(regs, post=True, call=True)
    got = gu.as_dict(res)
    dead = np.isnan(want["post"]).any(axis=2)
    assert dead.sum() >= 2 and set(np.flatnonzero(dead.any(axis=1))) <= set(sites)
    assert np.array_equal(np.isnan(got["post"]), np.isnan(want["post"]))
    assert np.array_equal(np.isnan(got["post"]).all(axis=2), dead)
    assert np.array_equal(got["call"] == 3, dead) and np.array_equal(want["call"] == 3, dead)
    tie = gu.near_ties(np.nan_to_num(want["post"]), gu.TOL["post"]) & ~dead
    assert tie.mean() < 1e-3
    assert np.array_equal(got["call"][~dead & ~tie], want["call"][~dead & ~tie])
    where = {"post": ~np.isnan(want["post"])}
    for k in SITE_KEYS + REGION_KEYS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert not np.isinf(got[k]).any(), k
        where[k] = ~np.isnan(want[k])
    assert np.isnan(want["n0"]).sum() >= 2 and np.isnan(want["het"]).sum() >= 2
    assert not np.isnan(got["het_prior"]).any() and not np.isnan(got["r_het_prior"]).any()
    _check(got, want, ("post",) + SITE_KEYS + REGION_KEYS, "dead cells", where)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_nothing_else_moves_and_the_same_bytes(pkg, cohort, mode):
    d = cohort[0]
    S, I = d.n_sites, d.n_ind
    regs = pkg.window_regions(d.pos_dist_mb, 700)
    with _handle(pkg, cohort, mode) as a, _handle(pkg, cohort, mode) as b:
        for h in (a, b):
            h.estep()
            h.viterbi()
        state = lambda h: (h.indF.tobytes(), h.alpha.tobytes(), h.freq.tobytes(), h.marg_prob.tobytes(),
                           h.ibd_tracts("viterbi").tobytes(), h.e_prob.tobytes())
        before = state(a)
        r1 = _bytes(a.geno_smooth(regs, sites=True, post=True, call=True))
        assert state(a) == before
        assert _bytes(a.geno_smooth(regs, sites=True, post=True, call=True)) == r1
        # whichever outputs are asked for: through the binding ...
        for kw in ({"regions": regs, "sites": False}, {"sites": True}, {"sites": False, "post": True},
                   {"sites": False, "call": True}, {"regions": regs, "call": True}):
            r = _bytes(a.geno_smooth(**kw))
            assert r and all(r[k] == r1[k] for k in r), kw
        # ... and through raw calls with NULLs
        L, R = a.lib, len(regs)
        u64p = C.POINTER(C.c_uint64)
        bg, en = (np.ascontiguousarray(regs[:, k]).astype(np.uint64) for k in (0, 1))
        out = {"regions": np.zeros((I, R), dtype=pkg.GENO_REGION_STAT_DTYPE),
               "sites": np.zeros(S, dtype=pkg.GENO_SITE_STAT_DTYPE), "post": np.zeros((S, I, 3)),
               "call": np.zeros((S, I), dtype=np.uint8)}
        ptr = {"regions": lambda x: C.c_void_p(x.ctypes.data), "sites": lambda x: C.c_void_p(x.ctypes.data),
               "post": lambda x: x.ctypes.data_as(C.POINTER(C.c_double)),
               "call": lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))}
        for k in out:
            args = [ptr[j](out[j]) if j == k else None for j in ("regions", "sites", "post", "call")]
            withr = k == "regions"
            assert L.nghmm_geno_smooth(a.handle, R if withr else 0, bg.ctypes.data_as(u64p) if withr else None,
                                       en.ctypes.data_as(u64p) if withr else None, *args) == 0, k
            assert out[k].tobytes() == r1[k], k
        assert state(a) == before
        for h in (a, b):
            h.iter_EM()
        for f in ("indF", "alpha", "freq", "marg_prob", "ind_lkl"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_results_follow_the_current_parameters(pkg, cohort):
    """After set_params the call answers for the new parameters: within the tolerance of yardstick
    B there, far from the old answer, and the bytes of a fresh handle at those parameters."""
    d, gl, F, A, freq = cohort
    rng = np.random.default_rng(7)
    F2, A2 = rng.uniform(0.05, 0.9, d.n_ind), rng.uniform(0.02, 1.5, d.n_ind)
    freq2 = np.clip(freq + rng.uniform(-0.04, 0.04, d.n_sites), 0.01, 0.99)
    regs = pkg.chromosome_regions(d.pos_dist_mb)
    want = gu.geno_smooth_b(np.exp(gl), d.pos_dist_mb, F2, A2, freq2, regs)
    with _handle(pkg, cohort, "fast") as h:
        h.estep()
        old = h.geno_smooth(regs, post=True, call=True)
        h.set_params(F2, A2, freq2)
        new = h.geno_smooth(regs, post=True, call=True)
    assert np.abs(new["post"] - old["post"]).max() > 1e-2
    assert np.abs(new["sites"]["ibd"] - old["sites"]["ibd"]).max() > 0.5
    _check(gu.as_dict(new), want, ("post",) + SITE_KEYS + REGION_KEYS, "new parameters")
    with _handle(pkg, cohort, "fast", F=F2, A=A2, freq=freq2) as g:
        assert _bytes(g.geno_smooth(regs, post=True, call=True)) == _bytes(new)


CUTS = ([0, 1877, 5003], [0, 1877, 3500, 5003])      # an odd site; both inside a chromosome


@pytest.fixture(scope="module")
def whole(pkg, cohort):
    """The single handle's answer with one region per chromosome and with windows."""
    d = cohort[0]
    with _handle(pkg, cohort, "fast") as h:
        return (h.geno_smooth(pkg.chromosome_regions(d.pos_dist_mb), post=True, call=True),
                h.geno_smooth(pkg.window_regions(d.pos_dist_mb, 700), sites=False))


@pytest.mark.parametrize("cuts", CUTS, ids=["two", "three"])
def test_chains(pkg, cohort, yardstick, whole, cuts):
    """Chains of 2 and 3 site shards, cut at an odd site and inside a chromosome: post, call and
    sites are the single handle's bytes; regions (a region across a cut is one region) within TOL
    of B and of the single handle; the same bytes on a second call."""
    d, gl, F, A, freq = cohort
    pos = d.pos_dist_mb
    chrom, win = pkg.chromosome_regions(pos), pkg.window_regions(pos, 700)
    starts = [int(s) for s in np.flatnonzero(np.isinf(pos))]
    assert cuts[-1] == d.n_sites and cuts[1] % 2 == 1
    assert all(abs(c - s) > 50 for c in cuts[1:-1] for s in starts)
    assert all(any(a < c < b for a, b in win) for c in cuts[1:-1])      # a window across every cut
    hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        ch = pkg.Chain(hs)
        got = ch.geno_smooth(chrom, post=True, call=True)
        assert _bytes(ch.geno_smooth(chrom, post=True, call=True)) == _bytes(got)
        gotw = ch.geno_smooth(win, sites=False)
    finally:
        for h in hs:
            h.close()
    for k in ("post", "call", "sites"):
        assert got[k].tobytes() == whole[0][k].tobytes(), (cuts, k)
    _check(gu.as_dict(got), yardstick, REGION_KEYS, f"chain {cuts} chromosomes")
    yw = gu.region_sums(yardstick, win)
    _check(gu.as_dict(gotw), yw, REGION_KEYS, f"chain {cuts} windows")
    # ... and of the single handle, in the same measure: only the grouping of a sum at a cut differs
    for single, chain, y in ((whole[0], got, yardstick), (whole[1], gotw, yw)):
        for f in gu.REGION_FIELDS:
            k = gu._key(f)
            err = np.abs(chain["regions"][f] - single["regions"][f]) / y["abs_" + k]
            print(f"  chain {cuts} against the single handle: {f} {err.max():.2e}/{gu.TOL[k]:.2e}")
            assert err.max() <= gu.TOL[k], (cuts, f, err.max())


def test_argument_errors(pkg, cohort):
    d = cohort[0]
    S, I = d.n_sites, d.n_ind
    u64p = C.POINTER(C.c_uint64)
    st = np.zeros(S, dtype=pkg.GENO_SITE_STAT_DTYPE)
    rg = np.zeros((I, 2), dtype=pkg.GENO_REGION_STAT_DTYPE)
    sp, rp = C.c_void_p(st.ctypes.data), C.c_void_p(rg.ctypes.data)
    u = lambda *v: np.array(v, dtype=np.uint64)
    up = lambda a: a.ctypes.data_as(u64p)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        with pytest.raises(pkg.NgsFHMMError) as ei:          # no data loaded
            h.geno_smooth()
        assert ei.value.code == -10 and "no data" in ei.value.message
    with _handle(pkg, cohort, "fast") as h:
        L = h.lib
        err = lambda: L.nghmm_last_error()
        assert L.nghmm_geno_smooth(h.handle, 0, None, None, None, None, None, None) == -10
        assert b"all NULL" in err()
        b, e = u(0, 100), u(50, 200)
        assert L.nghmm_geno_smooth(h.handle, 2, up(b), up(e), None, sp, None, None) == -10     # regions NULL
        assert b"NULL iff n_regions == 0" in err()
        assert L.nghmm_geno_smooth(h.handle, 0, None, None, rp, sp, None, None) == -10        # ... and the reverse
        assert b"NULL iff n_regions == 0" in err()
        for what, b, e in (("unsorted", u(100, 0), u(200, 50)), ("overlapping", u(0, 40), u(50, 200)),
                           ("empty", u(0, 60), u(50, 60)), ("end > S", u(0, 100), u(50, S + 1))):
            assert L.nghmm_geno_smooth(h.handle, 2, up(b), up(e), rp, sp, None, None) == -10, what
            assert b"region " in err() and b"sorted and do not overlap" in err(), what
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.geno_smooth(sites=False)
        assert ei.value.code == -10 and "all NULL" in ei.value.message
        assert L.nghmm_geno_smooth(None, 0, None, None, None, sp, None, None) == -10
        assert b"no data" in err()
        assert L.nghmm_chain_geno_smooth(None, 1, 0, None, None, None, sp, None, None) == -10
        b, e = u(0, 100), u(50, S)
        assert L.nghmm_geno_smooth(h.handle, 2, up(b), up(e), rp, sp, None, None) == 0
        # two handles that nghmm_chain_setup has not seen
        with _handle(pkg, cohort, "fast") as g:
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            assert L.nghmm_chain_geno_smooth(arr, 2, 0, None, None, None, sp, None, None) == -10
            assert b"nghmm_chain_setup" in err()


def _g10(v):
    return "NA" if v != v else "%.10g" % v


def test_cli_geno_smooth(pkg, tmp_path):
    """ngsF-HMM --geno_smooth --geno_summary on a chain of two with all parameters fixed (so the
    binding can be put at the run's final parameters exactly): PREFIX.geno.smooth is the binding's
    post, the two text files are the text made from the binding's records, with and without
    --geno_window; the other output files are those of a run without the flags, and the flags add
    exactly the new files."""
    I, S = 12, 3001
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast", "--n_gpus", 2,
            "--devices", "0,0", "--ibd_bed"]
    plain, a, b = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "b")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--geno_smooth", "--geno_summary"])
    cli_util.run_cli(base + ["--out", b, "--geno_summary", "--geno_window", 500])
    for ext in (".indF", ".ibd", ".geno", ".ibd.bed"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
        assert open(plain + ext, "rb").read() == open(b + ext, "rb").read(), ext
    files = lambda tag: sorted(f[len(tag):] for f in os.listdir(tmp_path) if f.startswith(tag + "."))
    assert files("a") == sorted(files("plain") + [".geno.smooth", ".geno.regions", ".geno.sites"])
    assert files("b") == sorted(files("plain") + [".geno.regions", ".geno.sites"])
    # the same through the binding: a chain cut where the host cuts (multiples of 16 sites)
    cut = S // 2 // 16 * 16
    regs = {"a": pkg.chromosome_regions(d.pos_dist_mb), "b": pkg.window_regions(d.pos_dist_mb, 500)}
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
        res = {"a": ch.geno_smooth(regs["a"], post=True), "b": ch.geno_smooth(regs["b"])}
    finally:
        for h in hs:
            h.close()
    assert open(a + ".geno.smooth", "rb").read() == res["a"]["post"].tobytes()
    for tag, prefix in (("a", a), ("b", b)):
        rg, st = res[tag]["regions"], res[tag]["sites"]
        out = pkg.het_outside_ibd(rg)
        want = ["\t".join(["ind", "chr", "first_pos", "last_pos", "n_sites", "het", "het_prior", "non_ibd",
                           "het_out", "dosage"])]
        for i in range(I):
            for r, (lo, hi) in enumerate(regs[tag]):
                want.append("\t".join([f"ind{i}", f"chr{int(d.chrom[lo])}", str(int(d.pos[lo])),
                                       str(int(d.pos[hi - 1])), str(hi - lo)] +
                                      [_g10(float(v)) for v in (rg["het"][i, r], rg["het_prior"][i, r],
                                                                rg["non_ibd"][i, r], out[i, r], rg["dosage"][i, r])]))
        got = open(prefix + ".geno.regions").read().split("\n")
        assert got[-1] == "" and got[:-1] == want, tag
        em = pkg.geno_em_freq(st, I)
        want = ["\t".join(["chr", "pos", "n0", "n1", "n2", "het_prior", "ibd", "em_freq"])]
        for s in range(S):
            want.append("\t".join([f"chr{int(d.chrom[s])}", str(int(d.pos[s]))] +
                                  [_g10(float(v)) for v in (st["n0"][s], st["n1"][s], st["n2"][s],
                                                            st["het_prior"][s], st["ibd"][s], em[s])]))
        got = open(prefix + ".geno.sites").read().split("\n")
        assert got[-1] == "" and len(got) == S + 2 and got[:-1] == want, tag
    assert len(regs["b"]) > len(regs["a"]) == 2
