"""Expected IBD above a minimum tract length on the device (nghmm_ibd_by_length /
nghmm_chain_ibd_by_length, include/nghmm.h) against brute-force enumeration and against yardstick
B of tests/bylength_util.py (np.longdouble, log space), which tests/test_bylength_cpu.py checks
against enumeration.

Tolerance.  The two yardsticks A (float64 running products) and B differ on the 20 x 5003 cohort,
over all region sets and the thresholds 1, 2, 8, 80, 81, 400, 2000 sites / 0, 0.05, 0.5, 2, 10 Mb,
by at most (tests/test_bylength_cpu.py measures and prints the figures; bylength_util.SPREAD holds
them)
    sites: tracts 9.3e-14, length 9.7e-11        mb: tracts 9.3e-14, length 9.6e-12
-- the spread of two correct restatements.  The tolerance is 16 x the spread per unit and field,
the project's rule and margin (expect_util.REGION_TOL: the device groups and rescales its products
unlike either restatement); nothing in it comes from a device.  The yardstick runs once on the
emissions numpy makes of the likelihoods and the frequency, and is shared by the tests."""
import ctypes as C
import os

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import expect_util as xu
import sample_util as su
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# Enumeration over 2^12 paths in float64 agrees with both restatements to 4e-15
# (tests/test_bylength_cpu.py); the device's emissions reach the host through a logarithm and go
# back through an exponential (1e-16 per site, twelve sites; lengths of the order of 10): 1e-12,
# as tests/test_gpu_expect.py.
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
    reports (both modes get the same sets), {unit: terms [I][S][K]} at COHORT_LEN, and the per-site
    posterior of the IBD state.  ("lane": T and T + 1 sites for the layout's own lane length T.)"""
    d, gl, F, A, freq = cohort
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    with _handle(pkg, cohort, "fast") as h:
        T = h.layout()[1]
    assert T > 0
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    terms = {u: bu.terms_b(e, d.pos_dist_mb, F, A, bu.COHORT_LEN[u], u) for u in UNITS}
    # ... and the thresholds that straddle the lane length of THIS layout, whatever it is
    terms["lane"] = bu.terms_b(e, d.pos_dist_mb, F, A, (T, T + 1), "sites")
    post = xu.terms_b(e, d.pos_dist_mb, F, A)["ibd"]
    return sets, terms, post, e


def _check(got, want, tol, tag):
    for f in bu.FIELDS:
        assert np.isfinite(got[f]).all(), (tag, f)
        err = np.abs(got[f] - want[f])
        t = tol[f] if isinstance(tol, dict) else tol
        print(f"  {tag:16s} {f:7s}: largest |device - yardstick| = {err.max():.3e} (tol {t:.3e})")
        assert (err <= t).all(), (tag, f, err.max())


@pytest.mark.parametrize("mode", MODES)
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths, both units: the whole data; every single start site against
    yardstick B; a missing cell, an excluded state (exact zeros)."""
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
        # (exact mode reports the excluded state's emission as the reader's -1e15: a probability of
        # exactly 0 either way, which the yardstick's prefix sums need spelt as -inf -- 1e15 in a sum
        # costs them eleven digits)
        e = np.where(e < -1e14, -np.inf, e)
        print()
        for unit in UNITS:
            L = bu.SMALL_LEN[unit]
            got = h.ibd_by_length(L, unit=unit)
            assert got.dtype == pkg.BYLENGTH_DTYPE and got.shape == (I, 1, len(L))
            tr, ln = bu.enumerate_by_length(e, pos, F, A, L, unit)
            want = np.zeros((I, 1, len(L)), dtype=bu.DTYPE)
            want["tracts"][:, 0], want["length"][:, 0] = tr, ln
            _check(got, want, ENUM_TOL, f"{unit} whole")
            assert got.tobytes() == h.ibd_by_length(L, unit=unit, regions=np.array([[0, S]])).tobytes()
            one = h.ibd_by_length(L, unit=unit, regions=xu.single_site_regions(S))
            _check(one, bu.region_records(bu.terms_b(e, pos, F, A, L, unit), xu.single_site_regions(S)),
                   ENUM_TOL, f"{unit} cells")
            assert (one["tracts"][1, 4] == 0.0).all() and (one["length"][1, 4] == 0.0).all()
            for k, l in enumerate(L):      # one threshold alone is the same record
                assert h.ibd_by_length(l, unit=unit).tobytes() == got[:, :, k:k + 1].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_yardstick(pkg, cohort, cohort_want, mode):
    """20 x 5003 against yardstick B within 16 x spread, both units, seven and five thresholds (80
    and 81 sites straddle a lane length of 80, and T and T + 1 sites are added for the layout's
    own lane length T; 2000 sites exceed every chromosome: exactly 0): the
    chromosomes; windows of 7, 64, 2048 and 2049 sites; single sites on both sides of every
    lane-chunk edge; a region across a chromosome start among regions with gaps; the whole data."""
    d = cohort[0]
    sets, terms, _, _ = cohort_want
    with _handle(pkg, cohort, mode) as h:
        T = int(sets["edges"][1, 1])                  # (the lane length the sets were made for)
        assert mode != "fast" or h.layout()[1] == T
        print()
        for unit in UNITS:
            for tag, reg in sets.items():
                got = h.ibd_by_length(bu.COHORT_LEN[unit], unit=unit, regions=reg)
                _check(got, bu.region_records(terms[unit], reg), bu.TOL[unit], f"{unit} {tag}")
                if unit == "sites":
                    assert (got["tracts"][..., -1] == 0).all() and (got["length"][..., -1] == 0).all()
        for tag in ("whole", "edges", "win7"):
            got = h.ibd_by_length((T, T + 1), regions=sets[tag])
            _check(got, bu.region_records(terms["lane"], sets[tag]), bu.TOL["sites"], f"lane {tag}")
        print(f"  largest |Q| met: {h.by_length_qmax():.1f}")


@pytest.mark.parametrize("mode", MODES)
def test_identities(pkg, cohort, mode):
    """Against the device's own ibd_expect: tracts at L = 1 site (and at 0 Mb) is starts per
    region; over the chromosomes length is ibd (1 site) and ibd_mb (0 Mb); both fields are
    non-increasing in k; length >= L_k tracts."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    with _handle(pkg, cohort, mode) as h:
        sets = xu.region_sets(S, pos, h.layout()[1] or xu.SPREAD_LANE_SITES)
        print()
        for tag in ("whole", "chrom", "win64", "gaps", "edges"):
            ex = h.ibd_expect(sets[tag], sites=False)[0]
            for unit, fl in (("sites", "ibd"), ("mb", "ibd_mb")):
                L = np.asarray(bu.COHORT_LEN[unit])
                got = h.ibd_by_length(L, unit=unit, regions=sets[tag])
                tol = bu.TOL[unit]
                err = np.abs(got["tracts"][..., 0] - ex["starts"]).max()
                print(f"  {unit:5s} {tag:6s} tracts against ibd_expect's starts: {err:.3e}")
                assert err <= tol["tracts"] + xu.REGION_TOL["starts"]
                if tag in ("whole", "chrom"):
                    err = np.abs(got["length"][..., 0] - ex[fl]).max()
                    print(f"  {unit:5s} {tag:6s} length against ibd_expect's {fl}: {err:.3e}")
                    assert err <= tol["length"] + xu.REGION_TOL[fl]
                for f in bu.FIELDS:      # (two records, each within its tolerance)
                    assert (np.diff(got[f], axis=-1) <= 2 * tol[f]).all(), (unit, tag, f)
                assert (got["tracts"] >= 0).all() and (got["length"] >= 0).all()
                assert (got["length"] >= L * got["tracts"] - tol["length"] - L * tol["tracts"]).all()


@pytest.mark.parametrize("mode", MODES)
def test_packed_called_genotypes(pkg, mode):
    """8 x 300 called genotypes as 2-bit codes: everything finite; no tract begins on a called
    heterozygote (the IBD state is excluded): exact zeros."""
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
            one = h.ibd_by_length(L, unit=unit, regions=xu.single_site_regions(S))
            whole = h.ibd_by_length(L, unit=unit)
            for f in bu.FIELDS:
                assert np.isfinite(one[f]).all() and np.isfinite(whole[f]).all(), (unit, f)
                assert (one[f][het] == 0.0).all() and (one[f][~het] > 0.0).any()
                np.testing.assert_allclose(whole[f][:, 0], one[f].sum(axis=1), rtol=1e-12, atol=1e-300)
            st = h.ibd_expect(None, sites=False)[0]["starts"][:, 0]
            np.testing.assert_allclose(whole["tracts"][:, 0, 0], st, rtol=1e-11)


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
                for unit in UNITS:
                    L = bu.COHORT_LEN[unit]
                    a, b = h.ibd_by_length(L, unit, regions), h.ibd_by_length(L, unit, regions)
                    assert a.tobytes() == b.tobytes()
                    h.ibd_by_length(L, unit)
                    assert h.ibd_by_length(L, unit, regions).tobytes() == a.tobytes()
                    # a region's record does not depend on which other regions are asked for
                    assert h.ibd_by_length(L, unit, regions[2:3]).tobytes() == a[:, 2:3].tobytes()
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
    """sample_paths(400, seed 77, all paths kept) on the cohort, the paths reduced with
    path_by_length, under bylength_util.sampler_check at SAMPLER_LEN (tests/test_bylength_cpu.py
    checks the condition on the restatement of the sampler)."""
    d = cohort[0]
    with _handle(pkg, cohort, "fast") as h:
        _, paths = h.sample_paths(xu.SAMPLER_DRAWS, seed=xu.SAMPLER_SEED, keep=xu.SAMPLER_DRAWS)
        exact = {u: h.ibd_by_length(bu.SAMPLER_LEN[u], unit=u)[:, 0] for u in UNITS}
    assert paths.shape == (xu.SAMPLER_DRAWS, d.n_ind, d.n_sites)
    print()
    for u in UNITS:
        tr, ln = bu.path_by_length(paths, d.pos_dist_mb, bu.SAMPLER_LEN[u], u)
        worst = bu.sampler_check(tr, ln, exact[u], u)
        print(f"  device sampler against the exact values in {u}: largest |z| = {worst:.2f}")


def test_chain_against_one_handle(pkg, cohort, cohort_want):
    """The same data on 1 handle and as 2 and 3 site shards with uneven cuts, one inside a tract of
    the alpha = 1e-3 individuals and one at a chromosome start: within the tolerance of the single
    handle, both units; windows reach across the cuts.  A threshold that reaches past the next
    shard is refused."""
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
        want = {(k, u): whole.ibd_by_length(bu.COHORT_LEN[u], u, sets[k]) for k in names for u in UNITS}
    for cuts in ([0, cut, S], [0, cut, starts[1], S]):
        hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
        try:
            ch = pkg.Chain(hs)
            print()
            for (k, u), w in want.items():
                got = ch.ibd_by_length(bu.COHORT_LEN[u], u, sets[k])
                assert got.shape == w.shape
                _check(got, w, bu.TOL[u], f"{len(hs)} shards {u} {k}")
            a, b = ch.ibd_by_length((1, 80), "sites", sets["chrom"]), ch.ibd_by_length((1, 80), "sites", sets["chrom"])
            assert a.tobytes() == b.tobytes()
        finally:
            for h in hs:
                h.close()
    cuts = [0, cut, cut + 47, S]
    hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        ch = pkg.Chain(hs)
        assert ch.ibd_by_length((1, 8, 40), "sites").shape == (d.n_ind, 1, 3)
        with pytest.raises(pkg.NgsFHMMError) as ei:
            ch.ibd_by_length((1, 80), "sites")
        assert ei.value.code == -10 and "past the next shard" in ei.value.message
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
    rc = h.lib.nghmm_ibd_by_length(h.handle, what, k,
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
            h.ibd_by_length(1)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        assert _raw(h, 0, [1, 5], [0], [S])[0] == 0 and _raw(h, 1, [0, 0.5], [0], [S])[0] == 0
        assert _raw(h, 0, list(range(1, 9)), [0], [S])[0] == 0
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
            h.ibd_by_length(1, unit="cm")
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_by_length(1, regions=np.array([[0.0, 5.0]]))
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_by_length((3, 2))
        assert ei.value.code == -10 and "increasing" in ei.value.message
        # a chain that was not set up
        with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as g:
            g.load(gl, d.pos_dist_mb)
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            b, e = np.array([0], dtype=np.uint64), np.array([S], dtype=np.uint64)
            L = np.array([1.0])
            buf = C.create_string_buffer(16 * I)
            u64 = C.POINTER(C.c_uint64)
            rc = h.lib.nghmm_chain_ibd_by_length(arr, 2, 0, 1, L.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                                 b.ctypes.data_as(u64), e.ctypes.data_as(u64),
                                                 C.cast(buf, C.c_void_p))
            assert rc == -10 and "nghmm_chain_setup" in h.lib.nghmm_last_error().decode()


def test_by_length_classes(pkg, cohort):
    """by_length_classes on the device's records: the classes add up to the first threshold's
    record, are non-negative within the tolerance, and the mean length of a class lies in it."""
    L = np.asarray(bu.COHORT_LEN["sites"], dtype=np.float64)
    with _handle(pkg, cohort, "fast") as h:
        got = h.ibd_by_length(L, regions=pkg.chromosome_regions(cohort[0].pos_dist_mb))
    cls = pkg.by_length_classes(got)
    tol = bu.TOL["sites"]
    for f in bu.FIELDS:
        assert cls[f].shape == got.shape
        np.testing.assert_allclose(cls[f].sum(axis=-1), got[f][..., 0], rtol=1e-12, atol=tol[f])
        assert (cls[f] >= -2 * tol[f]).all()
    sure = cls["tracts"] > 1e-2      # (a length within 2 tol / 1e-2 = 3e-7 sites)
    assert sure.any() and np.isnan(cls["mean_length"][cls["tracts"] == 0]).all()
    lo = np.broadcast_to(L, cls["tracts"].shape)[sure]
    assert (cls["mean_length"][sure] >= lo * (1 - 1e-5)).all()
    hi = np.broadcast_to(np.r_[L[1:], np.inf], cls["tracts"].shape)[sure]
    assert (cls["mean_length"][sure] < hi * (1 + 1e-5)).all()


def test_cli_ibd_by_length(pkg, tmp_path):
    """ngsF-HMM --ibd_by_length at 6 x 400, two chromosomes, all parameters fixed (so the binding
    can be put at the run's final parameters exactly): the file parses and matches ibd_by_length
    to the %.10g printed, in Mb and with --by_length_sites, per chromosome and with
    --by_length_window 50; without the flag the set of output files and their bytes are those of a
    run without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast"]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_by_length", "0,0.5,2"])
    cli_util.run_cli(base + ["--out", w, "--ibd_by_length", "1,5,40", "--by_length_sites", "--by_length_window", 50])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.bylength"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        for out, window, unit, L in ((a, 0, "mb", (0, 0.5, 2)), (w, 50, "sites", (1, 5, 40))):
            regions = summary_util.chrom_regions(chrom, window)
            got = h.ibd_by_length(L, unit=unit, regions=regions)
            lines = open(out + ".ibd.bylength").read().split("\n")
            assert lines[0] == "ind\tchr\tfirst_pos\tlast_pos\tn_sites\tmin_len\texp_tracts\texp_len"
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
                        for text, v in zip(f[6:], (got["tracts"][i, r, k], got["length"][i, r, k])):
                            assert text == "%.10g" % float(text)
                            assert abs(float(text) - v) <= 1e-9 * max(1.0, abs(v)), (lines[n - 1], v)
