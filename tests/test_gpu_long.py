"""The per-site posterior of lying in a long IBD tract on the device (nghmm_ibd_long /
nghmm_chain_ibd_long, include/nghmm.h) against brute-force enumeration and against yardstick B of
tests/long_util.py (np.longdouble prefixes), which tests/test_long_cpu.py checks against
enumeration.

Tolerance.  The two yardsticks A (float64 running products, plain window sums) and B differ on the
20 x 5003 cohort, over all region sets and the thresholds 1, 2, 8, 80, 81, 400, 2000 sites /
0, 0.05, 0.5, 2, 10 Mb, by at most (tests/test_long_cpu.py measures and prints the figures;
long_util.SPREAD holds them)
    sites: post 1.0e-13, sum 1.2e-13, sites 2.2e-11, mb 2.2e-12
    mb:    post 1.0e-13, sum 1.2e-13, sites 1.1e-11, mb 1.0e-12
-- the spread of two correct restatements.  The tolerance is 16 x the spread per unit and field,
the project's rule and margin; nothing in it comes from a device.  The yardstick runs once on the
emissions numpy makes of the likelihoods and the frequency, and is shared by the tests."""
import ctypes as C
import os

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import expect_util as xu
import layout_util
import long_util as lu
import sample_util as su
import summary_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# tests/test_gpu_bylength.py's ENUM_TOL, for the reason given there
ENUM_TOL = 1e-12
MODES = ["fast", "exact"]
UNITS = ("sites", "mb")


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


def _handle(pkg, cohort, mode, sites=None, fast_c=None):
    d, gl, F, A, freq = cohort
    lo, hi = sites or (0, d.n_sites)
    with layout_util.forced_layout(fast_c):
        h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT)
    h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
    h.set_params(F, A, freq)
    h.init_emission()
    return h


def _lane_len(T):
    """T, T + 1 sites straddle a lane-chunk edge, 64 T, 64 T + 1 a wave edge."""
    return (T, T + 1, 64 * T, 64 * T + 1)


@pytest.fixture(scope="module")
def cohort_want(pkg, cohort):
    """Yardstick B on the cohort, once: the region sets for the lane length of the layout the device
    reports (both modes get the same sets) and {unit: (P, T) [K][I][S]} at COHORT_LEN; "lane": at
    T, T + 1, 64 T and 64 T + 1 sites for the layout's own lane length T."""
    d, gl, F, A, freq = cohort
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    with _handle(pkg, cohort, "fast") as h:
        T = h.layout()[1]
    assert T > 0
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    want = {u: lu.post_b(e, d.pos_dist_mb, F, A, bu.COHORT_LEN[u], u) for u in UNITS}
    want["lane"] = lu.post_b(e, d.pos_dist_mb, F, A, _lane_len(T), "sites")
    return sets, want, T


def _check(err, tol, tag):
    print(f"  {tag:34s}: largest |device - yardstick| = {err:.3e} (tol {tol:.3e})")
    assert err <= tol, (tag, err, tol)


def _check_all(got, PT, pos, reg, tol, tag, threshold=0.5):
    """Every output of one call against the yardstick's (P, T)."""
    P = PT[0]
    if "post" in got:
        assert np.isfinite(got["post"]).all(), tag
        _check(np.abs(got["post"] - P).max(), tol["post"] if isinstance(tol, dict) else tol, f"{tag} post")
    if "sites" in got:
        want = lu.site_records(P, threshold)
        _check(np.abs(got["sites"]["sum"] - want["sum"]).max(), tol["sum"] if isinstance(tol, dict) else tol,
               f"{tag} site sum")
    if "regions" in got:
        want = lu.region_records(PT, pos, reg)
        for f in lu.REGION_FIELDS:
            assert np.isfinite(got["regions"][f]).all(), (tag, f)
            _check(np.abs(got["regions"][f] - want[f]).max(), tol[f] if isinstance(tol, dict) else tol, f"{tag} {f}")


@pytest.mark.parametrize("mode", MODES)
def test_enumeration(pkg, mode):
    """3 x 12 against all 2^12 paths, both units: post, the site records and the region records of
    the whole data, the chromosomes and every single site; a missing cell, an excluded state (exact
    zeros); one threshold alone is its slice of the call with all of them."""
    _, pos, F, A, _, gl, freq = xu.small_case()
    I, S = gl.shape[1], gl.shape[0]
    gl = np.where(np.isneginf(gl), -1e15, gl)          # (the reader's likelihood of an excluded genotype)
    m = pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT
    sets = {"whole": None, "chrom": np.array([[0, 7], [7, S]]), "single": xu.single_site_regions(S)}
    with pkg.NgsFHMM(I, S, mode=m) as h:
        h.load(np.ascontiguousarray(gl), pos)
        h.set_params(F, A, freq)
        h.init_emission()
        e = h.e_prob
        assert np.isneginf(e[1, 4, 1]) or e[1, 4, 1] < -1e14
        e = np.where(e < -1e14, -np.inf, e)            # (as tests/test_gpu_bylength.py)
        print()
        for unit in UNITS:
            L = bu.SMALL_LEN[unit]
            PJ = lu.enumerate_long(e, pos, F, A, L, unit)
            for tag, reg in sets.items():
                got = h.ibd_long(L, unit=unit, regions=reg, sites=True, post=True)
                R = 1 if reg is None else len(reg)
                assert got["regions"].dtype == pkg.LONG_REGION_DTYPE and got["regions"].shape == (I, R, len(L))
                assert got["sites"].dtype == pkg.LONG_SITE_DTYPE and got["sites"].shape == (S, len(L))
                assert got["post"].shape == (len(L), I, S)
                _check(np.abs(got["post"] - PJ[0]).max(), ENUM_TOL, f"{unit} {tag} post")
                _check(np.abs(got["sites"]["sum"] - PJ[0].sum(axis=1).T).max(), ENUM_TOL, f"{unit} {tag} site sum")
                assert np.array_equal(got["sites"]["count"], (got["post"] >= 0.5).sum(axis=1).T)
                want = lu.enumerated_regions(PJ, pos, [[0, S]] if reg is None else reg)
                for f in lu.REGION_FIELDS:
                    _check(np.abs(got["regions"][f] - want[f]).max(), ENUM_TOL, f"{unit} {tag} {f}")
                assert (got["post"][:, 1, 4] == 0.0).all(), "the excluded state lies in no tract"
            assert (got["regions"]["sites"][1, 4] == 0.0).all() and (got["regions"]["mb"][1, 4] == 0.0).all()
            assert np.array_equal(got["post"][0], h.ibd_long(L[0], unit, regions=False, sites=False, post=True)["post"][0])
            for k, l in enumerate(L):      # one threshold alone is the same bytes
                one = h.ibd_long(l, unit=unit, regions=sets["single"], sites=True, post=True)
                assert one["post"].tobytes() == got["post"][k:k + 1].tobytes()
                assert one["sites"].tobytes() == got["sites"][:, k:k + 1].tobytes()
                assert one["regions"].tobytes() == got["regions"][:, :, k:k + 1].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_yardstick(pkg, cohort, cohort_want, mode):
    """20 x 5003 against yardstick B within 16 x spread, both units, over every region set; the
    thresholds of COHORT_LEN, and T, T + 1, 64 T and 64 T + 1 sites for the layout's own lane
    length T (windows that straddle a lane-chunk edge and a wave edge); 2000 sites exceed every
    chromosome: exactly 0."""
    d = cohort[0]
    pos = d.pos_dist_mb
    sets, want, T = cohort_want
    with _handle(pkg, cohort, mode) as h:
        assert mode != "fast" or h.layout()[1] == T
        print()
        for unit in UNITS:
            L = bu.COHORT_LEN[unit]
            for tag, reg in sets.items():
                first = tag == "whole"
                got = h.ibd_long(L, unit=unit, regions=reg, sites=first, post=first)
                _check_all(got, want[unit], pos, reg, lu.TOL[unit], f"{unit} {tag}")
                if unit == "sites":
                    assert (got["regions"]["sites"][..., -1] == 0).all() and (got["regions"]["mb"][..., -1] == 0).all()
                if first:
                    assert np.array_equal(got["sites"]["count"], (got["post"] >= 0.5).sum(axis=1).T)
                    if unit == "sites":
                        assert (got["post"][-1] == 0).all() and (got["sites"]["sum"][:, -1] == 0).all()
        for tag in ("whole", "edges", "win7", "chrom"):
            first = tag == "whole"
            got = h.ibd_long(_lane_len(T), regions=sets[tag], sites=first, post=first)
            _check_all(got, want["lane"], pos, sets[tag], lu.TOL["sites"], f"lane {tag}")


@pytest.mark.parametrize("mode", MODES)
def test_identities(pkg, cohort, mode):
    """Against the handle's own ibd_by_length over the chromosomes (sites and mb are its length in
    sites and in Mb) and its own ibd_expect at L = 1 site and 0 Mb on every region set, each within
    the sum of the two tolerances; 0 <= post <= pi + tolerance; post non-increasing in k within
    2 x tolerance; the site records against the returned post."""
    d = cohort[0]
    pos, S, I = d.pos_dist_mb, d.n_sites, d.n_ind
    with _handle(pkg, cohort, mode) as h:
        sets = xu.region_sets(S, pos, h.layout()[1] or xu.SPREAD_LANE_SITES)
        print()
        for unit, fl, xf in (("sites", "sites", "ibd"), ("mb", "mb", "ibd_mb")):
            L = bu.COHORT_LEN[unit]
            tol = lu.TOL[unit]
            got = h.ibd_long(L, unit=unit, regions=sets["chrom"], sites=True, post=True)
            by = h.ibd_by_length(L, unit=unit, regions=sets["chrom"])
            err = np.abs(got["regions"][fl] - by["length"]).max()
            print(f"  {unit:5s} {fl} against ibd_by_length's length over the chromosomes: {err:.3e}")
            assert err <= tol[fl] + bu.TOL[unit]["length"]
            for tag, reg in sets.items():
                ex = h.ibd_expect(reg, sites=False)[0]
                one = h.ibd_long(L[0], unit=unit, regions=reg, sites=False)["regions"]
                err = np.abs(one[fl][..., 0] - ex[xf]).max()
                print(f"  {unit:5s} {tag:8s} {fl} at the first threshold against ibd_expect's {xf}: {err:.3e}")
                assert err <= tol[fl] + xu.REGION_TOL[xf]
            post = got["post"]
            pi = post[0]                              # (L = 1 site, 0 Mb: P = pi)
            assert not np.isnan(post).any() and (post >= 0).all() and (post <= pi[None] + tol["post"]).all()
            assert (np.diff(post, axis=0) <= 2 * tol["post"]).all()
            want = post.sum(axis=1).T
            assert (np.abs(got["sites"]["sum"] - want) <= I * 2.0 ** -53 * np.abs(want)).all()
            assert np.array_equal(got["sites"]["count"], (post >= 0.5).sum(axis=1).T)
            hi = h.ibd_long(L, unit=unit, regions=False, sites=True, post=False, threshold=0.9)["sites"]
            assert np.array_equal(hi["count"], (post >= 0.9).sum(axis=1).T)
            assert hi["sum"].tobytes() == got["sites"]["sum"].tobytes()


def test_a_second_layout(pkg, cohort, cohort_want):
    """The same cohort in a layout with another C (other lane-chunks, other wave edges): every
    output within 2 x TOL of the default layout's, and both within TOL of the yardstick."""
    d = cohort[0]
    pos = d.pos_dist_mb
    sets, want, T = cohort_want
    with _handle(pkg, cohort, "fast") as h0, _handle(pkg, cohort, "fast", fast_c=2) as h1:
        assert h1.layout()[1] != T
        print()
        for unit in UNITS:
            L = bu.COHORT_LEN[unit]
            tol = lu.TOL[unit]
            for tag in ("whole", "chrom", "win64", "gaps", "edges"):
                first = tag == "whole"
                a = h0.ibd_long(L, unit=unit, regions=sets[tag], sites=first, post=first)
                b = h1.ibd_long(L, unit=unit, regions=sets[tag], sites=first, post=first)
                _check_all(a, want[unit], pos, sets[tag], tol, f"default {unit} {tag}")
                _check_all(b, want[unit], pos, sets[tag], tol, f"C = 2 {unit} {tag}")
                for f in lu.REGION_FIELDS:
                    assert (np.abs(a["regions"][f] - b["regions"][f]) <= 2 * tol[f]).all()
                if first:
                    assert (np.abs(a["post"] - b["post"]) <= 2 * tol["post"]).all()
                    assert (np.abs(a["sites"]["sum"] - b["sites"]["sum"]) <= 2 * tol["sum"]).all()
        T1 = h1.layout()[1]
        got = h1.ibd_long((T1, T1 + 1), regions=sets["chrom"], post=True)
        assert np.isfinite(got["post"]).all() and (np.diff(got["post"], axis=0) <= 2 * lu.TOL["sites"]["post"]).all()


@pytest.mark.parametrize("mode", MODES)
def test_packed_called_genotypes(pkg, mode):
    """8 x 300 called genotypes as 2-bit codes: everything finite; a called heterozygote lies in
    no tract (the IBD state is excluded): exact zeros."""
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
            got = h.ibd_long(L, unit=unit, regions=xu.single_site_regions(S), sites=True, post=True)
            assert np.isfinite(got["post"]).all() and np.isfinite(got["sites"]["sum"]).all()
            for f in lu.REGION_FIELDS:
                assert np.isfinite(got["regions"][f]).all()
            assert (got["post"][:, het] == 0.0).all() and (got["post"][:, ~het] > 0.0).any()
            assert (got["regions"]["sites"][het] == 0.0).all() and (got["regions"]["mb"][het] == 0.0).all()
            np.testing.assert_array_equal(got["regions"]["sites"], np.moveaxis(got["post"], 0, 2))
            ex = h.ibd_expect(None, sites=False)[0]
            whole = h.ibd_long(L[0], unit=unit, sites=False)["regions"]
            np.testing.assert_allclose(whole["sites"][:, 0, 0], ex["ibd"][:, 0], rtol=1e-11)
            np.testing.assert_allclose(whole["mb"][:, 0, 0], ex["ibd_mb"][:, 0], rtol=1e-11, atol=1e-13)


def test_same_bits_and_nothing_else_moves(pkg, cohort):
    """Two calls give the same bits; a region's record does not depend on the other regions, nor
    any output's bytes on which others are asked for; parameters, posteriors and the decoded path
    stay, and an EM iteration after the calls gives the bits it gives without them."""
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
                    a = h.ibd_long(L, unit, regions, sites=True, post=True)
                    b = h.ibd_long(L, unit, regions, sites=True, post=True)
                    for k in a:
                        assert a[k].tobytes() == b[k].tobytes(), k
                    h.ibd_by_length(L, unit)          # (shares the cells' scratch)
                    r = h.ibd_long(L, unit, regions, sites=False)
                    assert list(r) == ["regions"] and r["regions"].tobytes() == a["regions"].tobytes()
                    s = h.ibd_long(L, unit, regions=False, sites=True)
                    assert list(s) == ["sites"] and s["sites"].tobytes() == a["sites"].tobytes()
                    p = h.ibd_long(L, unit, regions=False, sites=False, post=True)
                    assert list(p) == ["post"] and p["post"].tobytes() == a["post"].tobytes()
                    one = h.ibd_long(L, unit, regions[2:3], sites=False)["regions"]
                    assert one.tobytes() == a["regions"][:, 2:3].tobytes()
                    whole = h.ibd_long(L, unit, sites=True)
                    assert whole["sites"].tobytes() == a["sites"].tobytes()
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
def test_on_a_replica(pkg, cohort, mode):
    """A replica (nghmm_create_replica: the parent's data, parameters of its own) returns the bytes
    of an independent handle at the replica's parameters, and the parent's results stay the bytes
    they were: what a multi-start run relies on when a later replicate wins."""
    d, gl, F, A, freq = cohort
    regions = pkg.window_regions(d.pos_dist_mb, 777)
    other = (np.ascontiguousarray(F[::-1]), np.ascontiguousarray(A[::-1]), 0.3)

    def outputs(h):
        return [h.ibd_long(bu.COHORT_LEN[u], u, regions, sites=True, post=True) for u in UNITS]

    def same(a, b):
        return all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in x)

    with _handle(pkg, cohort, mode) as parent:
        before = outputs(parent)
        rep = parent.replica()
        try:
            rep.set_params(*other)
            rep.init_emission()
            got = outputs(rep)
            assert same(outputs(parent), before)
            assert same(outputs(rep), got)
        finally:
            rep.close()
    with _handle(pkg, cohort, mode) as alone:
        assert same(outputs(alone), before)
        alone.set_params(*other)
        alone.init_emission()
        want = outputs(alone)
    assert same(got, want) and not same(got, before)


def test_chain_against_one_handle(pkg, cohort, cohort_want):
    """The same data on 1 handle and as 2 and 3 site shards with uneven cuts, one inside a tract of
    the alpha = 1e-3 individuals and one at a chromosome start: within the tolerance of the single
    handle, both units; windows reach across the cuts in both directions.  A threshold that reaches
    past the neighbouring shard is refused."""
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    sets, want_b, _ = cohort_want
    post = want_b["sites"][0][0]                       # (L = 1 site: pi)
    starts = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    inside = [s for s in range(1100, 1400) if (post[:5, s - 40:s + 40] >= 0.9).all(axis=1).any()]
    assert inside, "a cut inside a confident tract of an alpha = 1e-3 individual"
    cut = inside[len(inside) // 2]
    assert cut not in starts and cut < starts[0]
    names = ("whole", "chrom", "win2048", "gaps", "win7", "edges")
    with _handle(pkg, cohort, "fast") as whole:
        want = {(k, u): whole.ibd_long(bu.COHORT_LEN[u], u, sets[k], sites=k == "whole", post=k == "whole")
                for k in names for u in UNITS}
    for cuts in ([0, cut, S], [0, cut, starts[1], S]):
        hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
        try:
            ch = pkg.Chain(hs)
            print()
            for (k, u), w in want.items():
                got = ch.ibd_long(bu.COHORT_LEN[u], u, sets[k], sites=k == "whole", post=k == "whole")
                tol = lu.TOL[u]
                assert sorted(got) == sorted(w)
                for f in lu.REGION_FIELDS:
                    assert got["regions"].shape == w["regions"].shape
                    _check(np.abs(got["regions"][f] - w["regions"][f]).max(), tol[f], f"{len(hs)} shards {u} {k} {f}")
                if k == "whole":
                    _check(np.abs(got["post"] - w["post"]).max(), tol["post"], f"{len(hs)} shards {u} post")
                    _check(np.abs(got["sites"]["sum"] - w["sites"]["sum"]).max(), tol["sum"], f"{len(hs)} shards {u} sum")
                    assert np.array_equal(got["sites"]["count"], (got["post"] >= 0.5).sum(axis=1).T)
            a = ch.ibd_long((1, 80), "sites", sets["chrom"], post=True)
            b = ch.ibd_long((1, 80), "sites", sets["chrom"], post=True)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes()
        finally:
            for h in hs:
                h.close()
    cuts = [0, cut, cut + 47, S]
    hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        ch = pkg.Chain(hs)
        assert ch.ibd_long((1, 8, 40), "sites")["regions"].shape == (d.n_ind, 1, 3)
        with pytest.raises(pkg.NgsFHMMError) as ei:
            ch.ibd_long((1, 80), "sites")
        assert ei.value.code == -10 and "shard" in ei.value.message
        assert "to the right" in ei.value.message or "to the left" in ei.value.message
    finally:
        for h in hs:
            h.close()


def _raw(h, what, lengths, begin, end, thr=0.5, regions=True, sites=True, post=False, n=None, k=None,
         null_len=False, null_begin=False):
    u64 = C.POINTER(C.c_uint64)
    dp = C.POINTER(C.c_double)
    b, e = np.array(begin, dtype=np.uint64), np.array(end, dtype=np.uint64)
    L = np.array(lengths, dtype=np.float64)
    n = len(b) if n is None else n
    k = len(L) if k is None else k
    kk = max(k, 1)
    rbuf = C.create_string_buffer(16 * h.n_ind * max(n, 1) * kk)
    sbuf = C.create_string_buffer(16 * h.n_sites * kk)
    pbuf = np.zeros(kk * h.n_ind * h.n_sites)
    rc = h.lib.nghmm_ibd_long(h.handle, what, k, None if null_len or not len(L) else L.ctypes.data_as(dp), thr, n,
                              None if null_begin or not len(b) else b.ctypes.data_as(u64),
                              None if not len(e) else e.ctypes.data_as(u64),
                              C.cast(rbuf, C.c_void_p) if regions else None,
                              C.cast(sbuf, C.c_void_p) if sites else None,
                              pbuf.ctypes.data_as(dp) if post else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg):
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=3, n_chrom=2)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, 0, [1], [0], [S])                     # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_long(1)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        h.set_params(0.3, 0.2, 0.2)
        h.init_emission()
        assert _raw(h, 0, [1, 5], [0], [S])[0] == 0 and _raw(h, 1, [0, 0.5], [0], [S], post=True)[0] == 0
        assert _raw(h, 0, list(range(1, 9)), [0], [S])[0] == 0
        assert _raw(h, 0, [1], [], [], regions=False, n=0)[0] == 0          # site records alone
        assert _raw(h, 0, [1], [], [], regions=False, sites=False, post=True, n=0)[0] == 0
        assert _raw(h, 0, [1], [0], [S], sites=False)[0] == 0
        assert _raw(h, 0, [1], [0], [S], thr=0.0)[0] == 0 and _raw(h, 0, [1], [0], [S], thr=1.0)[0] == 0
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
            ((0, [1], [0], [S]), {"thr": -0.1}),                # the count's threshold outside [0, 1]
            ((0, [1], [0], [S]), {"thr": 1.5}),
            ((0, [1], [0], [S]), {"thr": nan}),
            ((0, [1], [], []), {"n": 0, "regions": False, "sites": False}),   # all three outputs NULL
            ((0, [1], [], []), {"n": 0}),                       # records without regions
            ((0, [1], [0], [S]), {"regions": False}),           # regions without records
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
            h.ibd_long(1, unit="cm")
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_long(1, regions=np.array([[0.0, 5.0]]))
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_long((3, 2))
        assert ei.value.code == -10 and "increasing" in ei.value.message
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_long(1, regions=False, sites=False, post=False)
        assert ei.value.code == -10
        # a chain that was not set up
        with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as g:
            g.load(gl, d.pos_dist_mb)
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            b, e = np.array([0], dtype=np.uint64), np.array([S], dtype=np.uint64)
            L = np.array([1.0])
            buf = C.create_string_buffer(16 * I)
            u64 = C.POINTER(C.c_uint64)
            rc = h.lib.nghmm_chain_ibd_long(arr, 2, 0, 1, L.ctypes.data_as(C.POINTER(C.c_double)), 0.5, 1,
                                            b.ctypes.data_as(u64), e.ctypes.data_as(u64), C.cast(buf, C.c_void_p),
                                            None, None)
            assert rc == -10 and "nghmm_chain_setup" in h.lib.nghmm_last_error().decode()


def test_cli_ibd_long(pkg, tmp_path):
    """ngsF-HMM --ibd_long at 6 x 400, two chromosomes, all parameters fixed (so the binding can be
    put at the run's final parameters exactly): the three files parse and match ibd_long to the
    %.10g printed (post to the bit), in Mb and with --long_sites, per chromosome and with
    --long_window 50; without the flag the set of output files and their bytes are those of a run
    without it."""
    I, S = 6, 400
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast"]
    plain, a, w = str(tmp_path / "plain"), str(tmp_path / "a"), str(tmp_path / "w")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_long", "0,0.5,2"])
    cli_util.run_cli(base + ["--out", w, "--ibd_long", "1,5,40", "--long_sites", "--long_window", 50, "--long_thresh",
                             0.8, "--long_post"])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    made = lambda pre: sorted(f[len(pre):] for f in os.listdir(tmp_path) if f.startswith(pre + "."))
    assert made("a") == sorted(made("plain") + [".ibd.long.regions", ".ibd.long.sites"])
    assert made("w") == sorted(made("plain") + [".ibd.long.regions", ".ibd.long.sites", ".ibd.long.post"])
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    close = lambda text, v: text == "%.10g" % float(text) and abs(float(text) - v) <= 1e-9 * max(1.0, abs(v))
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(0.6, 0.05, 0.1)
        h.init_emission()
        h.iter_EM(freq_est=0, indF_fixed=True, alpha_fixed=True)
        for out, window, unit, L, thr in ((a, 0, "mb", (0, 0.5, 2), 0.5), (w, 50, "sites", (1, 5, 40), 0.8)):
            regions = summary_util.chrom_regions(chrom, window)
            got = h.ibd_long(L, unit=unit, regions=regions, sites=True, post=True, threshold=thr)
            lines = open(out + ".ibd.long.regions").read().split("\n")
            assert lines[0] == "ind\tchr\tfirst_pos\tlast_pos\tn_sites\tmin_len\texp_sites\texp_mb"
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
                        rec = got["regions"][i, r, k]
                        assert close(f[6], rec["sites"]) and close(f[7], rec["mb"]), (lines[n - 1], rec)
            lines = open(out + ".ibd.long.sites").read().split("\n")
            assert lines[0] == "chr\tpos\tmin_len\tcount\tpost_sum"
            assert lines[-1] == "" and len(lines) == 2 + S * len(L)
            n = 1
            for s in range(S):
                for k, l in enumerate(L):
                    f = lines[n].split("\t")
                    n += 1
                    rec = got["sites"][s, k]
                    assert f[:4] == [chrom[s], str(pos[s]), "%.10g" % l, str(int(rec["count"]))], lines[n - 1]
                    assert close(f[4], rec["sum"]), (lines[n - 1], rec)
            if out == w:
                raw = np.fromfile(out + ".ibd.long.post", dtype=np.float64)
                assert raw.size == len(L) * I * S and raw.tobytes() == got["post"].tobytes()
