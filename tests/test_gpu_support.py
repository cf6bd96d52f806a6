"""Tract support on the device (nghmm_tract_support / nghmm_chain_tract_support, include/nghmm.h)
against yardstick B of tests/support_util.py (log space, np.longdouble), which
tests/test_support_cpu.py checks against enumeration.

Tolerance.  The two yardsticks A and B differ on this cohort by at most (tests/test_support_cpu.py
prints the figures; support_util.SPREAD holds them)
    log_p_ibd 5.3e-13,   log_p_non 1.03e-12,   post_min 1.04e-13
over the posterior tracts at 0.5 and 0.9 and the hand-made ranges -- the spread of two correct
restatements.  It does not grow in proportion to the length of a range (4.1e-13 at one site,
1.0e-12 at 5003 sites), so the tolerance does not either: 16 x the spread, 1.65e-11 for the two
logarithms and 1.66e-12 for post_min, wherever the yardstick is finite.  Both are far inside the
project's own bound for chains of this length (1e-9 per site of the range, 1e-9 for post_min).
post_min_site must be equal wherever the yardstick's runner-up is more than that tolerance away."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cli_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

LOG_FIELDS = ("log_p_ibd", "log_p_non")


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


def _handle(pkg, cohort, mode, called=None, F=None, A=None, sites=None):
    d, gl, F0, A0, freq = cohort
    lo, hi = sites or (0, d.n_sites)
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | (pkg.GENO_PACKED if called == "packed" else 0)
    h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=m)
    pos = np.ascontiguousarray(d.pos_dist_mb[lo:hi])
    if called:
        h.load_raw(np.ascontiguousarray(d.gl[lo:hi]), pos, space=0, call_geno=True)
    else:
        h.load(np.ascontiguousarray(gl[lo:hi]), pos)
    h.set_params(F0 if F is None else F, A0 if A is None else A, freq)
    h.init_emission()
    return h


def _range_sets(h, pos, lane_sites):
    """The Viterbi tracts, the posterior tracts at 0.5 and 0.9 and the hand-made ranges."""
    h.estep()
    h.viterbi()
    sets = {"viterbi": h.ibd_tracts("viterbi"), "post0.5": h.ibd_tracts("posterior", 0.5),
            "post0.9": h.ibd_tracts("posterior", 0.9)}
    hand = sup.hand_ranges(h.n_ind, h.n_sites, pos, lane_sites)
    sets["hand"] = sup.to_records(hand)
    return sets


def _check(got, want, tag, site_stats=None):
    """got against yardstick B within the tolerance of the header; -inf exactly where B has it."""
    for f in LOG_FIELDS:
        inf = np.isneginf(want[f])
        assert not np.isnan(got[f]).any(), (tag, f)
        assert np.array_equal(np.isneginf(got[f]), inf), (tag, f, "-inf exactly where the yardstick has it")
        err = np.abs(got[f][~inf] - want[f][~inf])
        print(f"  {tag:9s} {f}: {len(err)} finite, largest |device - B| = {err.max() if len(err) else 0:.3e} "
              f"(tol {sup.LOG_TOL:.3e})")
        assert (err <= sup.LOG_TOL).all(), (tag, f, err.max())
    err = np.abs(got["post_min"] - want["post_min"])
    print(f"  {tag:9s} post_min: largest |device - B| = {err.max():.3e} (tol {sup.POST_TOL:.3e})")
    assert (err <= sup.POST_TOL).all(), (tag, err.max())
    clear = want["runner_up"] - want["post_min"] > sup.POST_TOL
    assert np.array_equal(got["post_min_site"][clear], want["post_min_site"][clear]), tag
    if site_stats is not None:
        site_stats[0] += int((~clear).sum())
        site_stats[1] += len(clear)
    with np.errstate(invalid="ignore"):
        lod = (got["log_p_ibd"] - got["log_p_non"]) / math.log(10.0)
    assert np.array_equal(got["lod"], lod, equal_nan=True)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_scores_match_the_yardstick(pkg, cohort, mode):
    d = cohort[0]
    pos = d.pos_dist_mb
    with _handle(pkg, cohort, mode) as h:
        T = h.layout()[1] or 80
        sets = _range_sets(h, pos, T)
        hand = sets["hand"]
        # the hand-made ranges are what they are meant to be
        a, b = hand[:, 1], hand[:, 1] + hand[:, 2] - 1
        assert set(a % 8) == set(range(8)) and set(b % 8) == set(range(8))
        if mode == "fast":
            bounds = np.arange(T, d.n_sites, T)
            assert np.isin(bounds - 1, b).sum() + np.isin(bounds, a).sum() >= len(bounds) // 2
            assert all(((a < t) & (b >= t)).any() for t in bounds)
        assert (hand[:, 2] == 1).sum() >= 5 and (hand[:, 2] == d.n_sites).sum() == 1
        cs = int([x for x in np.flatnonzero(np.isinf(pos)) if x > 0][0])
        assert ((hand[:, 0] == 2) & (a < cs) & (b >= cs)).any()
        assert len(sets["viterbi"]) > 50 and (sets["viterbi"]["n_sites"][sets["viterbi"]["ind"] < 5] > 3 * T).any()
        e, F, A = h.e_prob, h.indF, h.alpha
        stats = [0, 0]
        print()
        for tag, rec in sets.items():
            want = sup.support_b(e, pos, F, A, rec)
            for f in LOG_FIELDS:
                assert np.isfinite(want[f]).all(), (tag, f)
            got = h.tract_support(rec)
            assert got.dtype == pkg.TRACT_SCORE_DTYPE and len(got) == len(rec)
            _check(got, want, tag, stats)
            # a one-site range: ln of the per-site posterior
            n = sup.as_ranges(rec)[2] - sup.as_ranges(rec)[1] + 1
            one = n == 1
            np.testing.assert_allclose(got["log_p_ibd"][one], np.log(got["post_min"][one]), rtol=1e-13,
                                       atol=1e-14)
            whole = n == d.n_sites
            for k in np.flatnonzero(whole):
                assert math.exp(got["log_p_ibd"][k]) + math.exp(got["log_p_non"][k]) <= 1.0
        print(f"  post_min_site: {stats[0]} of {stats[1]} ranges have a runner-up within the tolerance")
        assert stats[0] < 0.02 * stats[1]
        # two adjacent ranges are scored separately, each as if the other were not there
        k = int(np.flatnonzero((hand[:-1, 0] == hand[1:, 0]) & (b[:-1] + 1 == a[1:]))[0])
        pair = h.tract_support(hand[k:k + 2])
        assert pair.tobytes() == h.tract_support(hand)[k:k + 2].tobytes()


@pytest.mark.parametrize("called", ["dense", "packed"])
def test_excluded_states_give_minus_infinity(pkg, cohort, called):
    """Called genotypes: a heterozygote excludes the IBD state (test_support_cpu.py shows that the
    restatement carries the exact zero), so every range over one has log_p_ibd = -inf exactly."""
    d = cohort[0]
    pos = d.pos_dist_mb
    with _handle(pkg, cohort, "fast", called=called) as h:
        sets = _range_sets(h, pos, h.layout()[1])
        e, F, A = h.e_prob, h.indF, h.alpha
        assert np.isneginf(e[..., 1]).any() and not np.isneginf(e[..., 0]).any()
        n_inf = 0
        print()
        for tag, rec in sets.items():
            want = sup.support_b(e, pos, F, A, rec)
            got = h.tract_support(rec)
            _check(got, want, tag)
            n_inf += int(np.isneginf(want["log_p_ibd"]).sum())
            assert not np.isneginf(want["log_p_non"]).any()
        assert n_inf > 20


def test_scores_follow_the_current_parameters(pkg, cohort):
    d, gl, F, A, freq = cohort
    pos = d.pos_dist_mb
    with _handle(pkg, cohort, "fast") as h:
        sets = _range_sets(h, pos, h.layout()[1])
        marg = h.marg_prob.copy()
        rng = np.random.default_rng(7)
        F2, A2 = rng.uniform(0.05, 0.9, d.n_ind), rng.uniform(0.02, 1.5, d.n_ind)
        h.set_params(F2, A2, freq)
        rec = sets["post0.5"]
        got = h.tract_support(rec)
        print()
        _check(got, sup.support_b(h.e_prob, pos, F2, A2, rec), "new")
        old = sup.support_b(h.e_prob, pos, F, A, rec)
        assert np.abs(got["log_p_ibd"] - old["log_p_ibd"]).max() > 1e-3
        assert h.marg_prob.tobytes() == marg.tobytes()       # still the old E-step's


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_nothing_else_moves_and_the_same_bytes(pkg, cohort, mode):
    d = cohort[0]
    with _handle(pkg, cohort, mode) as a, _handle(pkg, cohort, mode) as b:
        for h in (a, b):
            h.iter_EM()
            h.viterbi()
        rec = a.ibd_tracts("posterior", 0.5)
        before = (a.indF.tobytes(), a.alpha.tobytes(), a.freq.tobytes(), a.marg_prob.tobytes(),
                  a.ibd_tracts("viterbi").tobytes())
        s1 = a.tract_support(rec)
        after = (a.indF.tobytes(), a.alpha.tobytes(), a.freq.tobytes(), a.marg_prob.tobytes(),
                 a.ibd_tracts("viterbi").tobytes())
        assert before == after
        assert a.geno_posteriors().tobytes() == b.geno_posteriors().tobytes()
        assert a.tract_support(rec).tobytes() == s1.tobytes()
        sub = np.sort(np.random.default_rng(3).choice(len(rec), len(rec) // 3, replace=False))
        assert a.tract_support(rec[sub]).tobytes() == s1[sub].tobytes()
        assert len(a.tract_support(rec[:0])) == 0
        for h in (a, b):
            h.iter_EM()
        for f in ("indF", "alpha", "freq", "marg_prob", "ind_lkl"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_chains_equal_the_single_handle(pkg, cohort):
    d, gl, F, A, freq = cohort
    pos, S = d.pos_dist_mb, d.n_sites
    chrom = int(np.flatnonzero(np.isinf(pos))[1])
    with _handle(pkg, cohort, "fast") as whole:
        sets = _range_sets(whole, pos, whole.layout()[1])
        rec = np.concatenate([sets["hand"][sets["hand"][:, 0] < 1],            # [0, S - 1]
                              np.array([(t["ind"], t["first_site"], t["n_sites"]) for t in sets["viterbi"]
                                        if t["ind"] >= 1], dtype=np.int64).reshape(-1, 3)])
        want = whole.tract_support(rec)
        # a cut inside the longest tract of the long-tract individuals, away from the chromosome start
        v = sets["viterbi"]
        cand = v[(v["ind"] >= 1) & (v["ind"] < 5) & ((v["first_site"] > chrom + 40) |
                                                     (v["first_site"] + v["n_sites"] < chrom - 40))]
        t = cand[np.argmax(cand["n_sites"])]
        inside = int(t["first_site"] + t["n_sites"] // 2) | 1                   # an odd first site
        assert t["n_sites"] > 20 and t["first_site"] < inside < t["first_site"] + t["n_sites"]
        for cuts in ([0, S], sorted([0, inside, S]), sorted([0, inside, chrom, S])):
            hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
            try:
                got = pkg.Chain(hs).tract_support(rec)
                for f in LOG_FIELDS:
                    assert np.abs(got[f] - want[f]).max() <= sup.LOG_TOL, (cuts, f)
                assert np.abs(got["post_min"] - want["post_min"]).max() <= sup.POST_TOL
                same = got["post_min_site"] == want["post_min_site"]
                assert same.mean() > 0.98
                assert pkg.Chain(hs).tract_support(rec).tobytes() == got.tobytes()
            finally:
                for h in hs:
                    h.close()


def test_argument_errors(pkg, cohort):
    d = cohort[0]
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST) as h:
        with pytest.raises(pkg.NgsFHMMError) as ei:          # no data loaded
            h.tract_support([(0, 0, 1)])
        assert ei.value.code == -10 and "no data" in ei.value.message
    with _handle(pkg, cohort, "fast") as h:
        S, I = d.n_sites, d.n_ind
        for rec, word in (([(0, 5, 0)], "record 0 has n_sites = 0"),
                          ([(0, 0, 4), (0, S - 2, 3)], "record 1"),
                          ([(0, S, 1)], "outside the data"),
                          ([(I, 0, 1)], f"record 0 has ind = {I}"),
                          ([(1, 0, 4), (0, 10, 4)], "record 1 (ind 0, first_site 10) is out of order"),
                          ([(1, 10, 4), (1, 2, 4)], "out of order or overlaps record 0"),
                          ([(1, 0, 4), (1, 3, 4)], "out of order or overlaps record 0")):
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.tract_support(np.array(rec, dtype=np.int64))
            assert ei.value.code == -10 and word in ei.value.message, (rec, ei.value.message)
        L = h.lib
        buf = (pkg.hmm.Tract * 1)()
        buf[0].n_sites = 1
        out = (pkg.TractScore * 1)()
        assert L.nghmm_tract_support(h.handle, C.cast(buf, C.c_void_p), 1, None) == -10
        assert b"NULL" in L.nghmm_last_error()
        assert L.nghmm_tract_support(h.handle, None, 1, C.cast(out, C.c_void_p)) == -10
        assert L.nghmm_tract_support(None, C.cast(buf, C.c_void_p), 1, C.cast(out, C.c_void_p)) == -10
        assert L.nghmm_chain_tract_support(None, 1, C.cast(buf, C.c_void_p), 1, C.cast(out, C.c_void_p)) == -10
        assert L.nghmm_tract_support(h.handle, None, 0, None) == 0              # n == 0: nothing to do
        assert L.nghmm_tract_support(h.handle, C.cast(buf, C.c_void_p), 1, C.cast(out, C.c_void_p)) == 0
        # two handles that nghmm_chain_setup has not seen
        with _handle(pkg, cohort, "fast") as g:
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            assert L.nghmm_chain_tract_support(arr, 2, C.cast(buf, C.c_void_p), 1, C.cast(out, C.c_void_p)) == -10
            assert b"nghmm_chain_setup" in L.nghmm_last_error()


def test_cli_ibd_support(pkg, tmp_path):
    """ngsF-HMM --ibd_support on a chain of two with all parameters fixed (so the binding can be put
    at the run's final parameters exactly): the lines are Chain.tract_support of the Viterbi tracts,
    formatted as specified and in .ibd.bed's order; the other output files are those of a run
    without the flag."""
    I, S = 12, 3001
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=3, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.6,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--mode", "fast", "--n_gpus", 2,
            "--devices", "0,0", "--ibd_bed"]
    plain, a = str(tmp_path / "plain"), str(tmp_path / "a")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--ibd_support"])
    for ext in (".indF", ".ibd", ".geno", ".ibd.bed"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("a.")) == \
        sorted(["a" + f[5:] for f in os.listdir(tmp_path) if f.startswith("plain.")] + ["a.ibd.support"])
    bed = open(a + ".ibd.bed").read().split("\n")[:-1]
    got = open(a + ".ibd.support").read().split("\n")
    assert got[0] == "chr\tstart\tend\tind\tn_sites\tpost_mean\tlog10_p_ibd\tlod\tpost_min\tpost_min_pos"
    assert got[-1] == "" and len(got) == len(bed) + 2 and len(bed) > 10
    rows = [ln.split("\t") for ln in got[1:-1]]
    assert [r[:4] for r in rows] == [b.split("\t")[:4] for b in bed]
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
        tr = ch.ibd_tracts("viterbi")
        sc = ch.tract_support(tr)
    finally:
        for h in hs:
            h.close()
    assert len(tr) == len(rows)
    ln10 = math.log(10.0)
    for r, t, x in zip(rows, tr, sc):
        assert r[3] == f"ind{int(t['ind'])}" and int(r[4]) == int(t["n_sites"])
        assert int(r[1]) == int(d.pos[int(t["first_site"])]) - 1
        assert int(r[9]) == int(d.pos[int(x["post_min_site"])])
        want = (t["post_mean"], x["log_p_ibd"] / ln10, x["lod"], x["post_min"])
        for text, w in zip(r[5:9], want):
            assert text == "%.10g" % float(text)                    # the format
            assert abs(float(text) - w) <= 1e-9 * max(1.0, abs(w)), (r, w)
