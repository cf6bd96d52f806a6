"""Tract bounds on the device (nghmm_tract_bounds / nghmm_chain_tract_bounds, include/nghmm.h)
against yardstick B of tests/bounds_util.py (log space, np.longdouble) evaluated at the device's
resolved anchors; tests/test_bounds_cpu.py checks the yardstick against enumeration.

Tolerances.  post_anchor: support_util.POST_TOL.  The reach logarithms: 3 x support_util.LOG_TOL =
4.9e-11 (three logged quantities enter; LOG_TOL is 16 x the measured spread of the two support
yardsticks; the two bounds yardsticks differ by 9.7e-13 on this cohort).  Sites: with TIE = 3 x
LOG_TOL, start_ref(p e^-TIE) <= start_dev <= start_ref(p e^+TIE), likewise for end, and fewer than
1 % of all (record, level, side) cases may differ from the yardstick's site at all.  Anchors: the
yardstick's P(z = 0 | y) at the device's anchor is within POST_TOL, as a relative error, of the
core's minimum, and the anchor is the yardstick's wherever the runner-up is further away than that;
at most 2 % of the records may be unclear in this sense.

Measured on an MI355X (the tests print the figures): reach logarithms within 4.6e-13 of the
yardstick in fast mode, single handle or chain, and in exact mode; post_anchor within 9.2e-14;
0 of 22218 sites differ in either mode, and no anchor has a runner-up within the tolerance."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import bounds_util as bu
import cli_util
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

TIE = bu.TIE
LEVELS = bu.LEVELS


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


def _explicit_set(S, pos, T):
    """One-site cores, which are their own anchors: on both sides of every lane boundary
    (individual 6), on every residue mod 8 (7), at site 0 and S - 1 (8: two chromosomes, the
    limits are the chromosomes' edges), and two far apart in one chromosome (9: the limit is the
    neighbour's anchor, the stretch between them spans many lane-chunks)."""
    rec = []
    for t in range(T, S, T):
        rec += [(6, t - 1, t - 1), (6, t, t)]
    rec += [(7, s, s) for s in range(3, S - 1, 11)]
    rec += [(8, 0, 0), (8, S - 1, S - 1)]
    cs = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    rec += [(9, cs[0] + 7, cs[0] + 7), (9, cs[1] - 9, cs[1] - 9)]
    return sup.to_records(rec)


def _range_sets(h, pos, T):
    """name -> (records, anchors or None): the Viterbi tracts, the posterior tracts at 0.5 and 0.9
    and the hand-made ranges with auto anchors; the hand-made ranges with an anchor given for
    every other record; the one-site cores."""
    h.estep()
    h.viterbi()
    as3 = lambda t: np.array([(x["ind"], x["first_site"], x["n_sites"]) for x in t], dtype=np.int64).reshape(-1, 3)
    sets = {"viterbi": (as3(h.ibd_tracts("viterbi")), None),
            "post0.5": (as3(h.ibd_tracts("posterior", 0.5)), None),
            "post0.9": (as3(h.ibd_tracts("posterior", 0.9)), None)}
    hand = sup.to_records(sup.hand_ranges(h.n_ind, h.n_sites, pos, T))
    sets["hand"] = (hand, None)
    k = np.arange(len(hand))
    anc = (hand[:, 1] + (k * 5) % hand[:, 2]).astype(np.uint64)
    anc[k % 2 == 1] = bu.NO_ANCHOR
    sets["hand+anchors"] = (hand, anc)
    one = _explicit_set(h.n_sites, pos, T)
    sets["one-site"] = (one, one[:, 1].astype(np.uint64))
    return sets


class Stats:
    def __init__(self):
        self.sites = self.sites_differ = self.records = self.unclear = 0


def _check(model, pos, rec, anchors, got, tag, st, levels=LEVELS):
    """(bounds, start, end) against the yardstick `model` at the device's anchors."""
    bd, start, end = got
    n, m = len(rec), len(levels)
    ind, a, b = sup.as_ranges(rec)
    assert len(bd) == n and start.shape == end.shape == (n, m) and start.dtype == end.dtype == np.uint64
    for f in bd.dtype.names:
        if bd.dtype[f] == np.float64:
            assert not np.isnan(bd[f]).any(), (tag, f)
    anc = bd["anchor"].astype(np.int64)
    assert ((a <= anc) & (anc <= b)).all(), tag
    # anchors
    auto = np.ones(n, dtype=bool) if anchors is None else np.asarray(anchors) == bu.NO_ANCHOR
    if anchors is not None:
        assert np.array_equal(anc[~auto], np.asarray(anchors)[~auto].astype(np.int64)), tag
    own = bu.bounds_ref(model, pos, rec, anchors, levels)
    rtol = sup.POST_TOL
    p0_dev = model.p0[ind, anc]
    p0_min = model.p0[ind, own["anchor"]]
    assert (p0_dev[auto] <= p0_min[auto] * (1 + rtol)).all(), tag
    clear = own["runner_up"] > p0_min * (1 + rtol)
    assert np.array_equal(anc[auto & clear], own["anchor"][auto & clear]), tag
    st.records += int(auto.sum())
    st.unclear += int((auto & ~clear).sum())
    # everything else at the device's anchors
    ref = bu.bounds_ref(model, pos, rec, anc, levels)
    for f in ("left_limit", "right_limit"):
        assert np.array_equal(bd[f].astype(np.int64), ref[f]), (tag, f)
    err = np.abs(bd["post_anchor"] - ref["post_anchor"])
    assert (err <= sup.POST_TOL).all(), (tag, err.max())
    worst = 0.0
    for f in ("log_reach_left", "log_reach_right"):
        inf = np.isneginf(ref[f])
        assert np.array_equal(np.isneginf(bd[f]), inf), (tag, f, "-inf exactly where the yardstick has it")
        e = np.abs(bd[f][~inf] - ref[f][~inf])
        worst = max(worst, e.max() if len(e) else 0.0)
        assert (e <= TIE).all(), (tag, f, e.max())
        assert np.array_equal(bd["reach" + f[9:]], np.exp(bd[f])), (tag, f)
    s_dev, e_dev = start.astype(np.int64), end.astype(np.int64)
    differ = 0
    for k in range(n):
        lo, hi, c = ref["left_limit"][k], ref["right_limit"][k], anc[k]
        g, hh = ref["ln_g"][k], ref["ln_h"][k]
        dead = not ref["post_anchor"][k] > 0
        for j, p in enumerate(levels):
            if dead:
                assert s_dev[k, j] == c == e_dev[k, j], (tag, k)
                continue
            assert bu.start_of(g, lo, p * math.exp(-TIE)) <= s_dev[k, j] <= bu.start_of(g, lo, p * math.exp(TIE)), \
                (tag, k, j, s_dev[k, j], ref["start"][k, j])
            assert bu.end_of(hh, c, p * math.exp(TIE)) <= e_dev[k, j] <= bu.end_of(hh, c, p * math.exp(-TIE)), \
                (tag, k, j, e_dev[k, j], ref["end"][k, j])
            # censoring: the answer is the limit exactly when the reach is at least the level
            if lo < c and abs(bd["log_reach_left"][k] - math.log(p)) > TIE:
                assert (s_dev[k, j] == lo) == (bd["log_reach_left"][k] >= math.log(p)), (tag, k, j)
            if hi > c and abs(bd["log_reach_right"][k] - math.log(p)) > TIE:
                assert (e_dev[k, j] == hi) == (bd["log_reach_right"][k] >= math.log(p)), (tag, k, j)
        differ += int((s_dev[k] != ref["start"][k]).sum() + (e_dev[k] != ref["end"][k]).sum())
    # monotone and consistent
    assert (np.diff(s_dev, axis=1) <= 0).all() and (np.diff(e_dev, axis=1) >= 0).all(), tag
    assert (ref["left_limit"][:, None] <= s_dev).all() and (s_dev <= anc[:, None]).all(), tag
    assert (anc[:, None] <= e_dev).all() and (e_dev <= ref["right_limit"][:, None]).all(), tag
    st.sites += 2 * n * m
    st.sites_differ += differ
    print(f"  {tag:13s} {n:4d} records: post_anchor within {err.max():.2e}, reach logarithms within "
          f"{worst:.2e} (tol {TIE:.2e}), {differ} of {2 * n * m} sites differ")
    return ref


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_bounds_match_the_yardstick(pkg, cohort, mode):
    d = cohort[0]
    pos, S = d.pos_dist_mb, d.n_sites
    with _handle(pkg, cohort, mode) as h:
        Cw, T = h.layout()
        if mode == "fast":
            assert Cw >= 2 and T % 8 == 0 and 64 * T < S      # more than one wave per individual
        T = T or 16
        sets = _range_sets(h, pos, T)
        B = bu.FormB(h.e_prob, pos, h.indF, h.alpha)
        st = Stats()
        print()
        refs = {}
        for tag, (rec, anc) in sets.items():
            got = h.tract_bounds(rec, anc)
            assert got[0].dtype == pkg.TRACT_BOUND_DTYPE
            refs[tag] = (_check(B, pos, rec, anc, got, tag, st), got)
        print(f"  {st.sites_differ} of {st.sites} sites differ from the yardstick's; {st.unclear} of "
              f"{st.records} anchors have a runner-up within the tolerance")
        assert st.sites_differ < 0.01 * st.sites
        assert st.unclear <= 0.02 * st.records
        # what the sets are meant to hold
        hand, hanc = sets["hand+anchors"]
        given = hanc != bu.NO_ANCHOR
        assert set(hanc[given].astype(np.int64) % 8) == set(range(8))
        one = sets["one-site"][0]
        assert set(one[:, 1] % 8) == set(range(8))
        lanes = np.arange(T, S, T)
        assert np.isin(lanes - 1, one[one[:, 0] == 6, 1]).all() and np.isin(lanes, one[one[:, 0] == 6, 1]).all()
        ref, (bd, start, end) = refs["viterbi"]
        lo, hi, c = bd["left_limit"].astype(np.int64), bd["right_limit"].astype(np.int64), bd["anchor"].astype(np.int64)
        assert ((lo // T < c // T) | (c // T < hi // T)).any()               # across a lane-chunk boundary
        w = 64 * T
        assert (((lo < w) & (w <= c)) | ((c < w) & (w <= hi))).any()         # across the first wave boundary
        assert len(sets["viterbi"][0]) > 50
        # the levels do bite: intervals of more than one site, and censored and uncensored answers
        assert (start[:, 0] > start[:, 2]).any() and (end[:, 2] > end[:, 0]).any()
        assert (start == lo[:, None]).any() and (start != lo[:, None]).any()
        # individual 8: a core at site 0 and one at S - 1, two chromosomes: the limits are the edges
        ref, (bd, start, end) = refs["one-site"]
        k = np.flatnonzero(one[:, 0] == 8)
        first, last = bu.chrom_edges(pos)
        assert list(bd["left_limit"][k]) == [0, first[S - 1]] and list(bd["right_limit"][k]) == [last[0], S - 1]
        assert (start[k[0]] == 0).all() and bd["log_reach_left"][k[0]] == 0 and (end[k[1]] == S - 1).all()
        # individual 9: two cores in one chromosome: each one's limit is the other's anchor, and one
        # stretch of factors serves both reaches
        k = np.flatnonzero(one[:, 0] == 9)
        assert bd["right_limit"][k[0]] == bd["anchor"][k[1]] and bd["left_limit"][k[1]] == bd["anchor"][k[0]]
        for tag in ("one-site", "viterbi", "post0.5"):
            rec = sets[tag][0]
            bd = refs[tag][1][0]
            pair = np.flatnonzero((rec[:-1, 0] == rec[1:, 0]) & (bd["right_limit"][:-1] == bd["anchor"][1:]))
            assert len(pair) > 10
            with np.errstate(invalid="ignore"):
                lhs = bd["log_reach_right"][pair] - bd["log_reach_left"][pair + 1]
                rhs = np.log(bd["post_anchor"][pair + 1]) - np.log(bd["post_anchor"][pair])
            fin = np.isfinite(lhs) & np.isfinite(rhs)
            assert fin.sum() > 5 and np.abs(lhs[fin] - rhs[fin]).max() <= TIE, tag
        # against the shipped call: the run from the anchor to the right limit
        for tag in ("viterbi", "one-site"):
            rec = sets[tag][0]
            bd = refs[tag][1][0]
            rng = np.stack([rec[:, 0], bd["anchor"].astype(np.int64),
                            bd["right_limit"].astype(np.int64) - bd["anchor"].astype(np.int64) + 1], axis=1)
            keep = np.r_[True, (rng[1:, 0] != rng[:-1, 0]) | (rng[1:, 1] > rng[:-1, 1] + rng[:-1, 2] - 1)]
            sc = h.tract_support(rng[keep])        # (disjoint: a right limit may be the next anchor)
            x = bd[keep]
            with np.errstate(divide="ignore"):
                mine = x["log_reach_right"] + np.log(x["post_anchor"])
            fin = np.isfinite(sc["log_p_ibd"])
            assert np.array_equal(np.isfinite(mine), fin)
            # (either side is within its own tolerance of the yardstick: TIE and LOG_TOL)
            assert np.abs(mine[fin] - sc["log_p_ibd"][fin]).max() <= TIE + sup.LOG_TOL, tag
        # other levels: one, and eight
        rec = sets["post0.5"][0]
        _check(B, pos, rec, None, h.tract_bounds(rec, levels=[0.5]), "one level", Stats(), levels=(0.5,))
        lv8 = (0.999, 0.9, 0.75, 0.5, 0.25, 0.1, 0.01, 1e-6)
        _check(B, pos, rec, None, h.tract_bounds(rec, levels=lv8), "eight levels", Stats(), levels=lv8)


@pytest.mark.parametrize("called", ["dense", "packed"])
def test_a_heterozygote_stops_a_search(pkg, cohort, called):
    """Called genotypes: a heterozygote excludes the IBD state.  A search that meets one stops at
    the site next to it with a reach of -inf exactly, nothing is NaN, and a core whose every site
    is a heterozygote gives post_anchor == 0 and the degenerate record."""
    d = cohort[0]
    pos = d.pos_dist_mb
    with _handle(pkg, cohort, "fast", called=called) as h:
        T = h.layout()[1]
        sets = _range_sets(h, pos, T)
        e = h.e_prob
        het = np.isneginf(e[..., 1])                                         # [I][S]
        assert het.any() and not np.isneginf(e[..., 0]).any()
        B = bu.FormB(e, pos, h.indF, h.alpha)
        st = Stats()
        print()
        # a last level so low that only an excluded state ends the search (while the curve itself
        # is above it: it falls by a few units per hundred sites)
        levels, low = LEVELS + (1e-300,), math.log(1e-300) + TIE
        n_stopped = 0
        for tag in ("viterbi", "post0.5", "hand"):
            rec, anc = sets[tag]
            got = h.tract_bounds(rec, anc, levels=levels)
            ref = _check(B, pos, rec, anc, got, tag, st, levels=levels)
            bd, start, end = got
            for k in np.flatnonzero(np.isneginf(bd["log_reach_right"]) & (bd["post_anchor"] > 0)):
                i, c = rec[k, 0], int(bd["anchor"][k])
                nxt = c + 1 + int(np.flatnonzero(het[i, c + 1:])[0])
                assert nxt <= bd["right_limit"][k] and (end[k] <= nxt - 1).all()
                if ref["ln_h"][k][nxt - 1 - c] > low:
                    assert end[k, -1] == nxt - 1                              # the site next to it
                    n_stopped += 1
            for k in np.flatnonzero(np.isneginf(bd["log_reach_left"]) & (bd["post_anchor"] > 0)):
                i, c, lo = rec[k, 0], int(bd["anchor"][k]), int(bd["left_limit"][k])
                prv = int(np.flatnonzero(het[i, :c])[-1])
                assert prv >= lo and (start[k] >= prv + 1).all()
                if ref["ln_g"][k][prv + 1 - lo] > low:
                    assert start[k, -1] == prv + 1
                    n_stopped += 1
        assert n_stopped > 20 and st.sites_differ < 0.01 * st.sites
        # cores of heterozygotes only
        cores = []
        for i in range(het.shape[0]):
            ss = np.flatnonzero(het[i])
            pair = ss[:-1][np.diff(ss) == 1]
            if len(pair):
                cores.append((i, int(pair[0]), int(pair[0]) + 1))
            elif len(ss):
                cores.append((i, int(ss[0]), int(ss[0])))
        assert len(cores) > 5
        rec = sup.to_records(cores)
        bd, start, end = h.tract_bounds(rec)
        assert (bd["post_anchor"] == 0).all() and np.isneginf(bd["log_reach_left"]).all()
        assert np.isneginf(bd["log_reach_right"]).all() and (bd["reach_left"] == 0).all()
        assert (start == bd["anchor"][:, None]).all() and (end == bd["anchor"][:, None]).all()
        assert np.array_equal(bd["anchor"].astype(np.int64), rec[:, 1])       # the lowest site on ties


def test_bounds_follow_the_current_parameters(pkg, cohort):
    d, gl, F, A, freq = cohort
    pos = d.pos_dist_mb
    with _handle(pkg, cohort, "fast") as h:
        sets = _range_sets(h, pos, h.layout()[1])
        marg = h.marg_prob.copy()
        rng = np.random.default_rng(7)
        F2, A2 = rng.uniform(0.05, 0.9, d.n_ind), rng.uniform(0.02, 1.5, d.n_ind)
        rec = sets["post0.5"][0]
        old = h.tract_bounds(rec)
        h.set_params(F2, A2, freq)
        got = h.tract_bounds(rec)
        print()
        _check(bu.FormB(h.e_prob, pos, F2, A2), pos, rec, None, got, "new", Stats())
        assert np.abs(got[0]["log_reach_right"] - old[0]["log_reach_right"]).max() > 1e-3
        assert (got[1] != old[1]).any()
        assert h.marg_prob.tobytes() == marg.tobytes()       # still the old E-step's


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_nothing_else_moves_and_the_same_bytes(pkg, cohort, mode):
    with _handle(pkg, cohort, mode) as a, _handle(pkg, cohort, mode) as b:
        for h in (a, b):
            h.iter_EM()
            h.viterbi()
        rec = a.ibd_tracts("posterior", 0.5)
        state = lambda: (a.indF.tobytes(), a.alpha.tobytes(), a.freq.tobytes(), a.marg_prob.tobytes(),
                         a.ibd_tracts("viterbi").tobytes())
        before = state()
        s1 = a.tract_bounds(rec)
        assert before == state()
        assert a.geno_posteriors().tobytes() == b.geno_posteriors().tobytes()
        same = lambda x, y: all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
        assert same(a.tract_bounds(rec), s1)
        # a subset that keeps every kept record's two neighbours: runs of three, the middle one
        n = len(rec)
        mid = np.arange(1, n - 1, 4)
        sub = np.unique(np.r_[mid - 1, mid, mid + 1])
        part = a.tract_bounds(rec[sub])
        where = np.searchsorted(sub, mid)
        assert same([x[where] for x in part], [x[mid] for x in s1])
        assert all(len(x) == 0 for x in a.tract_bounds(rec[:0]))
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
        B = bu.FormB(whole.e_prob, pos, whole.indF, whole.alpha)
        rec = sets["viterbi"][0]
        want = whole.tract_bounds(rec)
        one, one_anc = sets["one-site"]
        want_one = whole.tract_bounds(one, one_anc)
        # a cut inside the longest tract of the long-tract individuals, away from the chromosome start
        v = rec[(rec[:, 0] < 5) & ((rec[:, 1] > chrom + 40) | (rec[:, 1] + rec[:, 2] < chrom - 40))]
        t = v[np.argmax(v[:, 2])]
        inside = int(t[1] + t[2] // 2) | 1                   # an odd first site
        assert t[2] > 20 and t[1] < inside < t[1] + t[2]
        print()
        for cuts in ([0, S], sorted([0, inside, S]), sorted([0, inside, chrom, S])):
            hs = [_handle(pkg, cohort, "fast", sites=(lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
            try:
                ch = pkg.Chain(hs)
                got = ch.tract_bounds(rec)
                _check(B, pos, rec, None, got, f"{len(hs)} shards", Stats())
                _check(B, pos, one, one_anc, ch.tract_bounds(one, one_anc), f"{len(hs)} one-site", Stats())
                for f in ("anchor", "left_limit", "right_limit"):
                    assert (got[0][f] == want[0][f]).mean() > 0.98, (cuts, f)
                ok = np.logical_and.reduce([got[0][f] == want[0][f] for f in ("anchor", "left_limit", "right_limit")])
                assert np.abs(got[0]["post_anchor"] - want[0]["post_anchor"])[ok].max() <= sup.POST_TOL
                for f in ("log_reach_left", "log_reach_right"):
                    x, y = got[0][f][ok], want[0][f][ok]
                    assert np.array_equal(np.isneginf(x), np.isneginf(y))
                    fin = np.isfinite(x)
                    assert np.abs(x[fin] - y[fin]).max() <= TIE, (cuts, f)
                assert (got[1] == want[1]).mean() > 0.98 and (got[2] == want[2]).mean() > 0.98
                again = ch.tract_bounds(rec)
                assert all(u.tobytes() == v.tobytes() for u, v in zip(got, again))
            finally:
                for h in hs:
                    h.close()


def test_argument_errors(pkg, cohort):
    d = cohort[0]
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST) as h:
        with pytest.raises(pkg.NgsFHMMError) as ei:          # no data loaded
            h.tract_bounds([(0, 0, 1)])
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
                h.tract_bounds(np.array(rec, dtype=np.int64))
            assert ei.value.code == -10 and word in ei.value.message, (rec, ei.value.message)
        rec = np.array([(0, 10, 5), (0, 20, 5)], dtype=np.int64)
        for anc, word in (([9, 22], "record 0: the anchor 9 is outside its core"),
                          ([12, 25], "record 1: the anchor 25 is outside its core")):
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.tract_bounds(rec, anchors=np.array(anc, dtype=np.uint64))
            assert ei.value.code == -10 and word in ei.value.message, (anc, ei.value.message)
        h.tract_bounds(rec, anchors=np.array([10, 24], dtype=np.uint64))
        for lv, word in (([0.5, 0.9], "strictly descending"), ([0.5, 0.5], "strictly descending"),
                         ([1.0, 0.5], "outside the open range (0, 1)"), ([0.5, 0.0], "outside the open range (0, 1)"),
                         ([0.5, float("nan")], "outside the open range (0, 1)"), ([-0.1], "outside the open range"),
                         ([], "between 1 and 8 levels"),
                         (list(np.linspace(0.9, 0.1, 9)), "between 1 and 8 levels")):
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.tract_bounds(rec, levels=lv)
            assert ei.value.code == -10 and word in ei.value.message, (lv, ei.value.message)
        L = h.lib
        buf = (pkg.hmm.Tract * 1)()
        buf[0].n_sites = 1
        out = (pkg.TractBound * 1)()
        lv = (C.c_double * 1)(0.5)
        s, e = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
        vp = lambda x: C.cast(x, C.c_void_p)
        full = [vp(buf), 1, None, lv, 1, vp(out), vp(s), vp(e)]
        assert L.nghmm_tract_bounds(h.handle, *full) == 0                   # (anchor may be NULL)
        for k in (0, 3, 5, 6, 7):
            args = list(full)
            args[k] = None
            assert L.nghmm_tract_bounds(h.handle, *args) == -10, k
            assert b"NULL" in L.nghmm_last_error()
        assert L.nghmm_tract_bounds(None, *full) == -10
        assert L.nghmm_chain_tract_bounds(None, 1, *full) == -10
        assert L.nghmm_tract_bounds(h.handle, None, 0, None, None, 0, None, None, None) == 0   # n == 0
        with _handle(pkg, cohort, "fast") as g:              # two handles that nghmm_chain_setup has not seen
            arr = (C.c_void_p * 2)(h.handle, g.handle)
            assert L.nghmm_chain_tract_bounds(arr, 2, *full) == -10
            assert b"nghmm_chain_setup" in L.nghmm_last_error()


def test_cli_ibd_bounds(pkg, tmp_path):
    """ngsF-HMM --ibd_bounds on a chain of two with all parameters fixed (so the binding can be put
    at the run's final parameters exactly): the lines are Chain.tract_bounds of the Viterbi tracts,
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
    cli_util.run_cli(base + ["--out", a, "--ibd_bounds", "--bounds_ci", 0.9])
    for ext in (".indF", ".ibd", ".geno", ".ibd.bed"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("a.")) == \
        sorted(["a" + f[5:] for f in os.listdir(tmp_path) if f.startswith("plain.")] + ["a.ibd.bounds"])
    bed = open(a + ".ibd.bed").read().split("\n")[:-1]
    got = open(a + ".ibd.bounds").read().split("\n")
    assert got[0] == ("chr\tstart\tend\tind\tanchor_pos\tpost_anchor\tstart_lo\tstart_med\tstart_hi\tend_lo\t"
                      "end_med\tend_hi\tleft_limit_pos\treach_left\tright_limit_pos\treach_right")
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
        bd, start, end = ch.tract_bounds(tr, levels=((1 + 0.9) / 2, 0.5, (1 - 0.9) / 2))
    finally:
        for h in hs:
            h.close()
    assert len(tr) == len(rows)
    at = lambda s: str(int(d.pos[int(s)]))
    for r, t, x, st, en in zip(rows, tr, bd, start, end):
        assert r[3] == f"ind{int(t['ind'])}" and int(r[1]) == int(d.pos[int(t["first_site"])]) - 1
        assert [r[4], r[12], r[14]] == [at(x["anchor"]), at(x["left_limit"]), at(x["right_limit"])]
        assert r[6:12] == [at(st[2]), at(st[1]), at(st[0]), at(en[0]), at(en[1]), at(en[2])]
        for text, w in zip((r[5], r[13], r[15]), (x["post_anchor"], x["reach_left"], x["reach_right"])):
            assert text == "%.10g" % float(text)                    # the format
            assert abs(float(text) - w) <= 1e-9 * abs(w), (r, w)
