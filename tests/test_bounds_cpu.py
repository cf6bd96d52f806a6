"""Tract bounds without a GPU: the two numpy yardsticks of tests/bounds_util.py against brute-force
enumeration, and their disagreement on the cohort of tests/test_gpu_bounds.py."""
import numpy as np
import pytest

import bounds_util as bu
import sample_util as su
import support_util as sup
import tracts_util


def _small_case(with_zero):
    """3 x 12: two chromosomes (a start at site 7), random likelihoods, one frequency per site;
    with_zero: individual 1 has a cell with likelihoods (0, 1, 0) at site 9: a heterozygote, which
    excludes IBD there."""
    rng = np.random.default_rng(11)
    I, S = 3, 12
    gl = np.log(rng.dirichlet(np.ones(3), size=(S, I)))
    if with_zero:
        with np.errstate(divide="ignore"):
            gl[9, 1] = np.log(np.array([0.0, 1.0, 0.0]))
    pos = rng.uniform(0.01, 0.6, S)
    pos[0] = pos[7] = np.inf
    e = su.emissions_np(gl, rng.uniform(0.1, 0.5, S))
    F, A = np.array([0.3, 0.6, 0.85]), np.array([0.4, 1.5, 0.05])
    return e, pos, F, A


@pytest.mark.parametrize("with_zero", [False, True])
def test_yardsticks_equal_enumeration(with_zero):
    """ln G and ln H of A and B against all 2^12 paths, for every individual and anchor, across the
    chromosome start at site 7; P(z = 0 | y) likewise; with an excluded state at (1, 9) every curve
    over it is -inf from there on in all three."""
    e, pos, F, A = _small_case(with_zero)
    S = e.shape[1]
    if with_zero:
        assert np.isneginf(e[1, 9, 1]), "the restatement carries the exact zero"
    models = {"A": bu.FormA(e, pos, F, A), "B": bu.FormB(e, pos, F, A)}
    for i in range(3):
        for c in range(S):
            g, h, p0 = bu.enumerate_curves(e, pos, F, A, i, c)
            if with_zero and i == 1 and c == 9:
                continue            # the anchor itself cannot be IBD: no curve
            if with_zero and i == 1:
                assert np.isneginf(h[9 - c:]).all() if c < 9 else np.isneginf(g[:10]).all()
            for name, m in models.items():
                for want, got in ((g, m.ln_g(i, 0, c)), (h, m.ln_h(i, c, S - 1))):
                    fin = np.isfinite(want)
                    assert np.array_equal(np.isneginf(got), ~fin), (name, i, c)
                    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=3e-13, err_msg=f"{name} {i} {c}")
                np.testing.assert_allclose(m.p0[i], p0, rtol=1e-12, atol=0)
                assert got[0] == 0.0 and m.ln_g(i, 0, c)[-1] == 0.0         # G(c) = H(c) = 1


def test_definition_on_a_small_case():
    """Anchors, limits, quantile sites and the degenerate record of bounds_ref, on the 3 x 12 case:
    the limit is the chromosome's edge or the neighbour's anchor, the two reaches across one
    stretch differ by the anchors' posteriors, a heterozygote stops a search at the site next to
    it."""
    e, pos, F, A = _small_case(True)
    rec = sup.to_records([(0, 1, 3), (0, 5, 6), (0, 8, 10), (1, 2, 5), (1, 7, 7), (1, 9, 9), (1, 10, 11),
                          (2, 7, 7)])
    for m in (bu.FormA(e, pos, F, A), bu.FormB(e, pos, F, A)):
        r = bu.bounds_ref(m, pos, rec)
        anc = r["anchor"]
        assert list(r["left_limit"]) == [0, anc[0], 7, 0, 7, 7, 9, 7]
        assert list(r["right_limit"]) == [anc[1], 6, 11, 6, 9, anc[6], 11, 11]
        # records 0 and 1 share a stretch
        lhs = r["log_reach_right"][0] - r["log_reach_left"][1]
        rhs = np.log(r["post_anchor"][1]) - np.log(r["post_anchor"][0])
        assert abs(lhs - rhs) < 1e-12
        # individual 1: site 9 excludes IBD
        assert r["post_anchor"][5] == 0 and np.isneginf(r["log_reach_left"][5])
        assert (r["start"][5] == 9).all() and (r["end"][5] == 9).all()
        assert (r["end"][4] <= 8).all() and r["end"][4][-1] == 8 and np.isneginf(r["log_reach_right"][4])
        assert (r["start"][6] >= 10).all() and r["start"][6][-1] == 10 and np.isneginf(r["log_reach_left"][6])
        for k in range(len(rec)):
            assert (np.diff(r["start"][k]) <= 0).all() and (np.diff(r["end"][k]) >= 0).all()
            assert (r["left_limit"][k] <= r["start"][k]).all() and (r["start"][k] <= anc[k]).all()
            assert (anc[k] <= r["end"][k]).all() and (r["end"][k] <= r["right_limit"][k]).all()
    # explicit anchors
    r = bu.bounds_ref(m, pos, rec, anchors=[3, bu.NO_ANCHOR, 8, 2, 7, 9, 11, 7])
    assert list(r["anchor"][[0, 2, 3, 6]]) == [3, 8, 2, 11] and r["anchor"][1] == anc[1]


def test_yardstick_disagreement_on_the_gpu_cohort(pkg):
    """A against B on the cohort of the GPU test (20 x 5003), posterior tracts at 0.5 and 0.9 with
    auto anchors and the levels 0.975 / 0.5 / 0.025, limits at the neighbours' anchors.  Measured
    (printed below): at 0.5, 616 tracts, no anchor and 0 of 3696 sites differ, reach logarithms
    within 9.7e-13, post_anchor within 2.4e-14; at 0.9, 595 tracts, no anchor and 0 of 3570 sites
    differ, reach logarithms within 4.6e-13.  The yardstick alone is far inside the device test's
    3 x LOG_TOL = 4.9e-11 and its 1 % of sites."""
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    pos = d.pos_dist_mb
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    a, b = bu.FormA(e, pos, F, A), bu.FormB(e, pos, F, A)
    cs = np.isinf(pos)
    for thr in (0.5, 0.9):
        rec = np.array([(i, s, n) for i, s, n, _ in tracts_util.rle_tracts(b.p1 >= thr, cs)],
                       dtype=np.int64).reshape(-1, 3)
        ra, rb = bu.bounds_ref(a, pos, rec), bu.bounds_ref(b, pos, rec)
        c = bu.compare(ra, rb)
        print(f"\n  threshold {thr}: {len(rec)} tracts, {c['anchors_differ']} anchors and "
              f"{c['sites_differ']} of {c['sites']} sites differ, reach logarithms within "
              f"{c['log_reach']:.2e}, post_anchor within {c['post_anchor']:.2e}")
        assert len(rec) > 500
        clear = rb["runner_up"] > _p0_at_anchor(b, rec, rb) * (1 + sup.POST_TOL)
        assert (ra["anchor"][clear] == rb["anchor"][clear]).all()
        assert c["log_reach"] <= bu.TIE / 3
        assert c["sites_differ"] < 0.01 * c["sites"]


def _p0_at_anchor(model, rec, r):
    ind, _, _ = sup.as_ranges(rec)
    return model.p0[ind, r["anchor"]]
