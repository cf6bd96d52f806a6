"""The per-site posterior of lying in a long IBD tract without a GPU: the two numpy yardsticks of
tests/long_util.py against brute-force enumeration, the identities and properties of
include/nghmm.h (nghmm_ibd_long) against bylength_util's and expect_util's yardsticks, long_tracts
against tracts_util.rle_tracts, and the spread of the two yardsticks on the cohort of
tests/test_gpu_long.py (the figure that test's tolerance is made of)."""
import os
import re

import numpy as np

import bylength_util as bu
import expect_util as xu
import long_util as lu
import sample_util as su
import support_util as sup
import tracts_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The yardsticks against enumeration: sums of at most 12 terms of order 1, each a product of at
# most 12 factors: a few hundred roundings of 1.1e-16 at the worst.  test_bylength_cpu.py's bound.
ENUM_ATOL = 2e-13
UNITS = ("sites", "mb")


def test_yardsticks_equal_enumeration():
    """A and B against all 2^12 paths, sites and Mb: two chromosomes, a missing cell, a called
    heterozygote whose IBD state is excluded (exact zeros at that cell); the region and site
    records made of them."""
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    sets = {"whole": np.array([[0, S]]), "chrom": np.array([[0, 7], [7, S]]), "single": xu.single_site_regions(S)}
    worst = 0.0
    for unit in UNITS:
        L = bu.SMALL_LEN[unit]
        want = lu.enumerate_long(e, pos, F, A, L, unit)
        assert (want[0][:, 1, 4] == 0.0).all()
        for name, fn in (("A", lu.post_a), ("B", lu.post_b)):
            P, T = fn(e, pos, F, A, L, unit)
            assert np.isfinite(P).all() and np.isfinite(T).all(), (name, unit)
            assert (P[:, 1, 4] == 0.0).all(), "the excluded state lies in no tract"
            worst = max(worst, np.abs(P - want[0]).max(), np.abs((P - T) - want[1])[:, :, ~xu.chrom_start(pos)].max())
            np.testing.assert_allclose(P, want[0], rtol=0, atol=ENUM_ATOL, err_msg=f"{name} {unit}")
            for tag, reg in sets.items():
                got, ref = lu.region_records((P, T), pos, reg), lu.enumerated_regions(want, pos, reg)
                for f in lu.REGION_FIELDS:
                    np.testing.assert_allclose(got[f], ref[f], rtol=0, atol=ENUM_ATOL, err_msg=f"{name} {unit} {tag}")
            np.testing.assert_allclose(lu.site_records(P)["sum"], want[0].sum(axis=1).T, rtol=0, atol=ENUM_ATOL)
    print(f"\n  yardsticks against enumeration: largest difference {worst:.2e}")
    assert worst <= 1e-13


def test_identities_and_properties():
    """Over whole chromosomes sites is by_length's length in sites and mb its length in Mb; at
    L = 1 site sites is ibd_expect's ibd and at 0 Mb mb its ibd_mb, on any region; 0 <= P <= pi, P
    non-increasing in k, P = pi at L = 1 site and 0 Mb, exact zeros for a threshold no chromosome
    reaches, nothing NaN; P - T is the pairwise probability of the enumeration."""
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    ex = xu.terms_b(e, pos, F, A)
    chrom = np.array([[0, 7], [7, S]])
    sets = {"whole": np.array([[0, S]]), "chrom": chrom, "single": xu.single_site_regions(S)}
    for fn, bfn, xfn in ((lu.post_a, bu.terms_a, xu.terms_a), (lu.post_b, bu.terms_b, xu.terms_b)):
        pi = xfn(e, pos, F, A)["ibd"]
        for unit, field in (("sites", "sites"), ("mb", "mb")):
            L = bu.SMALL_LEN[unit]
            P, T = fn(e, pos, F, A, L, unit)
            rec = lu.region_records((P, T), pos, chrom)
            want = bu.region_records(bfn(e, pos, F, A, L, unit), chrom)
            np.testing.assert_allclose(rec[field], want["length"], rtol=0, atol=ENUM_ATOL, err_msg=unit)
            assert np.array_equal(P[0], pi), "at L = 1 site and at 0 Mb P is pi"
            assert (P >= 0).all() and (P <= pi[None]).all() and not np.isnan(P).any()
            assert (np.diff(P, axis=0) <= ENUM_ATOL).all()
            for tag, reg in sets.items():
                r, w = lu.region_records((P, T), pos, reg), xu.region_records(ex, reg)
                np.testing.assert_allclose(r["sites" if unit == "sites" else "mb"][..., 0],
                                           w["ibd" if unit == "sites" else "ibd_mb"], rtol=0, atol=ENUM_ATOL)
        P, T = fn(e, pos, F, A, (8, 100), "sites")
        assert (P == 0).all() and (T == 0).all(), "no chromosome of the small case has 8 sites"
        P, T = fn(e, pos, F, A, (50.0,), "mb")
        assert (P == 0).all()


def test_window_tables_agree():
    """a <= lo_k(s) iff b_k(a) <= s, on the small case and on an uneven map."""
    rng = np.random.default_rng(5)
    pos = rng.uniform(0.001, 0.5, 60)
    pos[[0, 23, 24, 50]] = np.inf
    for p in (xu.small_case()[1], pos):
        S = len(p)
        for unit, L in (("sites", (1, 2, 3, 5, 30)), ("mb", (0.0, 0.2, 0.7, 3.0))):
            b, lo = bu.window_ends(p, L, unit), lu.window_starts(p, L, unit)
            cs = np.flatnonzero(xu.chrom_start(p))
            c0 = cs[np.searchsorted(cs, np.arange(S), side="right") - 1]
            for k in range(len(L)):
                for s in range(S):
                    for a in range(c0[s], s + 1):
                        assert (lo[k, s] >= a) == (0 <= b[k, a] <= s), (unit, k, s, a)


def test_long_tracts_against_rle(pkg):
    rng = np.random.default_rng(3)
    I, S = 7, 200
    post = rng.uniform(0, 1, (I, S))
    post[2, 40:90] = 0.9
    post[3] = 1.0
    post[4] = 0.0
    pos = rng.uniform(0.01, 0.2, S)
    pos[[0, 57, 140]] = np.inf
    for thr, ms in ((0.5, 1), (0.5, 3), (0.9, 1), (0.0, 1), (1.0, 2)):
        got = pkg.long_tracts(post, pos, threshold=thr, min_sites=ms)
        want = tracts_util.rle_tracts(post >= thr, np.isinf(pos), marg=post, min_sites=ms)
        assert got.dtype == pkg.hmm.TRACT_DTYPE and len(got) == len(want), (thr, ms)
        for g, w in zip(got, want):
            assert (int(g["ind"]), int(g["first_site"]), int(g["n_sites"])) == w[:3]
            assert abs(g["post_sum"] - w[3]) <= 1e-12 * S
            assert abs(g["post_mean"] - w[3] / w[2]) <= 1e-12
    assert len(pkg.long_tracts(post[4:5], pos)) == 0
    names, positions = ["c"] * S, np.arange(S) * 100 + 1
    assert len(pkg.bed_lines(pkg.long_tracts(post, pos), names, positions, [f"i{k}" for k in range(I)]))


def test_records_mirror_the_header(pkg):
    import ctypes as C
    hm = pkg.hmm
    assert C.sizeof(hm.LongRegionStat) == 16 and C.sizeof(hm.LongSiteStat) == 16
    assert list(pkg.LONG_REGION_DTYPE.names) == list(lu.REGION_FIELDS)
    assert list(pkg.LONG_SITE_DTYPE.names) == list(lu.SITE_FIELDS)
    assert pkg.LONG_SITE_DTYPE == lu.SITE_DTYPE and pkg.LONG_REGION_DTYPE == lu.REGION_DTYPE
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    for name, fields in (("nghmm_long_region_stat", lu.REGION_FIELDS), ("nghmm_long_site_stat", lu.SITE_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*[,;]", body) == list(fields)
    assert int(re.search(r"NGHMM_LONG_MB = (\d+)", header).group(1)) == pkg.LONG_MB == 1


def test_yardstick_spread_on_the_gpu_cohort(pkg):
    """|A - B| per unit and output field on the cohort, thresholds and region sets of the GPU test
    (printed; long_util.SPREAD holds the figures, and the GPU tolerance is 16 x them).  To
    re-measure: pytest -s tests/test_long_cpu.py -k spread, and copy the printed maxima."""
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    pos = d.pos_dist_mb
    for unit in UNITS:
        L = bu.COHORT_LEN[unit]
        a, b = lu.post_a(e, pos, F, A, L, unit), lu.post_b(e, pos, F, A, L, unit)
        assert all(np.isfinite(x).all() for x in a + b), unit
        worst = {"post": float(np.abs(a[0] - b[0]).max()),
                 "sum": lu.spread(lu.site_records(a[0]), lu.site_records(b[0]))["sum"], "sites": 0.0, "mb": 0.0}
        for name, reg in xu.region_sets(d.n_sites, pos, xu.SPREAD_LANE_SITES).items():
            s = lu.spread(lu.region_records(a, pos, reg), lu.region_records(b, pos, reg))
            worst = {f: max(worst[f], s.get(f, 0.0)) for f in worst}
        if unit == "sites":   # 2000 sites exceed every chromosome: exactly nothing
            assert (a[0][-1] == 0).all() and (b[0][-1] == 0).all()
        print(f"\n  spread |A - B| in {unit}: " + ", ".join(f"{f} {worst[f]:.3e}" for f in worst))
        # what the GPU test uses is what is measured here (within a factor of two: libm versions)
        for f in worst:
            assert 0 < lu.SPREAD[unit][f] and worst[f] <= 2 * lu.SPREAD[unit][f], (unit, f, worst[f])
    # far inside the project's own bound on posteriors (1e-9 per site) for a region of any length
    assert max(max(t.values()) for t in lu.TOL.values()) <= 1e-9 * 7
