"""Every output entry point across fast-mode layouts.  fast_create (csrc/kernels_fast.hip) cuts an
individual's sites into 64 C lanes of T sites; every walk-shaped kernel (k_info_*, k_expect_*,
k_moments_*, k_bounds_*, k_support_*, k_bylength_*, k_sample_*) combines lanes in a wave, waves in
an individual and pieces in a region, and neutralises the padding behind site S - 1.  The output
tests run them at the cohort's own layout; here NGHMM_FAST_C forces others, and the battery of
tests/replica_util.py (array form, estep() first, indF / alpha / freq as set, so that every
comparison is at identical parameters) is held to the same battery on a handle of the same data at
the reference layout by the rules of tests/layout_util.py: bytes, restated from the handle's own
read-backs, or within twice the tolerance of the entry point's own test file.

Every case reads layout() and asserts what it exists for, prints the layout, the lanes used and
the worst error / tolerance per entry point (run with -s), then asserts."""
import collections

import numpy as np
import pytest

import expect_util as xu
import layout_util as lu
import replica_util as ru
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

KINDS = [False, True]
KIND_IDS = ["dense", "packed"]


def _kind(packed):
    return "packed" if packed else "dense"


class Reference:
    """The cohorts, and per (cohort, packed) one open handle at the reference layout."""

    def __init__(self, pkg):
        self.pkg, self.cohorts, self.handles = pkg, {}, {}

    def cohort(self, n_ind, n_sites):
        key = (n_ind, n_sites)
        if key not in self.cohorts:
            self.cohorts[key] = lu.long_cohort(self.pkg) if key == lu.LONG_SHAPE else \
                sup.gpu_cohort(self.pkg, n_ind, n_sites)
        return self.cohorts[key]

    def handle(self, n_ind, n_sites, packed, fast_c=None):
        key = (n_ind, n_sites, packed, fast_c)
        if key not in self.handles:
            self.handles[key] = lu.handle(self.pkg, self.cohort(n_ind, n_sites), packed, fast_c)
        return self.handles[key]

    def close(self):
        for h in self.handles.values():
            h.close()


@pytest.fixture(scope="module")
def reference(pkg):
    ref = Reference(pkg)
    yield ref
    ref.close()


def _batteries(pkg, h, href, cohort, regions, ranges, scale=1):
    """The same questions to both handles from the same parameters; the report of RULES."""
    d, _, F, A, freq = cohort
    rec = sup.to_records(ranges)
    out = []
    for x in (h, href):
        ru.reset(x, (F, A, freq))
        out.append(ru.battery(pkg, x, regions, arrays=True, estep_only=True, ranges=rec))
    probe = lu.bounds_probe(href, out[0], rec, scale)
    ctx = lu.Context(d.n_ind, d.n_sites, d.pos_dist_mb, regions, F, A, probe, scale)
    return lu.compare(out[0], out[1], ctx)


def _freq_step(tag, h, href, cohort):
    """Case d: estep() and mstep_freq(1) on both handles from the same parameters; freq within
    1e-12 relative (the posteriors differ by at most 2e-13), the emissions made of them likewise."""
    _, _, F, A, freq = cohort
    got = []
    for x in (h, href):
        ru.reset(x, (F, A, freq))
        x.estep()
        x.mstep_freq(1)
        got.append((x.freq, x.e_prob))
    (f, e), (rf, re) = got
    assert not np.array_equal(rf, np.full_like(rf, freq)), "the frequency step moved nothing"
    r_f = float(np.max(np.abs(f - rf) / (lu.FREQ_RTOL * np.abs(rf))))
    fin = np.isfinite(re)
    assert np.array_equal(np.isfinite(e), fin)
    r_e = lu.eprob_ratio(e[fin], re[fin])
    print(f"  {tag}: frequency step, worst error / tolerance: freq {r_f:.3g}, e_prob {r_e:.3g}")
    assert r_f <= 1 and r_e <= 1, (tag, r_f, r_e)


def _cohort_regions(d, T, names):
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, T)
    return collections.OrderedDict((k, sets[k]) for k in names)


@pytest.mark.parametrize("packed", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("fast_c", [1, 2, 3, 4])
def test_cohort_across_waves_per_individual(pkg, reference, fast_c, packed):
    """Case a: 20 x 5003 with 1 to 4 waves per individual (the layout's own count is 5): one wave
    and no cross-wave combination at all, C below the 8-deep prefetch of the boundary scans, lanes
    of up to 80 sites; single-site regions and hand-made ranges on both sides of the lane edges of
    the layout under test.  Then the frequency step (case d)."""
    I, S = 20, 5003
    cohort = reference.cohort(I, S)
    d = cohort[0]
    href = reference.handle(I, S, packed)
    with lu.handle(pkg, cohort, packed, fast_c) as h:
        (C, T), (C0, T0) = h.layout(), href.layout()
        assert C == fast_c and C0 != fast_c and T != T0 and T > 0
        regions = _cohort_regions(d, T, ("whole", "chrom", "gaps", "win7", "edges"))
        ranges = sup.hand_ranges(I, S, d.pos_dist_mb, T)
        tag = f"cohort {_kind(packed)} fast_c={fast_c} against default {(C0, T0)}"
        lu.check(tag, h, _batteries(pkg, h, href, cohort, regions, ranges))
        _freq_step(tag, h, href, cohort)


@pytest.mark.parametrize("n_sites,fast_c,packed", [(6145, 6, False), (3073, 3, True), (9217, 9, False)],
                         ids=["dense-6145-c6", "packed-3073-c3", "dense-9217-c9"])
def test_empty_waves_and_a_one_site_last_lane(pkg, reference, n_sites, fast_c, packed):
    """Case b: the cohort's recipe at sizes where the forced layout pads heavily -- the last used
    lane holds one site (S % T == 1) and at least one whole wave holds nothing (two with C = 9,
    which is no multiple of 8 either).  One-site regions at S - 1, S - 2 and the first site of the
    last used lane, the region [S - T - 3, S), ranges that end at S - 1; the thresholds of the
    battery (2000 sites, 10 Mb among them) reach past S from the last lanes.  Then the frequency
    step (case d).

    The layout these sizes get by themselves has the same lanes as the forced one, or is the same
    (fast_create pads least), so the handle with ONE wave per individual is a second reference: its
    lanes are cut elsewhere."""
    I, S = 20, n_sites
    cohort = reference.cohort(I, S)
    d = cohort[0]
    hrefs = {"default": reference.handle(I, S, packed), "one wave": reference.handle(I, S, packed, 1)}
    with lu.handle(pkg, cohort, packed, fast_c) as h:
        C, T = h.layout()
        assert C == fast_c and hrefs["one wave"].layout()[0] == 1 and hrefs["one wave"].layout()[1] != T
        used = lu.lanes_used(S, T)
        assert 64 * C - used >= 64 and S % T == 1
        assert 64 * C - used >= 128 or fast_c != 9
        regions = _cohort_regions(d, T, ("whole", "chrom", "gaps", "edges"))
        regions.update(lu.tail_regions(S, T))
        ranges = sup.hand_ranges(I, S, d.pos_dist_mb, T) + lu.tail_ranges(S, T)
        for who, href in hrefs.items():
            tag = f"padded {_kind(packed)} {I} x {S} fast_c={fast_c} against {who} {href.layout()}"
            lu.check(tag, h, _batteries(pkg, h, href, cohort, regions, ranges))
            _freq_step(tag, h, href, cohort)


# fast_c: the (C, T) a dense handle of this size gets
LONG_LAYOUTS = {16: (16, 256), 48: (48, 88), 65: (65, 64), 129: (129, 32)}


@pytest.mark.parametrize("fast_c,packed", [(48, False), (65, False), (129, False), (129, True)],
                         ids=["dense-c48-control", "dense-c65", "dense-c129", "packed-c129"])
def test_more_than_64_waves_per_individual(pkg, reference, fast_c, packed):
    """Case c: 2 x 256 003, two chromosomes of unequal length, against the handle with 16 waves per
    individual.  With more than 64 waves a lane of the per-individual finish kernels holds K =
    ceil(C / 64) > 1 chunk operators: k_info_finish's loop (csrc/kernels_info.hip:156-159, K = 2
    and 3, its tail `k < C` both taken and not taken), base_sum and lkl_point_product likewise
    (obs_info at the current and at given points, lkl at 2 I points), the `k0 < C; k0 += 8` scans
    of k_sample_bounds and its relatives with C no multiple of 8.  With the region `whole` at C =
    129 every wave but the last lies wholly inside the region and is one piece of its segment: 125
    whole-wave pieces (8001 lanes used), so k_moments_segments takes K = 2 pieces per lane and nl =
    63 < 64 lanes (csrc/kernels_moments.hip:173-182).  C = 48 is the control: a K = 1 layout of the
    same data, which must meet the same bounds.

    The bytes and restated rules hold as they are.  Nobody has measured a yardstick at this
    length: the bound per field is the cohort's, x 2, x ceil(S / 5003) = 52 -- these roundings
    grow about linearly with the chain (DESIGN.md section 4 and the drift table of section 5).

    Regression: `length` of ibd_by_length in sites over `whole` missed this bound at every layout
    here, the K = 1 control included (1.31 to 1.42 of it; individual 0, L = 2000 sites:
    92867.15610435 with lanes of 256 sites against ...10414 / ...10412 with 88 / 64 / 32, the
    numpy yardsticks 92867.15610411): k_bylength_fill added every site's ln rho to a running Q at
    its full magnitude (max|Q| = 42 318 here, 598 on the cohort), so the error of Q_b - Q_a grew
    with the sites per lane.  With the lane's own sum kept apart the cases are within 0.21."""
    I, S = lu.LONG_SHAPE
    cohort = reference.cohort(I, S)
    d = cohort[0]
    cs = [int(x) for x in np.flatnonzero(np.isinf(d.pos_dist_mb)) if x > 0]
    assert len(cs) == 1 and cs[0] not in (S // 2, -(-S // 2))          # two chromosomes, unequal
    href = reference.handle(I, S, packed, fast_c=16)
    if not packed:
        assert href.layout() == LONG_LAYOUTS[16]
    assert href.layout()[0] == 16
    with lu.handle(pkg, cohort, packed, fast_c) as h:
        C, T = h.layout()
        assert C == fast_c and (packed or (C, T) == LONG_LAYOUTS[fast_c])
        assert -(-C // 64) == {48: 1, 65: 2, 129: 3}[fast_c]
        sets = xu.region_sets(S, d.pos_dist_mb, 0)
        regions = collections.OrderedDict((k, sets[k]) for k in ("whole", "chrom", "win2049"))
        regions["edges"] = lu.edge_sites(S, T)
        ranges = lu.wave_ranges(S, T, d.pos_dist_mb)
        W = 64 * T
        assert sum(1 for _, a, b in ranges if a // W != b // W) >= 3          # across wave edges
        assert lu.lanes_used(S, T) // 64 > 64 or fast_c != 129                # > 64 whole-wave pieces
        scale = -(-S // 5003)
        tag = f"long {_kind(packed)} {I} x {S} fast_c={fast_c} against {href.layout()}"
        rep = _batteries(pkg, h, href, cohort, regions, ranges, scale)
        print(f"\n  largest |Q| of ibd_by_length: {h.by_length_qmax():.1f} (reference {href.by_length_qmax():.1f})")
        lu.check(tag, h, rep)
