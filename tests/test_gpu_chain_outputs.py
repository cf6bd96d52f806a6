"""Every output entry point across the cuts of a chain of site shards.  Each nghmm_chain_* twin moves
state across a cut in its own way on top of the shared ChainRelay (boundary vectors; halos of Q, n,
pi, T_k; one byte of decoded state; tracts joined on the host; region parts added in rank order),
and its own test file cuts the 20 x 5003 cohort into two or three dense shards of 47 sites or more.
Here the battery of tests/replica_util.py runs on a pkg.Chain and is held to the same battery on
ONE handle of the same data at the same parameter bytes (tests/chain_util.py: prepare, CHAIN_RULES)
at cuts those files do not have:

  A  [0, 1, k, k+1, S-1, S]         one-site shards: the first, the last, and one inside a tract
  B  [0, k, k+79, S]                a 79-site shard inside a tract: L = 80 sites reaches exactly its
                                    79 sites from both sides, L = 81 one site past it
  C  [0, 1667, 1668, 1669, 3336, S] the last site of chromosome 1 and the first of chromosome 2
                                    stand alone; cuts on two chromosome starts
  D  eight shards where the host cuts (distributed.site_ranges_ragged), NGHMM_FAST_C 1 and 4 in turn
  G  two shards where the host cuts, NGHMM_FAST_C 1 and 2: neighbours of unequal lane length
  E  A and D with packed (called-genotype) members against a packed single handle
  F  a chain of one, fast and exact mode: the bytes of an independent handle

k is chosen on the host inside a confident tract of an alpha = 1e-3 individual (chain_util.cut_site).
Every threshold of bylength_util.COHORT_LEN is first asked alone of ibd_by_length and ibd_long: the
chain must take it exactly when chain_util.admitted (the reach rule, restated) says so, and refuse
it with NGHMM_ERR_ARG otherwise; the battery then asks the admitted ones together.

Members of unequal layouts: fast_create keeps at least 16 sites per lane whatever NGHMM_FAST_C
says, so a shard of D (624 sites) has one wave and T = 16 at either setting.  D keeps its forced
settings and prints what it got; G, whose shards are long enough, asserts the unequal lane lengths.

Every case prints its cuts, the members' (C, T) and the worst error / tolerance per entry point
(run with -s), and asserts what it exists for."""
import collections
import importlib

import numpy as np
import pytest

import bylength_util as bu
import chain_util as cu
import expect_util as xu
import layout_util as lu
import long_util
import replica_util as ru
import sample_util as su
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ENTRIES = ("ibd_by_length", "ibd_long")


class Reference:
    """The cohort, the cut site and the geometries, and per `packed` one open single handle."""

    def __init__(self, pkg):
        self.pkg = pkg
        self.cohort = sup.gpu_cohort(pkg)
        d, gl, F, A, freq = self.cohort
        self.pos = d.pos_dist_mb
        post = long_util.post_b(su.emissions_np(gl, np.full(d.n_sites, freq)), self.pos, F, A, [1], "sites")[0][0]
        self.k = cu.cut_site(post)
        self.starts = [int(x) for x in np.flatnonzero(np.isinf(self.pos)) if x > 0]
        self.cuts = cu.geometries(d.n_sites, self.k, self.starts)
        dd = importlib.import_module("ngsf-hmm_amd.distributed")
        assert cu.shards(self.cuts["D"]) == dd.site_ranges_ragged(d.n_sites, 8)
        assert cu.shards(self.cuts["G"]) == dd.site_ranges_ragged(d.n_sites, 2)
        self.handles = {}

    def handle(self, packed):
        if packed not in self.handles:
            self.handles[packed] = lu.handle(self.pkg, self.cohort, packed)
        return self.handles[packed]

    def close(self):
        cu.close(self.handles.values())


@pytest.fixture(scope="module")
def reference(pkg):
    ref = Reference(pkg)
    yield ref
    ref.close()


def _as_bytes(battery):
    return collections.OrderedDict((k, v if isinstance(v, bytes) else np.ascontiguousarray(v).tobytes())
                                   for k, v in battery.items())


def _probe_thresholds(pkg, ch, pos, cuts, more=()):
    """Every threshold of COHORT_LEN (and `more`, in sites) alone, of both entry points: taken
    exactly when the restatement admits it, refused with NGHMM_ERR_ARG otherwise.  Returns
    {(entry, unit, L): taken} and the battery's `lengths`; a disagreement fails here, so no threshold
    is left out of the battery on the library's word."""
    taken, wrong = {}, []
    for e in ENTRIES:
        for u, table in bu.COHORT_LEN.items():
            for L in tuple(table) + (tuple(more) if u == "sites" else ()):
                try:
                    if e == "ibd_long":
                        ch.ibd_long(L, unit=u, sites=False)
                    else:
                        ch.ibd_by_length(L, unit=u)
                    ok = True
                except pkg.NgsFHMMError as err:
                    assert err.code == -10 and "shard" in err.message, (e, u, L, err.code, err.message)
                    ok = False
                taken[(e, u, L)] = ok
                if ok != cu.admitted(pos, cuts, L, u, e):
                    wrong.append((e, u, L, "taken" if ok else "refused", cu.reach(pos, cuts, L, u)))
    assert not wrong, f"the library and the restated reach rule disagree: {wrong}"
    lengths = cu.admitted_lengths(pos, cuts)
    for e in ENTRIES:
        for u, L in lengths[e].items():
            assert L == tuple(l for l in bu.COHORT_LEN[u] if taken[(e, u, l)])
            assert any(cu.crosses(pos, cuts, l, u) for l in L), "no admitted window crosses a cut"
    return taken, lengths


def _decoded_across(path, cuts, k, need):
    """Some individual's decoded path is IBD on both sides of every cut inside k - 40 .. k + 120."""
    inside = [c for c in cuts[1:-1] if k - cu.STRETCH[0] < c <= k + cu.STRETCH[1]]
    assert len(inside) >= need, (cuts, k)
    for c in inside:
        assert ((path[:, c - 1] != 0) & (path[:, c] != 0)).any(), f"no decoded run across the cut at {c}"
    return inside


def _case(pkg, reference, name, packed=False, twice=False, reorder=False, more=(), cuts_in_tract=0):
    """One geometry: the threshold probes, the two batteries by CHAIN_RULES, and the repeats.
    Returns (the chain's battery, the members' layouts, what the probes found)."""
    cohort = reference.cohort
    d, _, F, A, freq = cohort
    pos, cuts = reference.pos, reference.cuts[name]
    whole = reference.handle(packed)
    T = whole.layout()[1]
    sets = xu.region_sets(d.n_sites, pos, T)
    regions = collections.OrderedDict((k, sets[k]) for k in ("whole", "chrom", "gaps"))
    regions.update(cu.cut_regions(cuts))
    ranges = sup.hand_ranges(d.n_ind, d.n_sites, pos, T) + cu.cut_ranges(cuts)
    rec = sup.to_records(ranges)
    hs = cu.members(pkg, cohort, cuts, packed, cu.FAST_C.get(name))
    try:
        ch = pkg.Chain(hs)
        layouts = [tuple(h.layout()) for h in hs]
        cu.set_point(hs, cuts, F, A, freq)
        taken, lengths = _probe_thresholds(pkg, ch, pos, cuts, more)
        tag = f"{name} {'packed' if packed else 'dense'}"
        rep, got, (F, A, f, em_c) = cu.batteries(pkg, ch, cuts, whole, cohort, regions, ranges, lengths)
        cu.check(tag, cuts, hs, rep)
        inside = _decoded_across(got["path"], cuts, reference.k, cuts_in_tract)
        print(f"  decoded runs across the cuts at {inside}; thresholds taken: "
              + "; ".join(f"{e} {u} {lengths[e][u]}" for e in ENTRIES for u in lengths[e]))
        first = _as_bytes(got)
        if reorder:
            # another order on the same chain: stale shared scratch would show
            cu.set_point(hs, cuts, F, A, f)
            ch.viterbi()
            other = cu.other_order(pkg, ch, regions, rec, lengths)
            assert len(other) >= 10
            differ = [k for k, v in other.items() if first.get(k) != v]
            assert not differ, f"{tag}: another order of calls gives other bytes at {differ}"
        if twice:
            cu.set_point(hs, cuts, F, A, f)
            again = _as_bytes(ru.battery(pkg, ch, regions, arrays=True, ranges=rec, em_step=em_c, lengths=lengths))
            assert not ru.differing(first, again), f"{tag}: a second battery differs at {ru.differing(first, again)}"
    finally:
        cu.close(hs)
    return got, layouts, taken


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_one_site_shards(pkg, reference, packed):
    """Geometry A (E: packed): the first and the last shard hold one site, and a one-site shard lies
    inside a tract, so tracts, windows, regions and ranges cross two cuts within two sites.  The
    decode's tracts hold one with k - 1, k and k + 1: joined across both cuts.  The battery twice
    on the same chain: the same bytes."""
    k = reference.k
    got, layouts, taken = _case(pkg, reference, "A", packed, twice=True, cuts_in_tract=2)
    t = got["ibd_tracts.viterbi"]
    a, b = t["first_site"].astype(np.int64), t["first_site"].astype(np.int64) + t["n_sites"].astype(np.int64)
    assert ((a <= k - 1) & (b > k + 1)).any(), "no tract joined across the two cuts at k and k + 1"
    # a window of 8 sites would cross the one-site shard: refused, in both directions
    assert not taken[("ibd_by_length", "sites", 8)] and not taken[("ibd_long", "sites", 8)]
    assert taken[("ibd_long", "sites", 2)]


def test_exact_fit(pkg, reference):
    """Geometry B: in sites L = 80 reaches exactly the 79 sites of the middle shard, from the left
    (a window that begins on the last site in front of it) and from the right (one that ends on the
    first site behind it), and is taken; L = 81 reaches 80 and is refused."""
    far, back = cu.reach(reference.pos, reference.cuts["B"], 80, "sites")
    assert far[0] == 79 and back[2] == 79
    got, layouts, taken = _case(pkg, reference, "B", cuts_in_tract=2)
    for e in ENTRIES:
        assert taken[(e, "sites", 80)] and not taken[(e, "sites", 81)], e
    assert got["ibd_long.sites.whole.post"].shape[0] == len(cu.admitted_lengths(
        reference.pos, reference.cuts["B"])["ibd_long"]["sites"])


def test_around_a_chromosome_start(pkg, reference):
    """Geometry C: the last site of chromosome 1 and the first of chromosome 2 are shards of their
    own, with a cut on that start and on the next.  No window leaves a chromosome, so every
    threshold is taken."""
    got, layouts, taken = _case(pkg, reference, "C")
    assert all(taken.values())


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_eight_shards_where_the_host_cuts(pkg, reference, packed):
    """Geometry D (E: packed): distributed.site_ranges_ragged(5003, 8), the members created with
    NGHMM_FAST_C 1 and 4 in turn (see the module's docstring for what that gives).  400 sites are
    taken; 700 exceed a shard of 624 and are refused; 2000 exceed every chromosome, have no window
    and are taken.  The battery twice, and the calls in another order, on the same chain."""
    got, layouts, taken = _case(pkg, reference, "D", packed, twice=True, reorder=True, more=(700,))
    assert len(layouts) == 8
    for e in ENTRIES:
        assert taken[(e, "sites", 400)] and not taken[(e, "sites", 700)] and taken[(e, "sites", 2000)], e


def test_neighbours_of_unequal_lane_length(pkg, reference):
    """Geometry G: two shards of about 2500 sites with one and two waves per individual: from
    layout(), the neighbours differ in C and in T."""
    got, layouts, taken = _case(pkg, reference, "G")
    (c0, t0), (c1, t1) = layouts
    assert (c0, c1) == (1, 2) and t0 != t1, layouts


@pytest.mark.parametrize("mode_name", ["fast", "exact"])
def test_a_chain_of_one(pkg, reference, mode_name):
    """Geometry F: for one handle every twin passes its arguments on.  Every key of the chain
    battery is the bytes of the same battery on an independent handle (exact mode: the region set
    `gaps` alone, as replica_util.REGION_SETS)."""
    cohort = reference.cohort
    d, _, F, A, freq = cohort
    S, pos = d.n_sites, reference.pos
    h1, h2 = (cu.member(pkg, cohort, 0, S, mode_name=mode_name) for _ in range(2))
    try:
        T = h1.layout()[1]
        sets = xu.region_sets(S, pos, T)
        regions = collections.OrderedDict((k, sets[k]) for k in (("whole", "chrom", "gaps") if mode_name == "fast"
                                                               else ru.REGION_SETS["exact"]))
        rec = sup.to_records(sup.hand_ranges(d.n_ind, S, pos, T))
        ch = pkg.Chain([h1])
        f, em_c, em_w = cu.prepare(ch, [0, S], h2, (F, A, freq))
        a = ru.battery(pkg, ch, regions, ranges=rec, em_step=em_c)
        b = cu.restrict(ru.battery(pkg, h2, regions, ranges=rec, em_step=em_w), a)
        assert len(a) > 40 and list(a) == list(b)
        assert not ru.differing(a, b), f"a chain of one differs from the handle at {ru.differing(a, b)}"
        assert a["freq"] != np.full(S, freq).tobytes(), "the EM step moved no frequency"
    finally:
        cu.close([h1, h2])
