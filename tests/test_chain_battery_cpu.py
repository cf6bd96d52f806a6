"""Keeps the chain battery (tests/chain_util.py, tests/test_gpu_chain_outputs.py) complete and its
rules total, and checks the geometries, the region and range sets on the cuts and the restatement
of the reach rule where no device is needed."""
import importlib
import inspect
import math
import os
import re

import numpy as np
import pytest

import bylength_util as bu
import chain_util as cu
import layout_util as lu
import long_util
import replica_util as ru
import sample_util as su
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 5003


def _declared_chain_calls():
    """Every nghmm_chain_* that a public header declares (all of include/ but nghmm_debug.h)."""
    text = ""
    for f in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if f.endswith(".h") and f != "nghmm_debug.h":
            text += open(os.path.join(ROOT, "include", f)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return set(re.findall(r"\b(nghmm_chain_[a-z_0-9]+)\s*\(", text))


def test_every_chain_twin_is_called(pkg):
    """From the source of replica_util.battery (and of chain_util.prepare, which runs the EM step)
    and of hmm.Chain: every nghmm_chain_* of the public headers but nghmm_chain_setup, which
    Chain() itself calls, is behind a method that the battery uses on its handle."""
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    declared = _declared_chain_calls()
    assert {"nghmm_chain_setup", "nghmm_chain_iter_em", "nghmm_chain_viterbi", "nghmm_chain_ibd_long",
            "nghmm_chain_ibd_longest", "nghmm_chain_geno_smooth", "nghmm_chain_tract_bounds"} <= declared
    used = set(re.findall(r"\bh\.([A-Za-z_][A-Za-z_0-9]*)", inspect.getsource(ru.battery)))
    used |= set(re.findall(r"\bch\.([A-Za-z_][A-Za-z_0-9]*)", inspect.getsource(cu.prepare)))
    reached = set()
    for attr in used:
        member = inspect.getattr_static(hm.Chain, attr, None)
        fn = member.fget if isinstance(member, property) else member
        if fn is not None and callable(fn):
            reached |= set(re.findall(r"self\.lib\.(nghmm_chain_[a-z_0-9]+)", inspect.getsource(fn)))
    assert "nghmm_chain_setup" in inspect.getsource(hm.Chain.__init__)
    missing = sorted(declared - reached - {"nghmm_chain_setup"})
    assert not missing, f"chain twins that the chain battery does not call: {missing}"
    # ... and every public method of Chain is used: a twin bound in hmm.py without its header line
    public = {n for n, v in vars(hm.Chain).items() if not n.startswith("_") and (callable(v) or isinstance(v, property))}
    assert not sorted(public - used), sorted(public - used)


class _Stub:
    """What battery() needs of a member: parameters."""
    indF = alpha = np.zeros(3)


def _stub_chain(pkg, calls):
    """A Chain without a library: every public method records its name and returns an array."""
    hm = importlib.import_module("ngsf-hmm_amd.hmm")

    def method(name):
        def f(self, *a, **k):
            calls.append(name)
            return np.zeros(2)
        return f
    body = {n: method(n) for n, v in vars(hm.Chain).items() if not n.startswith("_") and callable(v)}
    body.update(__init__=lambda self: None, freq=property(lambda self: np.zeros(2)),
                marg_prob=property(lambda self: np.zeros(2)), handles=[_Stub(), _Stub()], n_ind=3, n_sites=50)
    return type("StubChain", (hm.Chain,), body)()


def _chain_keys(pkg):
    calls = []
    z = np.zeros(2)
    keys = list(ru.battery(pkg, _stub_chain(pkg, calls), {"whole": np.array([[0, 50]])}, arrays=True,
                           ranges=np.zeros((1, 3), dtype=np.int64), em_step={"freq": z, "ind_lkl": z}))
    return keys, calls


def test_chain_rules_are_total_over_the_chain_battery(pkg):
    keys, calls = _chain_keys(pkg)
    assert {"indF", "freq", "marg_prob", "path", "tract_bounds.hand", "ibd_long.mb.whole", "geno_smooth.whole",
            "ibd_summary.posterior.whole", "mstep_freq.freq", "ibd_sharing.range"} <= set(keys)
    assert "ibd_long" in calls and "mstep_freq" in calls and "viterbi" in calls
    heads = {k.split(".")[0] for k in keys}
    assert not heads & set(cu.NO_TWIN) and "mstep_freq.e_prob" not in keys
    for k in keys:
        for full in (k, k + ".0", k + ".regions"):
            assert len(lu.rule_of(full, cu.CHAIN_RULES)) == 1, (full, lu.rule_of(full, cu.CHAIN_RULES))
    assert set(cu.CHAIN_RULES) == heads
    # the single handle's battery has these keys and more; restrict() leaves the chain's, in order
    src = inspect.getsource(ru.battery)
    single = {n.split(".")[0] for n in re.findall(r'_records\(out, f?"([^"]+)"', src)}
    assert heads | set(cu.NO_TWIN) == single == set(lu.RULES)
    # every rule is an override named in OVERRIDES or layout_util's own, and has its class
    for k, rule in cu.CHAIN_RULES.items():
        assert rule is (cu.OVERRIDES[k] if k in cu.OVERRIDES else lu.RULES[k]), k
        assert rule.__doc__ or k not in cu.OVERRIDES, f"{k}: an override says what it rests on"
    classed = [k for v in cu.RULE_CLASS.values() for k in v]
    assert sorted(classed) == sorted(cu.CHAIN_RULES)
    assert set(cu.RULE_CLASS["em_step"]) | {"geno_smooth"} == set(cu.OVERRIDES)
    for k, v in cu.TOLERANCES.items():
        assert math.isfinite(v) and v > 0, k
    # the project's own figures (tests/test_gpu_siteshard.py::test_chain_shapes), as they stand there
    text = open(os.path.join(ROOT, "tests", "test_gpu_siteshard.py")).read()
    body = text[text.index("def test_chain_shapes"):text.index("def test_chain_of_eight")]
    assert "ch.ind_lkl, whole.ind_lkl, rtol=1e-12" in body and cu.IND_LKL_RTOL == 1e-12
    assert "ch.freq, whole.freq, rtol=1e-10, atol=1e-13" in body and (cu.FREQ_RTOL, cu.FREQ_ATOL) == (1e-10, 1e-13)
    assert "ch.marg_prob, whole.marg_prob, atol=1e-9" in body and cu.MARG_ATOL == 1e-9


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


@pytest.fixture(scope="module")
def geo(pkg, cohort):
    """(pos, k, {name: cuts}) as tests/test_gpu_chain_outputs.py makes them."""
    d, gl, F, A, freq = cohort
    pos = d.pos_dist_mb
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    post = long_util.post_b(e, pos, F, A, [1], "sites")[0][0]
    k = cu.cut_site(post)
    starts = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    return pos, k, cu.geometries(d.n_sites, k, starts), post


def test_the_geometries(pkg, geo):
    pos, k, G, post = geo
    assert cu.CUT_WINDOW[0] <= k < cu.CUT_WINDOW[1]
    assert (post[:5, k - 40:k + 121] >= 0.9).all(axis=1).any()
    starts = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    assert starts == [1668, 3336] and k + 120 < starts[0]
    for name, cuts in G.items():
        assert cuts[0] == 0 and cuts[-1] == S and all(a < b for a, b in cu.shards(cuts)), name
    size = lambda name: [b - a for a, b in cu.shards(G[name])]
    assert size("A")[0] == 1 and size("A")[-1] == 1 and size("A")[2] == 1 and G["A"][2] == k
    assert size("B")[1] == 79 and G["B"][1] == k and G["B"][2] < starts[0]
    assert G["C"][1:5] == [starts[0] - 1, starts[0], starts[0] + 1, starts[1]] and size("C")[1:3] == [1, 1]
    dd = importlib.import_module("ngsf-hmm_amd.distributed")
    for name, n in (("D", 8), ("G", 2)):
        assert cu.shards(G[name]) == dd.site_ranges_ragged(S, n), name
    # fast_create keeps 16 sites per lane: NGHMM_FAST_C = 4 needs 4 x 64 x 16 sites
    assert max(size("D")) < 2 * 64 * 16 <= min(size("G"))


def _sorted_disjoint(reg, n_sites):
    reg = np.asarray(reg)
    return bool((reg[:, 0] < reg[:, 1]).all() and (reg[1:, 0] >= reg[:-1, 1]).all()
                and reg[0, 0] >= 0 and reg[-1, 1] <= n_sites)


def _shard_of(cuts, site):
    return int(np.searchsorted(np.asarray(cuts), site, side="right")) - 1


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "G"])
def test_cut_regions(geo, name):
    cuts = geo[2][name]
    sets = cu.cut_regions(cuts)
    for reg in sets.values():
        assert _sorted_disjoint(reg, S)
    one = sets["cut1"]
    assert (one[:, 1] - one[:, 0] == 1).all()
    for c in cuts[1:-1]:                                       # both sides of every cut
        assert c - 1 in one[:, 0] and c in one[:, 0]
    allreg = np.concatenate(list(sets.values()))
    as_set = {(int(a), int(b)) for a, b in allreg}
    sh = cu.shards(cuts)
    assert set(sh) <= as_set                                    # a region that is exactly one shard
    for a, b in sh:
        if b - a == 1:
            assert (a, b) in {(int(x), int(y)) for x, y in one}   # ... exactly a one-site shard
    n_sh = [_shard_of(cuts, b - 1) - _shard_of(cuts, a) + 1 for a, b in sets["span"]]
    assert max(n_sh) >= min(3, len(cuts) - 1)
    inner = set(cuts[1:-1])
    assert any(a in inner for a, _ in as_set) and any(b in inner for _, b in as_set)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "G"])
def test_cut_ranges(pkg, cohort, geo, name):
    pos, _, G, _ = geo
    cuts = G[name]
    got = cu.cut_ranges(cuts)
    hand = sup.hand_ranges(20, S, pos, 16)
    assert not {i for i, _, _ in hand} & {i for i, _, _ in got}
    assert {i for i, _, _ in got} == set(cu.RANGE_INDS) and not set(cu.RANGE_INDS) & set(range(10))
    rec = sup.to_records(hand + got)
    assert len(rec) == len(set(hand + got)) and (rec[:, 2] >= 1).all() and (rec[:, 0] < 20).all()
    for i in np.unique(rec[:, 0]):
        r = rec[rec[:, 0] == i]
        assert (r[1:, 1] >= r[:-1, 1] + r[:-1, 2]).all(), f"individual {i}: ranges overlap"
        assert r[0, 1] >= 0 and r[-1, 1] + r[-1, 2] <= S
    inner = cuts[1:-1]
    ends = {b for i, _, b in got if i == cu.RANGE_INDS[0]}
    begins = {a for i, a, _ in got if i == cu.RANGE_INDS[1]}
    assert begins == set(inner) and ends <= {c - 1 for c in inner} and len(ends) >= len(inner) - 1
    for a, b in cu.shards(cuts):
        if b - a == 1 and 0 < a < S - 1:
            assert (cu.RANGE_INDS[1], a, a) in got            # a one-site range on a one-site shard
    i3 = [(a, b) for i, a, b in got if i == cu.RANGE_INDS[2]]
    assert len(i3) == 1 and _shard_of(cuts, i3[0][1]) - _shard_of(cuts, i3[0][0]) + 1 >= min(3, len(cuts) - 1)


def test_reach_on_a_made_up_chain():
    """The restatement against windows counted by hand: 30 sites, a chromosome start at 20."""
    pos = np.full(30, 0.5)
    pos[0] = pos[20] = np.inf
    cuts = [0, 8, 12, 30]
    # L = 5 sites: from site 7 the window ends at 11 (4 past the cut at 8: exactly the next shard);
    # from site 11 it ends at 15 (4 past 12); into site 8 it begins at 4 (4 before the cut)
    assert cu.reach(pos, cuts, 5, "sites") == ([4, 4, 0], [0, 4, 4])
    assert cu.admitted(pos, cuts, 5, "sites", "ibd_by_length") and cu.admitted(pos, cuts, 5, "sites", "ibd_long")
    # L = 6: 5 past the cut at 8, the shard behind holds 4
    assert cu.reach(pos, cuts, 6, "sites")[0][0] == 5
    assert not cu.admitted(pos, cuts, 6, "sites", "ibd_by_length")
    assert cu.reach(pos, cuts, 6, "sites")[1] == [0, 5, 5] and not cu.admitted(pos, cuts, 6, "sites", "ibd_long")
    # a window ends at the data's and at a chromosome's first site at the latest: into [2, 12) the
    # windows of 6 sites reach back 2 (site 5 from site 0), not 5; behind the start at 20 likewise
    far, back = cu.reach(pos, [0, 2, 12, 30], 6, "sites")
    assert far == [5, 5, 0] and back == [0, 2, 5]
    far, back = cu.reach(pos, [0, 18, 22, 30], 6, "sites")
    assert far == [2, 5, 0] and back == [0, 5, 2]                    # (19 is the last site of its chromosome)
    # no window inside a chromosome: nothing reaches anywhere
    assert cu.reach(pos, cuts, 21, "sites") == ([0, 0, 0], [0, 0, 0]) and not cu.crosses(pos, cuts, 21, "sites")
    # Mb: 0.5 per step; 2 Mb = 5 sites
    assert cu.reach(pos, cuts, 2.0, "mb") == cu.reach(pos, cuts, 5, "sites")
    assert cu.reach(pos, cuts, 0.0, "mb") == ([0, 0, 0], [0, 0, 0])


def test_thresholds_on_the_geometries(geo):
    """What the device test relies on: every geometry admits, per unit and entry point, a threshold
    of COHORT_LEN whose window crosses a cut; B in sites admits 80 and refuses 81; D admits 400
    sites and refuses 700.  (2000 sites exceed every chromosome: no window exists, so nothing
    reaches past a shard and every chain takes it; the answer is 0.)"""
    pos, k, G, _ = geo
    print()
    for name, cuts in G.items():
        lengths = cu.admitted_lengths(pos, cuts)
        print(f"  {name} {cuts}: " + "; ".join(f"{e} {u} {lengths[e][u]}" for e in lengths for u in lengths[e]))
        for e in lengths:
            for u, L in lengths[e].items():
                assert any(cu.crosses(pos, cuts, l, u) for l in L), (name, e, u)
                assert cu.admitted(pos, cuts, 2000, "sites", e) and not cu.crosses(pos, cuts, 2000, "sites")
            assert set(lengths["ibd_long"][u]) <= set(lengths["ibd_by_length"][u])
    for e in ("ibd_by_length", "ibd_long"):
        assert cu.admitted(pos, G["B"], 80, "sites", e) and not cu.admitted(pos, G["B"], 81, "sites", e)
        assert cu.admitted(pos, G["D"], 400, "sites", e) and not cu.admitted(pos, G["D"], 700, "sites", e)
    far, back = cu.reach(pos, G["B"], 80, "sites")
    assert far[0] == 79 and back[2] == 79
    assert cu.reach(pos, G["B"], 81, "sites")[0][0] == 80
    # something is refused in Mb too
    assert any(not cu.admitted(pos, cuts, l, "mb", "ibd_long") for cuts in G.values() for l in bu.COHORT_LEN["mb"])
