"""Every output entry point on multi-start replicas (nghmm_create_replica, include/nghmm.h: "every
call behaves exactly as on an independent handle loaded with the same data").  A replica borrows
its parent's likelihoods in every layout and owns what an EM run writes; each output entry point
reaches the likelihoods by a route of its own, keeps scratch by the handle and reads the handle's
parameters, emissions, posteriors, decoded path and flags.  The command line runs all of them on a
replica whenever replicate 1 does not win (tests/test_gpu_multistart.py has that test).

The battery of tests/replica_util.py runs one EM iteration, a decode and every output on the
20 x 5003 cohort of the output tests; every comparison is bytes == bytes against an independent
handle (both modes are deterministic: there is no tolerance to choose).  The independent runs are
made once per mode and shared by the tests."""
import ctypes as C

import numpy as np
import pytest

import replica_util as ru
import support_util as sup
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

VARIANTS = [("fast", False), ("exact", False), ("fast", True), ("exact", True)]
IDS = ["fast-dense", "exact-dense", "fast-packed", "exact-packed"]


@pytest.fixture(scope="module")
def cohort(pkg):
    return sup.gpu_cohort(pkg)


@pytest.fixture(scope="module")
def region_sets(pkg, cohort):
    """{mode: regions of the battery}; the single-site regions of "edges" sit on both sides of the
    lane-chunk edges of the layout the device reports for the cohort."""
    d = cohort[0]
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST) as h:
        lane_sites = h.layout()[1]
    assert 0 < lane_sites < d.n_sites
    return {m: ru.cohort_regions(pkg, cohort, m, lane_sites) for m in ("fast", "exact")}


@pytest.fixture(scope="module")
def want(pkg, cohort, region_sets):
    """want(mode_name, packed, k): two batteries from start k on an independent handle, one handle
    after the other; made once and left unchanged."""
    d = cohort[0]
    starts = ru.starts(d.n_ind, d.n_sites, 3)
    cache = {}

    def get(mode_name, packed, k):
        key = (mode_name, packed, k)
        if key not in cache:
            cache[key] = ru.independent(pkg, cohort, ru.mode_of(pkg, mode_name, packed), packed,
                                        starts[k], region_sets[mode_name])
        return cache[key]
    get.starts = starts
    return get


def _parent(pkg, cohort, mode_name, packed):
    d = cohort[0]
    h = pkg.NgsFHMM(d.n_ind, d.n_sites, mode=ru.mode_of(pkg, mode_name, packed))
    ru.load(pkg, h, cohort, packed)
    return h


def _round(out, r):
    return {k: v for k, v in out.items() if k.startswith(f"{r}:")}


def _same(got, want, who):
    assert list(got) == list(want), who
    bad = ru.differing(got, want)
    assert not bad, f"{who} differs from an independent handle at {bad}"


@pytest.mark.parametrize("mode_name,packed", VARIANTS, ids=IDS)
def test_replica_outputs_equal_an_independent_handle(pkg, cohort, region_sets, want, mode_name, packed):
    """The parent from start A, one replica from start B, the batteries interleaved (parent,
    replica, parent, replica): every key of the replica is that of an independent handle from B,
    every key of the parent that of one from A.  The two starts differ in every key but the data
    itself, so an output read from the other handle's state, or a scratch buffer keyed to the wrong
    handle, shows (tests/test_replica_battery_cpu.py checks the starts on the oracle)."""
    regions = region_sets[mode_name]
    A, B = want.starts[:2]
    want_A, want_B = want(mode_name, packed, 0), want(mode_name, packed, 1)
    same = [k for k in want_A if not ru.is_data(k) and want_A[k] == want_B[k]]
    assert not same, f"the two starts give the same bytes at {same}: the comparison would be empty there"
    assert all(want_A[k] == want_B[k] for k in want_A if ru.is_data(k))
    parent = _parent(pkg, cohort, mode_name, packed)
    rep = parent.replica()
    try:
        got_A, got_B = {}, {}
        ru.reset(parent, A)
        got_A.update({f"1:{k}": v for k, v in ru.battery(pkg, parent, regions).items()})
        state_A = ru.probe(pkg, parent)
        ru.reset(rep, B)
        got_B.update({f"1:{k}": v for k, v in ru.battery(pkg, rep, regions).items()})
        state_B = ru.probe(pkg, rep)
        # (a battery rewrites the handle's EM state before it reads it: what the OTHER handle's run
        # did to this one's state shows only in between)
        bad = ru.differing(ru.probe(pkg, parent), state_A)
        assert not bad, f"the replica's run changed the parent's state at {bad}"
        got_A.update({f"2:{k}": v for k, v in ru.battery(pkg, parent, regions).items()})
        bad = ru.differing(ru.probe(pkg, rep), state_B)
        assert not bad, f"the parent's run changed the replica's state at {bad}"
        got_B.update({f"2:{k}": v for k, v in ru.battery(pkg, rep, regions).items()})
        _same(got_B, want_B, "the replica")
        _same(got_A, want_A, "the parent")
    finally:
        rep.close()
        parent.close()


@pytest.mark.parametrize("mode_name,packed", VARIANTS, ids=IDS)
def test_parent_is_untouched_by_its_replicas(pkg, cohort, region_sets, want, mode_name, packed):
    """The parent's battery before any replica exists; two replicas run the whole battery from
    other starts; the parent's battery from the same reset state and its following iter_EM are
    those of a handle that never had replicas; so is its next battery after each replica is closed
    -- the replica made first goes first for the dense variants, last for the packed ones, so that
    both orders are run."""
    regions = region_sets[mode_name]
    A, B, Cc = want.starts
    want_A = want(mode_name, packed, 0)
    parent = _parent(pkg, cohort, mode_name, packed)
    reps = []
    try:
        _same(ru.run(pkg, parent, A, regions, rounds=1), _round(want_A, 1), "the parent before any replica")
        reps = [parent.replica(), parent.replica()]
        _same(ru.run(pkg, reps[0], B, regions, rounds=1), _round(want(mode_name, packed, 1), 1), "replica 1")
        ru.run(pkg, reps[1], Cc, regions, rounds=1)      # (test_concurrent_output_calls compares this start)
        _same(ru.run(pkg, parent, A, regions, rounds=1), _round(want_A, 1), "the parent after its replicas ran")
        parent.iter_EM()
        for k in ("indF", "alpha", "freq", "ind_lkl", "marg_prob"):
            assert getattr(parent, k).tobytes() == want_A[f"2:{k}"], f"the parent's next iter_EM: {k}"
        for r in (reps if not packed else reps[::-1]):
            r.close()
            _same(ru.run(pkg, parent, A, regions, rounds=1), _round(want_A, 1),
                  "the parent after a replica was closed")
    finally:
        for r in reps:
            if not r.closed:
                r.close()
        parent.close()


@pytest.mark.parametrize("mode_name,packed", VARIANTS, ids=IDS)
def test_concurrent_output_calls(pkg, cohort, region_sets, want, mode_name, packed):
    """Parent and two replicas, one host thread and one stream each, every thread two batteries:
    the three sequential independent runs, key by key."""
    regions = region_sets[mode_name]
    parent = _parent(pkg, cohort, mode_name, packed)
    hs = [parent, parent.replica(), parent.replica()]
    try:
        got = ru.in_threads([lambda h=h, s=s: ru.run(pkg, h, s, regions) for h, s in zip(hs, want.starts)])
        for k, g in enumerate(got):
            _same(g, want(mode_name, packed, k), "the parent" if k == 0 else f"replica {k}")
    finally:
        for h in hs[:0:-1]:
            h.close()
        parent.close()


def _refused(pkg, call):
    with pytest.raises(pkg.NgsFHMMError) as ei:
        call()
    assert ei.value.code == -10 and ei.value.message and ei.value.message != "invalid argument", ei.value
    return ei.value.message


@pytest.mark.parametrize("mode_name,packed", VARIANTS, ids=IDS)
def test_replica_contract_errors(pkg, mode_name, packed):
    """What a replica and a parent with live replicas refuse, each with NGHMM_ERR_ARG and a
    message: a replica of a replica, loads, chains, groups, site shards.  A replica made before the
    parent's first decode has no decoded path of its own, whatever the parent has decoded since."""
    I, S = 8, 300
    d = pkg.simulate.simulate(I, S, seed=5, n_chrom=2, indF=0.4, alpha=0.1)
    mode = ru.mode_of(pkg, mode_name, packed)
    gl = pkg.simulate.normalise_log_gl(d.gl)

    def fresh():
        h = pkg.NgsFHMM(I, S, mode=mode)
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=packed)
        h.set_params(0.4, 0.1, 0.2)
        h.init_emission()
        return h
    parent, other = fresh(), fresh()
    rep = parent.replica()
    try:
        rep.set_params(0.2, 0.3, 0.1)
        rep.init_emission()
        assert "replica" in _refused(pkg, rep.replica)
        pos = np.ascontiguousarray(d.pos_dist_mb, dtype=np.float64)
        for h in (rep, parent):          # the data belong to the parent, and not while replicas read them
            assert "replica" in _refused(pkg, lambda: h.load(gl, d.pos_dist_mb))
            assert "replica" in _refused(pkg, lambda: h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=packed))
            assert "replica" in _refused(pkg, lambda: h._check(h.lib.nghmm_load_begin(
                h.handle, pos.ctypes.data_as(C.POINTER(C.c_double)))))
            for setup in (pkg.Chain, pkg.Group):
                _refused(pkg, lambda: setup([other, h]))
                _refused(pkg, lambda: setup([h, other]))
            msg = _refused(pkg, lambda: h.site_shard_setup(0, 1, 0, 0, 0, None))
            assert mode_name != "fast" or "replica" in msg
        # the refused loads left the data and both handles usable; the parent decodes, the replica
        # has not: the parent's path_decoded must not leak
        parent.iter_EM()
        parent.viterbi()
        parent.ibd_tracts("viterbi")
        for call in (lambda: rep.ibd_sharing("viterbi"), lambda: rep.ibd_tracts("viterbi"),
                     lambda: rep.ibd_summary(pkg.chromosome_regions(d.pos_dist_mb), "viterbi"),
                     lambda: rep.ibd_expect(viterbi=True)):
            assert "no Viterbi decode" in _refused(pkg, call)
        rep.iter_EM()
        path = rep.viterbi()
        assert rep.ibd_sharing("viterbi")["vit_both"].trace() == int(path.sum())
        late = parent.replica()          # ... nor does a replica made after the parent's decode inherit it
        try:
            assert "no Viterbi decode" in _refused(pkg, lambda: late.ibd_tracts("viterbi"))
        finally:
            late.close()
    finally:
        rep.close()
        parent.close()
        other.close()
