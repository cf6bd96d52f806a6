"""Keeps the rules of the layout tests (tests/layout_util.py) total over the battery of
tests/replica_util.py, and checks their tolerances and the extra region and range sets where no
device is needed."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import bounds_util
import bylength_util as bu
import info_util
import layout_util as lu
import replica_util as ru
import support_util as sup


def _battery_keys():
    """The keys battery() writes, from its source: every _records(out, "...") with {u} and {tag}
    filled in, and below each the components that tuples and dicts add."""
    src = inspect.getsource(ru.battery)
    names = re.findall(r'_records\(out, f?"([^"]+)"', src)
    assert len(names) == len(re.findall(r"_records\(out,", src)) > 30
    keys = []
    for n in names:
        for u in bu.COHORT_LEN:
            keys.append(n.replace("{u}", u).replace("{tag}", "whole"))
    return sorted(set(keys))


def test_every_battery_key_has_exactly_one_rule():
    keys = _battery_keys()
    assert {"gl", "marg_prob", "ibd_moments.mb.whole", "ibd_summary.posterior.whole", "tract_bounds.hand",
            "mstep_freq.e_prob", "obs_info.at"} <= set(keys)
    for k in keys:
        for full in (k, k + ".0", k + ".regions"):        # (tuples and dicts add components)
            assert len(lu.rule_of(full)) == 1, (full, lu.rule_of(full))
    # ... and no rule is left over from a key the battery no longer writes
    heads = {k.split(".")[0] for k in keys}
    assert set(lu.RULES) == heads
    assert all(callable(r) for r in lu.RULES.values())


def test_forced_layout_restores_the_environment(monkeypatch):
    monkeypatch.delenv(lu.ENV, raising=False)
    with lu.forced_layout(7):
        assert os.environ[lu.ENV] == "7"
    assert lu.ENV not in os.environ
    with lu.forced_layout(None):
        assert lu.ENV not in os.environ
    monkeypatch.setenv(lu.ENV, "3")
    with pytest.raises(RuntimeError):
        with lu.forced_layout(9):
            assert os.environ[lu.ENV] == "9"
            raise RuntimeError
    assert os.environ[lu.ENV] == "3"
    with lu.forced_layout(0):                              # the layout's own C inside
        assert lu.ENV not in os.environ
    assert os.environ[lu.ENV] == "3"


def test_tolerances_are_finite_and_positive():
    assert len(lu.TOLERANCES) > 25
    for k, v in lu.TOLERANCES.items():
        assert math.isfinite(v) and v > 0, k
    for v in (lu.SITES_DIFFER, lu.ANCHORS_DIFFER, lu.MIN_SITE_DIFFER):
        assert 0 < v < 1


def _sorted_disjoint(reg, S):
    reg = np.asarray(reg)
    return bool((reg[:, 0] < reg[:, 1]).all() and (reg[1:, 0] >= reg[:-1, 1]).all()
                and reg[0, 0] >= 0 and reg[-1, 1] <= S)


def _ranges_ok(ranges, n_ind, S):
    rec = sup.to_records(ranges)
    assert len(rec) == len(set(ranges)) and (rec[:, 2] >= 1).all() and (rec[:, 0] < n_ind).all()
    for i in np.unique(rec[:, 0]):
        r = rec[rec[:, 0] == i]
        assert (r[1:, 1] >= r[:-1, 1] + r[:-1, 2]).all(), f"individual {i}: ranges overlap"
        assert r[0, 1] >= 0 and r[-1, 1] + r[-1, 2] <= S
    return rec


@pytest.mark.parametrize("S,T", [(6145, 24), (3073, 32), (9217, 24)])
def test_tail_sets(S, T):
    """The sets of the padded cases, at the (S, T) those cases assert on the device."""
    assert S % T == 1
    sets = lu.tail_regions(S, T)
    for reg in sets.values():
        assert _sorted_disjoint(reg, S)
    one = sets["tail1"]
    assert (one[:, 1] - one[:, 0] == 1).all()
    last_lane = (lu.lanes_used(S, T) - 1) * T
    assert last_lane == S - 1
    assert {S - 1, S - 2, last_lane, last_lane - T} <= set(one[:, 0].tolist())
    assert sets["tail"].tolist() == [[S - T - 3, S]]
    pos = np.full(S, 0.01)
    pos[0] = pos[S // 3] = pos[2 * S // 3] = np.inf
    hand = sup.hand_ranges(20, S, pos, T)
    tail = lu.tail_ranges(S, T)
    assert not {i for i, _, _ in hand} & {i for i, _, _ in tail}
    rec = _ranges_ok(hand + tail, 20, S)
    ends = rec[:, 1] + rec[:, 2] - 1
    at_end = rec[ends == S - 1]
    assert len(at_end) >= 4 and 1 in at_end[:, 2] and (at_end[:, 2] > 2 * T).any()


@pytest.mark.parametrize("T,C", [(88, 48), (64, 65), (32, 129)])
def test_wave_edge_sets(T, C):
    """The sets of the long case: single sites on both sides of every wave edge, ranges across."""
    I, S = lu.LONG_SHAPE
    W = 64 * T
    reg = lu.edge_sites(S, T)
    assert _sorted_disjoint(reg, S) and (reg[:, 1] - reg[:, 0] == 1).all() and 24 <= len(reg) <= 400
    edges = np.arange(W, S, W)
    assert np.isin(edges, reg[:, 0]).all() and np.isin(edges - 1, reg[:, 0]).all()
    assert (np.isin(reg[:, 0] % T, (0, T - 1)) | np.isin(reg[:, 0], (0, S - 1))).all()
    pos = np.full(S, 0.001)
    pos[0] = pos[100_003] = np.inf
    rec = _ranges_ok(lu.wave_ranges(S, T, pos), I, S)
    a, b = rec[:, 1], rec[:, 1] + rec[:, 2] - 1
    assert ((a // W) != (b // W)).sum() >= 3
    assert np.isin(b[rec[:, 0] == 0] + 1, edges).any() and np.isin(a[rec[:, 0] == 0], edges).any()
    assert ((rec[:, 0] == 1) & (b - a > 4 * W)).any() and ((rec[:, 0] == 1) & (a == b)).sum() == 2


def _fake_bounds(pkg, model, pos, rec, anchors, levels):
    """What a handle's tract_bounds returns, made of the yardstick (bounds_util.bounds_ref)."""
    r = bounds_util.bounds_ref(model, pos, rec, anchors, levels)
    bd = np.zeros(len(rec), dtype=pkg.TRACT_BOUND_DTYPE)
    for f in ("anchor", "left_limit", "right_limit", "post_anchor", "log_reach_left", "log_reach_right"):
        bd[f] = r[f]
    bd["reach_left"], bd["reach_right"] = np.exp(bd["log_reach_left"]), np.exp(bd["log_reach_right"])
    return bd, r["start"].astype(np.uint64), r["end"].astype(np.uint64)


def test_the_bounds_rule_brackets_every_site(pkg):
    """rule_bounds on answers made of the numpy yardstick: equal answers pass; ONE quantile site
    moved by a site or two, or one wrong anchor posterior, fails."""
    eprob, pos = info_util.random_case(5, 4, 900)
    F, A = np.array([0.3, 0.5, 0.7, 0.2]), np.array([0.02, 0.4, 1e-3, 1.5])
    model = bounds_util.FormB(eprob, pos, F, A)
    rec = sup.to_records([(0, 5, 80), (0, 200, 200), (1, 10, 290), (1, 310, 420), (2, 0, 899), (3, 450, 600),
                          (3, 601, 640)])
    key = "tract_bounds.hand"

    def answers():
        bd, s, e = _fake_bounds(pkg, model, pos, rec, None, bounds_util.LEVELS)
        anc = bd["anchor"]
        probe = {key: (_fake_bounds(pkg, model, pos, rec, anc, bounds_util.LEVELS),
                       _fake_bounds(pkg, model, pos, rec, anc, lu.bracket_levels()))}
        return {f"{key}.0": bd, f"{key}.1": s, f"{key}.2": e}, probe

    def failed(got, ref, probe):
        ctx = lu.Context(4, 900, pos, {}, F, A, probe)
        rep = lu.Report()
        lu.rule_bounds(rep, "tract_bounds", got, ref, ctx)
        return [label for label, _, _ in rep.failed]

    ref, probe = answers()
    got, _ = answers()
    assert failed(got, ref, probe) == []
    assert failed(got, ref, {}) == [f"{key} probe"]
    # one start inside its limits, moved towards the anchor
    s = got[f"{key}.1"]
    k = int(np.argmax(got[f"{key}.0"]["anchor"].astype(np.int64) - s[:, 0].astype(np.int64)))
    assert int(got[f"{key}.0"]["anchor"][k]) - int(s[k, 0]) >= 3
    s[k, 0] += 2
    assert f"{key} start bracket" in failed(got, ref, probe)
    got, _ = answers()
    e = got[f"{key}.2"]
    k = int(np.argmax(e[:, 2].astype(np.int64) - got[f"{key}.0"]["anchor"].astype(np.int64)))
    e[k, 2] -= 1
    assert f"{key} end bracket" in failed(got, ref, probe)
    got, _ = answers()
    got[f"{key}.0"]["post_anchor"][3] *= 1 - 1e-9
    assert {f"{key} post_anchor", f"{key} post_anchor own"} <= set(failed(got, ref, probe))
