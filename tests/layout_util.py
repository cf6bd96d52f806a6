"""Fast-mode layouts for the tests (tests/test_gpu_layouts.py): a handle cuts every individual's site
axis into 64 C lanes of T sites (C waves per individual; NgsFHMM.layout() reports (C, T)), and
every walk-shaped kernel combines lanes in a wave, waves in an individual and pieces in a region,
and neutralises the padded cells behind site S - 1.

forced_layout sets NGHMM_FAST_C around the creation of a handle.  compare() holds one battery of
tests/replica_util.py (array form, estep() first, parameters as set) to the battery of a handle of
the same data at another layout, key by key, by the rules of RULES:

  bytes      the same bytes: the data, the parameters as set, everything whose walk is one lane per
             individual and chromosome over site-major data (freq_info, geno_smooth, ibd_longest:
             the header promises a chain "the single handle's bytes" for them), the decoded path,
             the drawn paths and what is counted on a path;
  restated   from the handle's OWN read-backs (marg_prob, path) by tracts_util, summary_util and
             sharing_util, with the equalities and bounds of their own device tests;
  tolerance  within twice the tolerance that the entry point's own test file applies to the device
             against its yardstick on the 20 x 5003 cohort (both handles are within that tolerance
             of the yardstick: the triangle inequality), times ctx.scale for longer data.

No bound here is taken from a device's output.  tests/test_layouts_cpu.py keeps RULES total over
the battery's keys.  tests/chain_util.py reuses the rules, with named overrides, for a chain of
site shards against one handle."""
import collections
import contextlib
import math
import os

import numpy as np

import bounds_util
import bylength_util
import expect_util as xu
import info_util
import long_util
import moments_util
import replica_util as ru
import sharing_util
import summary_util
import support_util as sup
import tracts_util

ENV = "NGHMM_FAST_C"
U = 2.0 ** -53

# ind_lkl and lkl: 2 x the 1e-13 relative that tests/test_gpu_fast.py
# (test_fast_more_than_64_waves_per_individual) allows against the binary128 anchor
LKL_RTOL = 2e-13
# marg_prob: 2 x its 1e-13 absolute; posteriors are snapped to 0 / 1 at 1e-5, and at most two cells
# per individual may be snapped differently (a value next to 1e-5), as there
POST_ATOL = 2e-13
SNAP = 1e-5
SNAPPED_CELLS = 2
# frequencies "1e-12 given the same posteriors" (EXACT_TOL of tests/test_gpu_estmaf_injected.py), and
# the log emissions made of them; a logarithm of a value next to 1 carries the rounding of the
# value itself (2^-53 absolute, twice for two handles, twice for the sum in front of it)
# -- an absolute term ON TOP of the 1e-12 relative that the frequency step's check is specified
# with: a deliberate deviation, 4.4e-16 in size
FREQ_RTOL = 1e-12
EPROB_ATOL = 4 * U
# ibd_mb of a drawn path: 2 x the 1e-12 relative of tests/test_gpu_sample.py (the order in which
# the lanes' distances are added follows the layout; the counts are integers) -- a deliberate
# deviation from "the same bytes" for this one field of sample_paths; the paths and counts are bytes
DRAW_MB_RTOL = 2e-12
# tract_bounds (tests/test_gpu_bounds.py): fewer than 1 % of all (record, level, side) sites may
# differ at all, at most 2 % of the auto anchors (a runner-up within the tolerance)
SITES_DIFFER, ANCHORS_DIFFER = 0.01, 0.02
# tract_support (tests/test_gpu_support.py): fewer than 2 % of the ranges may have their smallest
# posterior at another site (a runner-up within the tolerance)
MIN_SITE_DIFFER = 0.02


@contextlib.contextmanager
def forced_layout(fast_c):
    """NGHMM_FAST_C = fast_c around the creation of a handle (nghmm_create reads it once); None or
    0: the layout's own C.  The environment is restored."""
    old = os.environ.get(ENV)
    if fast_c:
        os.environ[ENV] = str(int(fast_c))
    else:
        os.environ.pop(ENV, None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


def handle(pkg, cohort, packed=False, fast_c=None):
    """A fast-mode handle of the cohort (support_util.gpu_cohort's tuple), loaded, with the
    cohort's parameters set and the emissions made."""
    d, gl, F, A, freq = cohort
    with forced_layout(fast_c):
        h = pkg.NgsFHMM(d.n_ind, d.n_sites, mode=ru.mode_of(pkg, "fast", packed))
    ru.load(pkg, h, cohort, packed)
    ru.reset(h, (F, A, freq))
    return h


# More than 64 waves per individual need 32 sites per lane (fast_create's floor): 129 waves, 256 003
# sites.
LONG_SHAPE = (2, 256_003)


def long_cohort(pkg):
    """2 x 256 003, two chromosomes of unequal length (the second starts at site 100 003), missing
    cells; alpha = 1e-3 for individual 0 (tracts that span many waves).  The tuple of
    support_util.gpu_cohort."""
    I, S = LONG_SHAPE
    d = pkg.simulate.simulate(I, S, seed=43, n_chrom=2, indF="r", alpha="r", missing_rate=0.03)
    pos = d.pos_dist_mb
    mid = int([x for x in np.flatnonzero(np.isinf(pos)) if x > 0][0])
    pos[mid] = pos[mid - 1]
    pos[100_003] = np.inf
    return d, pkg.simulate.normalise_log_gl(d.gl), np.array([0.6, 0.25]), np.array([1e-3, 0.4]), 0.15


def lanes_used(n_sites, lane_sites):
    return -(-n_sites // lane_sites)


def describe(h):
    """(C, T, lanes used, wholly empty waves) of a fast-mode handle."""
    C, T = h.layout()
    used = lanes_used(h.n_sites, T)
    return C, T, used, (64 * C - used) // 64


# ---------------------------------------------------------------------------------------------
# region and range sets

def _one(sites):
    s = np.unique(np.asarray(sites, dtype=np.int64))
    return np.stack([s, s + 1], axis=1)


def tail_regions(n_sites, lane_sites):
    """Case b (a last used lane of one site, empty waves behind it): one-site regions at S - 2,
    S - 1 and the first site of the last used lane (S - 1 itself when S % T == 1) and of the lane
    before it; and the region [S - T - 3, S), which ends in that lane."""
    S, T = n_sites, lane_sites
    last = (lanes_used(S, T) - 1) * T
    return collections.OrderedDict([
        ("tail1", _one([S - 2, S - 1, last, last - T])),
        ("tail", np.array([[S - T - 3, S]], dtype=np.int64))])


def tail_ranges(n_sites, lane_sites):
    """Case b, for tract_support / tract_bounds: ranges [(ind, first, last)] that end at S - 1 --
    of one site, of the last two lanes, of many lanes -- for individuals 6 to 9, which
    support_util.hand_ranges leaves alone."""
    S, T = n_sites, lane_sites
    return [(6, S - 1, S - 1), (7, S - T - 3, S - 1), (8, S - 40 * T - 5, S - 1),
            (9, S - T - 1, S - T - 1), (9, S - 2, S - 1)]


def edge_sites(n_sites, lane_sites):
    """Case c: single sites on both sides of every wave edge (multiples of 64 T) and of a few dozen
    lane edges spread over the data, with site 0 and S - 1."""
    S, T = n_sites, lane_sites
    w = np.arange(64 * T, S, 64 * T)
    lanes = np.arange(T, S, T)
    lanes = lanes[:: max(1, len(lanes) // 24)]
    return _one(np.r_[w - 1, w, lanes - 1, lanes, 0, S - 1])


def wave_ranges(n_sites, lane_sites, pos):
    """Case c (two individuals), for tract_support / tract_bounds: individual 0 -- ranges that end
    on the last site of a wave, begin on the first, and lie across a wave edge, in turn over the
    wave edges; individual 1 -- the whole first chromosome less a site, one-site ranges at a wave
    edge, a range across many waves with odd ends.  Sorted, disjoint within an individual."""
    S, T = n_sites, lane_sites
    W = 64 * T
    out = []
    for n, t in enumerate(range(W, S - 8, W)):
        if n % 3 == 0:
            out.append((0, t - 5, t - 1))
        elif n % 3 == 1:
            out.append((0, t, t + 4))
        else:
            out.append((0, t - 3, t + 3))
    cs = [int(x) for x in np.flatnonzero(np.isinf(pos)) if x > 0]
    a = cs[0] if cs else S // 2
    out.append((1, 1, a - 2))
    t = (a // W + 1) * W
    out += [(1, t - 1, t - 1), (1, t, t), (1, t + 3, min(t + 5 * W + 11, S - 2))]
    return sorted(set(out))


# ---------------------------------------------------------------------------------------------
# the rules

class Context:
    """What the rules need besides the two batteries: the data's shape and distances, the region
    sets the batteries were asked with, the other handle's tract_bounds at this handle's anchors
    (bounds_probe), the parameters as set, and the factor
    on the cohort tolerances (1 on the cohort; ceil(S / 5003) on longer data: the roundings grow
    about linearly with the chain, DESIGN.md section 4 and the drift table of section 5)."""

    def __init__(self, n_ind, n_sites, pos, regions, F, A, bounds=None, scale=1):
        self.I, self.S, self.pos = n_ind, n_sites, np.asarray(pos, dtype=np.float64)
        self.regions, self.bounds, self.scale = regions, bounds or {}, scale
        self.F = np.broadcast_to(np.asarray(F, dtype=np.float64), (n_ind,))
        self.A = np.broadcast_to(np.asarray(A, dtype=np.float64), (n_ind,))
        self.cs = xu.chrom_start(self.pos)


class Report:
    """Worst error / bound per label; the failures, raised together at the end."""

    def __init__(self):
        self.ratio = collections.OrderedDict()
        self.failed = []

    def add(self, label, ratio, note=""):
        ratio = float(ratio)
        self.ratio[label] = max(self.ratio.get(label, 0.0), ratio)
        if not ratio <= 1.0:
            self.failed.append((label, ratio, note))

    def need(self, label, ok, note=""):
        self.add(label, 0.0 if ok else math.inf, note)

    def worst_per_key(self):
        out = collections.OrderedDict()
        for label, r in self.ratio.items():
            k = label.split(" ", 1)[0]
            out[k] = max(out.get(k, 0.0), r)
        return out


def _ratio(err, bound):
    """Largest err / bound; inf where the bound is 0 and the error is not."""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    if err.size == 0:
        return 0.0
    if np.isnan(err).any():
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _keys(d, name):
    return [k for k in d if k == name or k.startswith(name + ".")]


def _fields(rep, key, got, ref, tol, scale=1, minus_inf=False):
    """Every field of a record array within scale x 2 x tol[field] of the reference handle's."""
    rep.need(f"{key} shape", got.shape == ref.shape and got.dtype == ref.dtype)
    for f in got.dtype.names:
        g, r = got[f], ref[f]
        rep.need(f"{key} {f} nan", not np.isnan(g).any())
        ok = np.ones(g.shape, dtype=bool)
        if minus_inf:
            ok = ~np.isneginf(r)
            rep.need(f"{key} {f} -inf", np.array_equal(np.isneginf(g), ~ok), "-inf in the same places")
        else:
            rep.need(f"{key} {f} finite", np.isfinite(g).all())
        err = np.where(ok, np.abs(np.where(ok, g, 0.0) - np.where(ok, r, 0.0)), 0.0)
        at = np.unravel_index(int(np.argmax(err)), err.shape) if err.size else ()
        note = f"|{g[at]!r} - {r[at]!r}| = {err[at]:.3e} at {tuple(int(x) for x in at)}, bound {2 * scale * tol[f]:.3e}" \
            if err.size else ""
        rep.add(f"{key} {f}", _ratio(err, 2 * scale * tol[f]), note)


def rule_bytes(rep, name, got, ref, ctx):
    for k in _keys(got, name):
        a, b = got[k], ref[k]
        same = a == b if isinstance(a, bytes) else (a.dtype == b.dtype and a.shape == b.shape
                                                    and a.tobytes() == b.tobytes())
        rep.need(k, same, "bytes differ")


def rule_lkl(rep, name, got, ref, ctx):
    rep.add(name, _ratio(np.abs(got[name] - ref[name]), LKL_RTOL * np.abs(ref[name])))


def rule_marg(rep, name, got, ref, ctx):
    g, r = got[name], ref[name]
    snapped = (g != r) & ((g == 0) | (g == 1) | (r == 0) | (r == 1))
    rep.add(f"{name} snapped", snapped.sum(axis=1).max() / SNAPPED_CELLS)
    rep.need(f"{name} snap", (np.abs(g - r)[snapped] <= SNAP + POST_ATOL).all(), "a snapped cell far from 1e-5")
    rep.add(name, _ratio(np.abs(g - r)[~snapped], POST_ATOL))


def eprob_ratio(got, ref):
    return _ratio(np.abs(got - ref), FREQ_RTOL * np.abs(ref) + EPROB_ATOL)


def rule_eprob(rep, name, got, ref, ctx):
    rep.need(f"{name} -inf", np.array_equal(np.isneginf(got[name]), np.isneginf(ref[name])))
    fin = np.isfinite(ref[name])
    rep.add(name, eprob_ratio(got[name][fin], ref[name][fin]))


def rule_mstep_freq(rep, name, got, ref, ctx):
    if f"{name}.freq" not in got:             # (an estep-only battery has no frequency step)
        return
    rep.add(f"{name}.freq", _ratio(np.abs(got[f"{name}.freq"] - ref[f"{name}.freq"]),
                                   FREQ_RTOL * np.abs(ref[f"{name}.freq"])))
    rule_eprob(rep, f"{name}.e_prob", got, ref, ctx)


def rule_format(rep, name, got, ref, ctx):
    """The .ibd file's posterior lines are "%f" of the handle's own marg_prob."""
    marg = got["marg_prob"]
    I = ctx.I
    lo, n = ru.posterior_part(I)
    for k, rows in ((name, range(I)), (f"{name}.part", range(lo, lo + n))):
        want = b"".join("\t".join("%f" % v for v in marg[i]).encode() + b"\n" for i in rows)
        rep.need(k, got[k] == want, "not printf(\"%f\") of the handle's own posteriors")


def rule_draws(rep, name, got, ref, ctx):
    rule_bytes(rep, f"{name}.1", got, ref, ctx)
    g, r = got[f"{name}.0"], ref[f"{name}.0"]
    for f in g.dtype.names:
        if g.dtype[f].kind == "f":
            rep.add(f"{name}.0 {f}", _ratio(np.abs(g[f] - r[f]), DRAW_MB_RTOL * np.abs(r[f])))
        else:
            rep.need(f"{name}.0 {f}", np.array_equal(g[f], r[f]))


def rule_tracts(rep, name, got, ref, ctx):
    """tests/test_gpu_tracts.py: the coordinates of tracts_util.rle_tracts on the handle's own path
    / posteriors, post_sum within 1e-12 relative, post_mean = post_sum / n_sites."""
    marg, path = got["marg_prob"], got["path"]
    for k, state, min_sites in ((f"{name}.viterbi", path != 0, 1), (f"{name}.posterior", marg >= 0.5, 3)):
        t = got[k]
        want = tracts_util.rle_tracts(state, ctx.cs, marg, min_sites)
        coords = [(int(x["ind"]), int(x["first_site"]), int(x["n_sites"])) for x in t]
        rep.need(f"{k} coords", coords == [w[:3] for w in want])
        if coords == [w[:3] for w in want]:
            ws = np.array([w[3] for w in want])
            rep.add(f"{k} post_sum", _ratio(np.abs(t["post_sum"] - ws), 1e-12 * np.abs(ws) + 1e-300))
        rep.need(f"{k} post_mean", np.array_equal(t["post_mean"], t["post_sum"] / t["n_sites"]))


def rule_summary(rep, name, got, ref, ctx):
    """tests/test_gpu_summary.py: integers equal, doubles within 2 n 2^-53 relative of
    summary_util.summarize on the handle's own path / posteriors."""
    marg, path = got["marg_prob"], got["path"]
    first = True
    for tag, reg in ctx.regions.items():
        for key, thr, vit, with_sites in ((f"{name}.{tag}", 0.5, True, first),
                                          (f"{name}.posterior.{tag}", 0.9, False, False)):
            want_reg, want_sites, n_mb = summary_util.summarize(path, marg, ctx.pos, reg, thr, vit, True)
            r = got[f"{key}.0"]
            rep.need(f"{key} shape", r.shape == want_reg.shape)
            for f in ("vit_sites", "post_sites"):
                rep.need(f"{key} {f}", np.array_equal(r[f], want_reg[f]))
            n = np.broadcast_to(np.diff(np.asarray(reg), axis=1).T, r.shape)
            rep.add(f"{key} post_sum", _ratio(np.abs(r["post_sum"] - want_reg["post_sum"]),
                                              2.0 * n * U * np.abs(want_reg["post_sum"])))
            rep.add(f"{key} vit_mb", _ratio(np.abs(r["vit_mb"] - want_reg["vit_mb"]),
                                            2.0 * n_mb * U * np.abs(want_reg["vit_mb"])))
            rep.need(f"{key} sites", (f"{key}.1" in got) == with_sites)
            if with_sites:
                s = got[f"{key}.1"]
                for f in ("vit_count", "post_count"):
                    rep.need(f"{key} site {f}", np.array_equal(s[f], want_sites[f]))
                rep.add(f"{key} site post_sum", _ratio(np.abs(s["post_sum"] - want_sites["post_sum"]),
                                                       2.0 * ctx.I * U * np.abs(want_sites["post_sum"])))
        first = False


def rule_sharing(rep, name, got, ref, ctx):
    """tests/test_gpu_sharing.py: counts equal, post_prod within 2 (n + 1) 2^-53 relative of
    sharing_util.sharing on the handle's own path / posteriors, and symmetric."""
    marg, path = got["marg_prob"], got["path"]
    for key, thr, (a, b) in ((name, 0.5, (0, ctx.S)), (f"{name}.range", 0.7, ru.sharing_range(ctx.S))):
        vit, both, prod = sharing_util.sharing(path, marg, thr, a, b)
        rep.need(f"{key} vit_both", np.array_equal(got[f"{key}.vit_both"], vit))
        rep.need(f"{key} post_both", np.array_equal(got[f"{key}.post_both"], both))
        p = got[f"{key}.post_prod"]
        rep.add(f"{key} post_prod", _ratio(np.abs(p - prod), 2.0 * (b - a + 1) * U * np.abs(prod)))
        rep.need(f"{key} symmetric", np.array_equal(p, p.T))


def rule_support(rep, name, got, ref, ctx):
    """tests/test_gpu_support.py's _check, against the other handle: the two logarithms within
    2 LOG_TOL (-inf in the same places), post_min within 2 POST_TOL, its site the same but for a
    runner-up within the tolerance, lod made of the record's own logarithms."""
    for key in (name, f"{name}.hand"):
        if key not in got:
            continue
        g, r = got[key], ref[key]
        rep.need(f"{key} shape", g.shape == r.shape)
        for f in ("log_p_ibd", "log_p_non"):
            inf = np.isneginf(r[f])
            rep.need(f"{key} {f} nan", not np.isnan(g[f]).any())
            rep.need(f"{key} {f} -inf", np.array_equal(np.isneginf(g[f]), inf))
            rep.add(f"{key} {f}", _ratio(np.abs(g[f][~inf] - r[f][~inf]), 2 * ctx.scale * sup.LOG_TOL))
        rep.add(f"{key} post_min", _ratio(np.abs(g["post_min"] - r["post_min"]), 2 * ctx.scale * sup.POST_TOL))
        moved = int((g["post_min_site"] != r["post_min_site"]).sum())
        rep.need(f"{key} post_min_site", moved < MIN_SITE_DIFFER * len(g) or moved == 0, f"{moved} of {len(g)}")
        with np.errstate(invalid="ignore"):
            lod = (g["log_p_ibd"] - g["log_p_non"]) / math.log(10.0)
        rep.need(f"{key} lod", np.array_equal(g["lod"], lod, equal_nan=True))


def bracket_levels(scale=1, levels=bounds_util.LEVELS):
    """Every level p as the pair (p e^+t, p e^-t), t = 2 scale TIE, in descending order: the
    answers of the other handle at these bracket every answer at p that differs from it by a level
    crossed within rounding (tests/test_gpu_bounds.py brackets with the yardstick's curves at
    p e^+-TIE; between two handles, each within TIE of them, twice that)."""
    t = 2 * scale * bounds_util.TIE
    return tuple(x for p in levels for x in (p * math.exp(t), p * math.exp(-t)))


def bounds_probe(href, got, ranges, scale=1):
    """{key: (records, the reference handle at the ANCHORS OF `got`, the same at bracket_levels)}
    for the battery's two tract_bounds calls -- as tests/test_gpu_bounds.py evaluates its yardstick
    at the device's resolved anchors."""
    out = {}
    for key, rec in (("tract_bounds", got["ibd_tracts.viterbi"]), ("tract_bounds.hand", ranges)):
        if f"{key}.0" in got and rec is not None:
            anc = got[f"{key}.0"]["anchor"].astype(np.uint64)
            out[key] = (href.tract_bounds(rec, anc), href.tract_bounds(rec, anc, bracket_levels(scale)))
    return out


def rule_bounds(rep, name, got, ref, ctx):
    """tests/test_gpu_bounds.py's _check with the other handle in the yardstick's place.
    Anchors: post_anchor within 2 POST_TOL of the other handle's at ITS anchor, whichever site
    either chose, and at most 2 % of the anchors differ (a runner-up within the tolerance).
    Everything else against the other handle asked at this handle's anchors (ctx.bounds): the
    anchors as given, the limits equal, post_anchor within 2 POST_TOL, the reach logarithms within
    2 TIE with -inf in the same places; every quantile site between the other handle's answers at
    p e^+-2 TIE (a level crossed within rounding, and nothing else); a record without posterior
    mass at its anchor answers the anchor; the answer is the limit exactly when the handle's own
    reach is at least the level; fewer than 1 % of the sites differ at all; the answers monotone in
    the level and inside the limits."""
    levels = bounds_util.LEVELS
    tie = ctx.scale * bounds_util.TIE
    for key in (name, f"{name}.hand"):
        if f"{key}.0" not in got:
            continue
        (bd, start, end), (rbd, rstart, rend) = ([d[f"{key}.{j}"] for j in range(3)] for d in (got, ref))
        rep.need(f"{key} shape", bd.shape == rbd.shape and start.shape == rstart.shape == (len(bd), len(levels)))
        n = len(bd)
        same = bd["anchor"] == rbd["anchor"]
        rep.add(f"{key} anchors", (n - int(same.sum())) / max(ANCHORS_DIFFER * n, 1e-300) if n else 0.0)
        rep.add(f"{key} post_anchor own", _ratio(np.abs(bd["post_anchor"] - rbd["post_anchor"]),
                                                 2 * ctx.scale * sup.POST_TOL))
        rep.need(f"{key} probe", key in ctx.bounds, "the other handle was not asked at this handle's anchors")
        if key not in ctx.bounds:
            continue
        (abd, astart, aend), (_, bstart, bend) = ctx.bounds[key]
        rep.need(f"{key} anchor as given", np.array_equal(abd["anchor"], bd["anchor"]))
        for f in ("left_limit", "right_limit"):
            rep.need(f"{key} {f}", np.array_equal(bd[f], abd[f]))
        rep.add(f"{key} post_anchor", _ratio(np.abs(bd["post_anchor"] - abd["post_anchor"]),
                                             2 * ctx.scale * sup.POST_TOL))
        for f in ("log_reach_left", "log_reach_right"):
            rep.need(f"{key} {f} nan", not np.isnan(bd[f]).any())
            inf = np.isneginf(abd[f])
            rep.need(f"{key} {f} -inf", np.array_equal(np.isneginf(bd[f]), inf))
            ok = ~inf & ~np.isneginf(bd[f])
            rep.add(f"{key} {f}", _ratio(np.abs(bd[f][ok] - abd[f][ok]), 2 * tie))
            rep.need(f"{key} reach{f[9:]}", np.array_equal(bd["reach" + f[9:]], np.exp(bd[f])))
        s, e = start.astype(np.int64), end.astype(np.int64)
        c = bd["anchor"].astype(np.int64)[:, None]
        lo, hi = bd["left_limit"].astype(np.int64)[:, None], bd["right_limit"].astype(np.int64)[:, None]
        dead = ~(abd["post_anchor"] > 0)
        rep.need(f"{key} dead", bool((s[dead] == c[dead]).all() and (e[dead] == c[dead]).all()))
        live = ~dead
        bs, be = bstart.astype(np.int64), bend.astype(np.int64)
        # (columns 2 j, 2 j + 1 of the probe: level j times e^+t, e^-t; a higher level starts later
        # and ends sooner)
        rep.need(f"{key} start bracket", bool(((bs[live, 1::2] <= s[live]) & (s[live] <= bs[live, 0::2])).all()),
                 "a start outside the other handle's answers at p e^-+2 TIE")
        rep.need(f"{key} end bracket", bool(((be[live, 0::2] <= e[live]) & (e[live] <= be[live, 1::2])).all()),
                 "an end outside the other handle's answers at p e^+-2 TIE")
        lp = np.log(np.asarray(levels))[None, :]
        for side, x, lim, f in (("left", s, lo, "log_reach_left"), ("right", e, hi, "log_reach_right")):
            lr = bd[f][:, None]
            with np.errstate(invalid="ignore"):
                clear = live[:, None] & (lim != c) & (np.abs(lr - lp) > tie)
            rep.need(f"{key} censoring {side}", bool(((x == lim) == (lr >= lp))[clear].all()),
                     "the answer is the limit exactly when the reach is at least the level")
        differ = int((s != astart.astype(np.int64)).sum() + (e != aend.astype(np.int64)).sum())
        rep.add(f"{key} sites", differ / (SITES_DIFFER * 2 * start.size) if start.size else 0.0,
                f"{differ} of {2 * start.size}")
        rep.need(f"{key} order", bool((np.diff(s, axis=1) <= 0).all() and (np.diff(e, axis=1) >= 0).all()
                                      and (lo <= s).all() and (s <= c).all() and (c <= e).all()
                                      and (e <= hi).all()))


def rule_info(rep, name, got, ref, ctx):
    """tests/test_gpu_info.py's three bounds (info_util.bounds: lkl 1e-12 |l|, gradient 1e-9 (|g| +
    |h_kk| x_k), Hessian 1e-9 max(|h_kl|, sqrt|h_kk h_ll|)), twice, at the point of each record."""
    for key, (F, A) in ((name, (ctx.F, ctx.A)), (f"{name}.at", ru.info_points(ctx.I))):
        g, r = got[key], ref[key]
        b = info_util.bounds(r, F, A)
        for f in info_util.FIELDS:
            rep.need(f"{key} {f} finite", np.isfinite(g[f]).all())
            rep.add(f"{key} {f}", _ratio(np.abs(g[f] - r[f]), 2 * ctx.scale * b[f]))


def rule_expect(rep, name, got, ref, ctx):
    for k in _keys(got, name):
        tol = xu.REGION_TOL if k.endswith(".0") else xu.SITE_TOL
        _fields(rep, k, got[k], ref[k], tol, ctx.scale, minus_inf=True)


def _by_unit(table):
    def rule(rep, name, got, ref, ctx):
        for k in _keys(got, name):
            unit = k.split(".")[1]
            _fields(rep, k, got[k], ref[k], table[unit], ctx.scale)
    return rule


def _array(rep, key, got, ref, tol, scale=1):
    """A plain array within scale x 2 x tol of the reference handle's."""
    rep.need(f"{key} shape", got.shape == ref.shape and got.dtype == ref.dtype)
    rep.need(f"{key} finite", bool(np.isfinite(got).all()))
    if got.shape == ref.shape:
        rep.add(key, _ratio(np.abs(got - ref), 2 * scale * tol))


def rule_long(rep, name, got, ref, ctx):
    """tests/test_gpu_long.py: the region records by long_util.TOL per unit and field; post and the
    site records' sum by its "post" and "sum" (twice over, times ctx.scale, as every tolerance
    rule); count restated as (post >= 0.5).sum of the handle's OWN post, which the battery asks for
    wherever it asks for the site records."""
    for k in _keys(got, name):
        unit, part = k.split(".")[1], k.split(".")[-1]
        tol = long_util.TOL[unit]
        if part == "regions":
            _fields(rep, k, got[k], ref[k], tol, ctx.scale)
        elif part == "post":
            _array(rep, k, got[k], ref[k], tol["post"], ctx.scale)
        else:
            rep.need(f"{k} part", part == "sites", "an output that ibd_long does not have")
            _array(rep, f"{k} sum", got[k]["sum"], ref[k]["sum"], tol["sum"], ctx.scale)
            own = k[:-len("sites")] + "post"
            rep.need(f"{k} post", own in got, "site records without the handle's own post")
            if own in got:
                rep.need(f"{k} count", np.array_equal(got[k]["count"], (got[own] >= 0.5).sum(axis=1).T),
                         "not (post >= 0.5).sum of the handle's own post")


# battery key (its first component) -> rule
RULES = collections.OrderedDict([
    ("indF", rule_bytes), ("alpha", rule_bytes), ("freq", rule_bytes), ("gl", rule_bytes),
    ("path", rule_bytes), ("geno_posteriors", rule_bytes),
    ("freq_info", rule_bytes), ("geno_smooth", rule_bytes), ("ibd_longest", rule_bytes),
    ("sample_paths", rule_draws),
    ("format_posteriors", rule_format), ("ibd_tracts", rule_tracts), ("ibd_summary", rule_summary),
    ("ibd_sharing", rule_sharing),
    ("ind_lkl", rule_lkl), ("lkl", rule_lkl), ("marg_prob", rule_marg), ("e_prob", rule_eprob),
    ("mstep_freq", rule_mstep_freq),
    ("tract_support", rule_support), ("tract_bounds", rule_bounds), ("obs_info", rule_info),
    ("ibd_expect", rule_expect), ("ibd_moments", _by_unit(moments_util.COHORT_TOL)),
    ("ibd_by_length", _by_unit(bylength_util.TOL)), ("ibd_long", rule_long),
])

# every tolerance the rules import or state, for tests/test_layouts_cpu.py
TOLERANCES = {
    "LKL_RTOL": LKL_RTOL, "POST_ATOL": POST_ATOL, "FREQ_RTOL": FREQ_RTOL, "EPROB_ATOL": EPROB_ATOL,
    "DRAW_MB_RTOL": DRAW_MB_RTOL, "LOG_TOL": sup.LOG_TOL, "POST_TOL": sup.POST_TOL, "TIE": bounds_util.TIE,
    **{f"REGION_TOL.{k}": v for k, v in xu.REGION_TOL.items()},
    **{f"SITE_TOL.{k}": v for k, v in xu.SITE_TOL.items()},
    **{f"COHORT_TOL.{u}.{k}": v for u, d in moments_util.COHORT_TOL.items() for k, v in d.items()},
    **{f"bylength.TOL.{u}.{k}": v for u, d in bylength_util.TOL.items() for k, v in d.items()},
    **{f"long.TOL.{u}.{k}": v for u, d in long_util.TOL.items() for k, v in d.items()},
}


def rule_of(key, rules=None):
    """The names of the rules that own a battery key: exactly one, or RULES is wrong.
    rules: another table in RULES' place (tests/chain_util.CHAIN_RULES)."""
    return [name for name in (RULES if rules is None else rules) if key == name or key.startswith(name + ".")]


def compare(got, ref, ctx, rules=None):
    """Both batteries (array form) by RULES, or by the table given.  Returns the Report; the caller
    prints and asserts."""
    rules = RULES if rules is None else rules
    rep = Report()
    rep.need("keys", list(got) == list(ref), "the two batteries have other keys")
    for k in got:
        rep.need(f"{k} rule", len(rule_of(k, rules)) == 1, "no rule, or two")
    for name, rule in rules.items():
        if _keys(got, name):
            rule(rep, name, got, ref, ctx)
    return rep


def show(tag, h, rep):
    C, T, used, empty = describe(h)
    print(f"\n  {tag}: layout (C, T) = ({C}, {T}), {used} of {64 * C} lanes used, {empty} empty waves, "
          f"S % T = {h.n_sites % T}")
    worst = rep.worst_per_key()
    group = collections.OrderedDict()
    for k, r in worst.items():
        name = rule_of(k)[0] if rule_of(k) else k
        group[name] = max(group.get(name, 0.0), r)
    print("  worst error / tolerance: " + ", ".join(f"{k} {r:.3g}" for k, r in group.items()))


def check(tag, h, rep):
    show(tag, h, rep)
    assert not rep.failed, f"{tag}: " + "; ".join(f"{l}: {r:.3g} {n}" for l, r, n in rep.failed[:12])
