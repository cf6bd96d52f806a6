"""The cut of a chain as the third axis of the battery tests (tests/test_gpu_chain_outputs.py): the
battery of tests/replica_util.py on a pkg.Chain of site shards -- every call that has an
nghmm_chain_* twin, under the same keys -- held to the same battery on ONE handle of the same data
by CHAIN_RULES, which is tests/layout_util.RULES ("site shards are a fast-mode layout",
tests/test_gpu_siteshard.py) with the overrides named below.  No tolerance here is new and none
comes from a device: each override cites the header text or the existing test it rests on.

Same parameters on both sides (prepare): a chain has no estep(), so both sides run ONE EM step with
indF and alpha fixed from the same start, the chain's frequencies are then set on every member AND
on the single handle, and the emissions are made again.  Every walk-shaped output (it reads the
parameters and the emissions) then runs at identical parameter bytes; the outputs that read the
posteriors are restated from each side's own read-backs, as layout_util.RULES does.

geometries() names the cuts; cut_regions() and cut_ranges() place regions and hand-made ranges on
them; reach() / admitted() restate in Python which thresholds nghmm_chain_ibd_by_length and
nghmm_chain_ibd_long refuse.  tests/test_chain_battery_cpu.py checks all of that without a device
and keeps CHAIN_RULES total over the chain battery's keys."""
import collections

import numpy as np

import bylength_util as bu
import genosmooth_util
import layout_util as lu
import long_util
import replica_util as ru
import support_util as sup

# what replica_util.battery leaves out on a Chain: hmm.Chain has no such call
NO_TWIN = ("e_prob", "gl", "geno_posteriors", "format_posteriors", "lkl")

# tests/test_gpu_siteshard.py::test_chain_shapes, after EM steps with indF and alpha fixed: the
# project's own figures for a chain against one handle
IND_LKL_RTOL = 1e-12
FREQ_RTOL, FREQ_ATOL = 1e-10, 1e-13
MARG_ATOL = 1e-9

# the individuals of cut_ranges: support_util.hand_ranges uses 0 to 5, layout_util.tail_ranges 6 to 9
RANGE_INDS = (10, 11, 12, 13)
CUT_WINDOW = (1100, 1400)
STRETCH = (40, 120)          # the cut site k has a confident tract over k - 40 .. k + 120


# ---------------------------------------------------------------------------------------------
# geometries

def cut_site(post, lo=CUT_WINDOW[0], hi=CUT_WINDOW[1]):
    """The cut site k, from the numpy posterior [I][S] (long_util.post_b at L = 1 site): the middle
    one of the sites in lo .. hi at which one of the individuals 0 to 4 (alpha = 1e-3) is >= 0.9
    over k - 40 .. k + 120."""
    ks = [k for k in range(lo, hi) if (post[:5, k - STRETCH[0]:k + STRETCH[1] + 1] >= 0.9).all(axis=1).any()]
    assert ks, "no site inside a confident tract of an alpha = 1e-3 individual"
    return ks[len(ks) // 2]


def ragged(n_sites, world):
    """distributed.site_ranges_ragged's cuts (where the host cuts for --n_gpus), restated: multiples
    of 16 sites except the last.  tests/test_chain_battery_cpu.py holds it to the package's."""
    cuts = [0]
    for r in range(1, world):
        cuts.append(max((n_sites * r // world) // 16 * 16, cuts[-1] + 1))
    return cuts + [n_sites]


def geometries(n_sites, k, starts):
    """{name: cuts}.  A: one-site shards first, last and inside a tract.  B: a 79-site shard inside
    a tract and inside chromosome 1 (L = 80 sites reaches exactly 79 sites into it from both
    sides).  C: the last site of chromosome 1 and the first of chromosome 2 stand alone, with cuts
    on two starts.  D: eight shards where the host cuts.  G: two shards where the host cuts, long
    enough for layouts of more than one wave per individual (fast_create keeps 16 sites per lane,
    so a shard below 2048 sites has one wave whatever NGHMM_FAST_C says)."""
    S = n_sites
    return collections.OrderedDict([
        ("A", [0, 1, k, k + 1, S - 1, S]),
        ("B", [0, k, k + 79, S]),
        ("C", [0, starts[0] - 1, starts[0], starts[0] + 1, starts[1], S]),
        ("D", ragged(S, 8)),
        ("G", ragged(S, 2))])


# NGHMM_FAST_C of the members in turn (None: the layout's own)
FAST_C = {"D": (1, 4), "G": (1, 2)}


def shards(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


def _one(sites):
    s = np.unique(np.asarray(sites, dtype=np.int64))
    return np.stack([s, s + 1], axis=1)


def cut_regions(cuts):
    """Region sets on the cuts of a chain, each sorted and disjoint:
    cut1    one-site regions on both sides of every cut (a one-site shard is one of them);
    shards  every shard as a region of its own: each begins at a cut and ends at one;
    span    [cuts[1] - 1, cuts[2] + 1): the last site of shard 0, all of shard 1 and the first site
            of shard 2 -- and the same around the last shard but two, where that is disjoint (two
            shards: the two sites at the cut)."""
    cuts = [int(c) for c in cuts]
    inner = cuts[1:-1]
    assert inner
    span = [(max(cuts[1] - 1, 0), min(cuts[2], cuts[-1] - 1) + 1)] if len(inner) > 1 else [(cuts[1] - 1, cuts[1] + 1)]
    if len(cuts) >= 5 and cuts[-3] - 1 >= span[0][1]:
        span.append((cuts[-3] - 1, min(cuts[-2] + 1, cuts[-1])))
    return collections.OrderedDict([
        ("cut1", _one([c - 1 for c in inner] + inner)),
        ("shards", np.array(shards(cuts), dtype=np.int64)),
        ("span", np.array(span, dtype=np.int64))])


def cut_ranges(cuts):
    """Hand-made ranges [(ind, first, last)] on the cuts, for tract_support / tract_bounds, on
    RANGE_INDS: individual 10 -- ranges that end on a shard's last site; 11 -- ranges that begin on
    a shard's first site (on a one-site shard both are one-site ranges); 12 -- a range across
    three shards (two: the two sites at the cut); 13 -- the whole data less its two end sites.
    Disjoint within an individual."""
    cuts = [int(c) for c in cuts]
    S, inner = cuts[-1], cuts[1:-1]
    i_end, i_begin, i_three, i_all = RANGE_INDS
    out, last = [], -1
    for c in inner:
        a = max(c - 5, last + 1)
        if a <= c - 1:
            out.append((i_end, a, c - 1))
            last = c - 1
    for c, nxt in zip(inner, inner[1:] + [S]):
        out.append((i_begin, c, min(c + 4, nxt - 1)))
    out.append((i_three, max(cuts[1] - 1, 0), cuts[2] if len(inner) > 1 else cuts[1]))
    out.append((i_all, 1, S - 2))
    return sorted(set(out))


# ---------------------------------------------------------------------------------------------
# which thresholds a chain refuses

def reach(pos, cuts, min_len, unit):
    """(far [n], back [n]) of one threshold, from include/nghmm.h's text for
    nghmm_chain_ibd_by_length / nghmm_chain_ibd_long and the two loops of csrc/capi_bylength.hip and
    csrc/capi_long.hip that fill Shard::H and Shard::HL.  For the shard [lo, hi): far is the
    largest b(a) - hi + 1 over its sites a, b(a) the last site of the shortest window that begins
    at a, has length >= L and lies within a's chromosome (bylength_util.window_ends: from the
    definition); back is the largest lo - l(s) over its sites s, l(s) the first site of the
    shortest such window that ENDS at s (long_util.window_starts).  0 where no window leaves the
    shard."""
    b = bu.window_ends(pos, [min_len], unit)[0]
    l = long_util.window_starts(pos, [min_len], unit)[0]
    far, back = [], []
    for lo, hi in shards(cuts):
        e = b[lo:hi][b[lo:hi] >= 0]
        far.append(max(int(e.max()) - hi + 1, 0) if len(e) else 0)
        s = l[lo:hi][l[lo:hi] >= 0]
        back.append(max(lo - int(s.min()), 0) if len(s) else 0)
    return far, back


def admitted(pos, cuts, min_len, unit, entry):
    """Whether the chain takes the threshold: nghmm_chain_ibd_by_length refuses it when a shard's
    far exceeds the size of the shard behind it; nghmm_chain_ibd_long by the same rule, and by the
    mirrored one (back against the shard in front)."""
    assert entry in ("ibd_by_length", "ibd_long")
    far, back = reach(pos, cuts, min_len, unit)
    size = [hi - lo for lo, hi in shards(cuts)]
    n = len(size)
    ok = all(far[r] <= size[r + 1] for r in range(n - 1) if far[r])
    if entry == "ibd_long":
        ok = ok and all(back[r] <= size[r - 1] for r in range(1, n) if back[r])
    return ok


def crosses(pos, cuts, min_len, unit):
    """Whether a window of the threshold crosses a cut at all."""
    far, back = reach(pos, cuts, min_len, unit)
    return any(far) or any(back)


def admitted_lengths(pos, cuts, table=bu.COHORT_LEN):
    """replica_util.battery's `lengths`: per entry point and unit the thresholds of the table that
    the chain takes, in order."""
    return {e: {u: tuple(l for l in L if admitted(pos, cuts, l, u, e)) for u, L in table.items()}
            for e in ("ibd_by_length", "ibd_long")}


# ---------------------------------------------------------------------------------------------
# handles

def member(pkg, cohort, lo, hi, packed=False, fast_c=None, mode_name="fast"):
    """A handle of the sites [lo, hi) of the cohort (support_util.gpu_cohort's tuple), loaded."""
    d, gl = cohort[0], cohort[1]
    with lu.forced_layout(fast_c):
        h = pkg.NgsFHMM(d.n_ind, hi - lo, mode=ru.mode_of(pkg, mode_name, packed))
    pos = np.ascontiguousarray(d.pos_dist_mb[lo:hi])
    if packed:
        h.load_raw(np.ascontiguousarray(d.gl[lo:hi]), pos, space=0, call_geno=True)
    else:
        h.load(np.ascontiguousarray(gl[lo:hi]), pos)
    return h


def members(pkg, cohort, cuts, packed=False, fast_c=None, mode_name="fast"):
    """One member per shard; fast_c: NGHMM_FAST_C of the members in turn."""
    hs = []
    try:
        for r, (lo, hi) in enumerate(shards(cuts)):
            hs.append(member(pkg, cohort, lo, hi, packed, fast_c[r % len(fast_c)] if fast_c else None, mode_name))
    except BaseException:
        close(hs)
        raise
    return hs


def close(hs):
    for h in hs:
        h.close()


def set_point(hs, cuts, F, A, freq):
    """(F, A, freq) on every member -- its own slice of a frequency vector -- and the emissions."""
    f = np.asarray(freq, dtype=np.float64)
    for h, (lo, hi) in zip(hs, shards(cuts)):
        h.set_params(F, A, f[lo:hi] if f.ndim else float(f))
        h.init_emission()


def prepare(ch, cuts, whole, start):
    """The order of the module's docstring on a chain and on the single handle.  Returns
    (the frequencies both now hold, em_step of the chain, em_step of the single handle) for
    replica_util.battery."""
    F, A, freq = start
    S = cuts[-1]
    set_point(ch.handles, cuts, F, A, freq)
    set_point([whole], [0, S], F, A, freq)
    whole.iter_EM(1, True, True)
    ch.iter_EM(1, True, True)
    em_w = {"freq": whole.freq, "ind_lkl": np.array(whole.ind_lkl, copy=True)}
    em_c = {"freq": ch.freq, "ind_lkl": np.array(ch.ind_lkl, copy=True)}
    f = em_c["freq"]
    set_point(ch.handles, cuts, F, A, f)
    set_point([whole], [0, S], F, A, f)
    return f, em_c, em_w


def restrict(battery, keys):
    """The single handle's battery at the keys of the chain's, in the chain's order."""
    return type(battery)((k, battery[k]) for k in keys if k in battery)


def other_order(pkg, ch, regions, ranges, lengths):
    """ibd_long -> tract_bounds -> sample_paths -> ibd_expect on a chain whose decode is done, as
    bytes under the battery's keys: the battery asks them in another order, between other calls
    that share the Carver's scratch."""
    out = collections.OrderedDict()
    tag, reg = next(iter(regions.items()))
    for u in bu.COHORT_LEN:
        ru._records(out, f"ibd_long.{u}.{tag}",
                    ch.ibd_long(lengths["ibd_long"][u], unit=u, regions=reg, sites=True, post=True))
    ru._records(out, "tract_bounds.hand", ch.tract_bounds(ranges))
    ru._records(out, "sample_paths", ch.sample_paths(3, seed=5, keep=2))
    ru._records(out, f"ibd_expect.{tag}", ch.ibd_expect(reg, sites=True, viterbi=True))
    return out


# ---------------------------------------------------------------------------------------------
# the rules

class Context(lu.Context):
    """layout_util.Context and the cuts of the chain."""

    def __init__(self, cuts, *args, **kw):
        super().__init__(*args, **kw)
        self.cuts = [int(c) for c in cuts]

    def crossing(self, regions):
        """[R] bool: the regions with a cut strictly inside."""
        reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
        inner = np.asarray(self.cuts[1:-1], dtype=np.int64)
        return ((reg[:, :1] < inner[None, :]) & (inner[None, :] < reg[:, 1:])).any(axis=1)


def rule_chain_geno_smooth(rep, name, got, ref, ctx):
    """include/nghmm.h, nghmm_chain_geno_smooth: "post, call and sites are ... THE SINGLE HANDLE'S
    BYTES"; "a region that crosses a cut is one region, its shards' parts added on the host in rank
    order: within rounding of the single handle's sums, not their bytes".  A region inside one shard
    is not promised more, and is not the single handle's bytes either: a handle adds a region piece
    by piece on a grid of kSummarySeg sites that begins at ITS first site
    (csrc/kernels_genosmooth.hip), so a member groups the same sites otherwise.  So: bytes, but for
    the region records, which tests/test_gpu_genosmooth.py::test_chains holds -- all of them, across
    a cut or not -- to genosmooth_util.TOL x the sum of the absolute values of the record's terms.
    Every term of the four fields is a probability or w0 2 f (1 - f): none is negative, so that
    sum is the record itself (the single handle's).  The report names the records across a cut
    apart from the others."""
    for k in lu._keys(got, name):
        if not k.endswith(".regions"):
            lu.rule_bytes(rep, k, got, ref, ctx)
            continue
        g, r = got[k], ref[k]
        rep.need(f"{k} shape", g.shape == r.shape and g.dtype == r.dtype)
        cross = ctx.crossing(ctx.regions[k.split(".")[1]])
        for f in genosmooth_util.REGION_FIELDS:
            tol = genosmooth_util.TOL[genosmooth_util._key(f)]
            rep.need(f"{k} {f} finite", bool(np.isfinite(g[f]).all()))
            for which, sel in (("across a cut", cross), ("inside a shard", ~cross)):
                rep.add(f"{k} {f} {which}", lu._ratio(np.abs(g[f] - r[f])[:, sel], tol * np.abs(r[f])[:, sel]))


def rule_chain_ind_lkl(rep, name, got, ref, ctx):
    """tests/test_gpu_siteshard.py::test_chain_shapes: rtol 1e-12."""
    rep.add(name, lu._ratio(np.abs(got[name] - ref[name]), IND_LKL_RTOL * np.abs(ref[name])))


def rule_chain_freq(rep, name, got, ref, ctx):
    """tests/test_gpu_siteshard.py::test_chain_shapes: rtol 1e-10 with atol 1e-13."""
    rep.need(f"{name} finite", bool(np.isfinite(got[name]).all()))
    rep.add(name, lu._ratio(np.abs(got[name] - ref[name]), FREQ_RTOL * np.abs(ref[name]) + FREQ_ATOL))


def rule_chain_marg(rep, name, got, ref, ctx):
    """tests/test_gpu_siteshard.py::test_chain_shapes: atol 1e-9."""
    rep.need(f"{name} shape", got[name].shape == ref[name].shape)
    rep.add(name, lu._ratio(np.abs(got[name] - ref[name]), MARG_ATOL))


def rule_chain_mstep_freq(rep, name, got, ref, ctx):
    """nghmm_chain_mstep_freq from the posteriors of the chain's own EM step: the frequencies by
    test_chain_shapes' figure for them (the chain battery has no e_prob)."""
    rule_chain_freq(rep, f"{name}.freq", got, ref, ctx)


# layout_util.RULES without the keys a chain does not have, and these overrides
OVERRIDES = collections.OrderedDict([
    ("geno_smooth", rule_chain_geno_smooth), ("ind_lkl", rule_chain_ind_lkl), ("freq", rule_chain_freq),
    ("marg_prob", rule_chain_marg), ("mstep_freq", rule_chain_mstep_freq)])
CHAIN_RULES = collections.OrderedDict((k, OVERRIDES.get(k, v)) for k, v in lu.RULES.items() if k not in NO_TWIN)

# which class every rule falls in for a chain (DESIGN.md's testing section has the same table)
RULE_CLASS = {
    "bytes": ("indF", "alpha", "path", "freq_info", "ibd_longest"),
    "bytes, region sums within tolerance": ("geno_smooth",),
    "restated": ("ibd_tracts", "ibd_summary", "ibd_sharing"),
    "tolerance": ("sample_paths", "tract_support", "tract_bounds", "obs_info", "ibd_expect", "ibd_moments",
                  "ibd_by_length", "ibd_long"),
    "em_step": ("ind_lkl", "freq", "marg_prob", "mstep_freq"),
}

TOLERANCES = {"IND_LKL_RTOL": IND_LKL_RTOL, "FREQ_RTOL": FREQ_RTOL, "FREQ_ATOL": FREQ_ATOL, "MARG_ATOL": MARG_ATOL,
              **{f"genosmooth.TOL.{k}": genosmooth_util.TOL[genosmooth_util._key(k)]
                 for k in genosmooth_util.REGION_FIELDS}}


def compare(got, ref, ctx):
    """The chain's battery against the single handle's (array form, restricted) by CHAIN_RULES."""
    return lu.compare(got, ref, ctx, CHAIN_RULES)


def batteries(pkg, ch, cuts, whole, cohort, regions, ranges, lengths):
    """prepare, then the same questions to the chain and to the single handle.  Returns (the
    report of CHAIN_RULES, the chain's battery, what set_point needs to put the chain back)."""
    d, _, F, A, freq = cohort
    rec = sup.to_records(ranges)
    f, em_c, em_w = prepare(ch, cuts, whole, (F, A, freq))
    got = ru.battery(pkg, ch, regions, arrays=True, ranges=rec, em_step=em_c, lengths=lengths)
    ref = restrict(ru.battery(pkg, whole, regions, arrays=True, ranges=rec, em_step=em_w, lengths=lengths), got)
    probe = lu.bounds_probe(whole, got, rec)
    ctx = Context(cuts, d.n_ind, d.n_sites, d.pos_dist_mb, regions, F, A, probe)
    return compare(got, ref, ctx), got, (F, A, f, em_c)


def show(tag, cuts, hs, rep):
    print(f"\n  {tag}: cuts {list(cuts)}, members (C, T) = {[tuple(h.layout()) for h in hs]}")
    group = collections.OrderedDict()
    for k, r in rep.worst_per_key().items():
        owner = lu.rule_of(k, CHAIN_RULES)
        name = owner[0] if owner else k
        group[name] = max(group.get(name, 0.0), r)
    print("  worst error / tolerance: " + ", ".join(f"{k} {r:.3g}" for k, r in group.items()))


def check(tag, cuts, hs, rep):
    show(tag, cuts, hs, rep)
    assert not rep.failed, f"{tag}: " + "; ".join(f"{l}: {r:.3g} {n}" for l, r, n in rep.failed[:12])
