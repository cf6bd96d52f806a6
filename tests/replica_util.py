"""The battery of the replica tests (tests/test_gpu_replica_outputs.py): one EM iteration, a decode and EVERY output entry point of include/nghmm.h on one handle, each
with arguments that reach its own scratch and code paths, as an ordered dict of name -> bytes.

nghmm_create_replica promises that every call on a replica behaves exactly as on an independent
handle loaded with the same data, so two batteries are compared with ==, key by key: there is no
tolerance (both modes are deterministic; post_prod's split plan is a function of
(I, site_begin, site_end) alone).  The layout tests (tests/test_gpu_layouts.py) ask for the same
battery as arrays and compare two handles of different lane layouts by tests/layout_util.RULES.
The chain tests (tests/test_gpu_chain_outputs.py) run it on a pkg.Chain of site shards -- every
call that has an nghmm_chain_* twin, under the same keys -- and compare with one handle by
tests/chain_util.CHAIN_RULES.

COVERED is the set of C entry points the battery reaches; tests/test_replica_battery_cpu.py holds it
against the public headers under include/, so that an entry point added without a replica test
fails there."""
import collections
import threading

import numpy as np

import bylength_util as bu
import expect_util as xu
import freqinfo_util as fu

COVERED = frozenset({
    "nghmm_iter_em", "nghmm_mstep_freq", "nghmm_viterbi",
    "nghmm_get_params", "nghmm_get_posteriors", "nghmm_get_emissions", "nghmm_get_gl",
    "nghmm_geno_posteriors", "nghmm_format_posteriors", "nghmm_lkl_batch",
    "nghmm_ibd_tracts", "nghmm_sample_paths", "nghmm_tract_support", "nghmm_tract_bounds",
    "nghmm_freq_info", "nghmm_geno_smooth", "nghmm_obs_info", "nghmm_ibd_summary",
    "nghmm_ibd_expect", "nghmm_ibd_moments", "nghmm_ibd_by_length", "nghmm_ibd_longest",
    "nghmm_ibd_long", "nghmm_ibd_sharing",
})

# the region sets of the battery (expect_util.region_sets): chromosome starts, gaps, a region across
# a chromosome start, one-site regions and both sides of every lane-chunk edge, without new shapes.
# Exact mode has no lane-chunks and every call walks each individual's sites serially there (a
# battery with one set takes a second on an MI355X, with four sets 1.8 s; fast mode 0.07 s with
# four): it gets "gaps" alone, which has the region across a chromosome start, the one-site regions
# and the gaps.
REGION_SETS = {"fast": ("whole", "chrom", "gaps", "edges"), "exact": ("gaps",)}
# a site range off the 64-site step of the sharing kernels
SHARING_RANGE = (37, 4001)

# the only key that is the data itself: equal whatever the start
DATA_KEYS = ("gl",)


def sharing_range(n_sites):
    """SHARING_RANGE, cut to data of fewer sites (an odd end still)."""
    return SHARING_RANGE[0], min(SHARING_RANGE[1], n_sites - 5)


def cohort_regions(pkg, cohort, mode_name, lane_sites):
    """{name: [R][2]} of the battery for support_util.gpu_cohort in mode "fast" or "exact";
    lane_sites: the sites per lane of the fast-mode layout (NgsFHMM.layout), which places the
    single-site regions of "edges"."""
    d = cohort[0]
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, lane_sites)
    return collections.OrderedDict((k, sets[k]) for k in REGION_SETS[mode_name])


def starts(n_ind, n_sites, n=3):
    """n clearly different starts (indF [I], alpha [I], freq [S]): disjoint bands of every
    parameter, so that no output of two of them can agree by accident."""
    bands = [((0.02, 0.25), (0.01, 0.4), (0.03, 0.2)),
             ((0.6, 0.95), (0.8, 2.0), (0.32, 0.48)),
             ((0.3, 0.55), (0.45, 0.75), (0.21, 0.3))]
    out = []
    for k in range(n):
        rng = np.random.default_rng(1000 + k)
        f, a, q = bands[k % len(bands)]
        out.append((rng.uniform(*f, n_ind), rng.uniform(*a, n_ind), rng.uniform(*q, n_sites)))
    return out


def load(pkg, h, cohort, packed):
    d, gl = cohort[0], cohort[1]
    if packed:
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=True)
    else:
        h.load(gl, d.pos_dist_mb)


def mode_of(pkg, mode_name, packed):
    return (pkg.MODE_FAST if mode_name == "fast" else pkg.MODE_EXACT) | (pkg.GENO_PACKED if packed else 0)


def reset(h, start):
    h.set_params(*start)
    h.init_emission()


class _Arrays(collections.OrderedDict):
    """A battery that keeps every record as a copy of the array itself (text stays bytes)."""


def _records(out, name, rec):
    """A structured array, or a tuple / dict of arrays some of which may be None, as bytes (into an
    _Arrays: as arrays)."""
    if isinstance(rec, dict):
        for k, v in rec.items():
            _records(out, f"{name}.{k}", v)
    elif isinstance(rec, tuple):
        for k, v in enumerate(rec):
            _records(out, f"{name}.{k}", v)
    elif rec is not None:
        if isinstance(rec, bytes):
            out[name] = rec
        elif isinstance(out, _Arrays):
            out[name] = np.array(rec, copy=True)
        else:
            out[name] = np.ascontiguousarray(rec).tobytes()


def lkl_points(n_ind):
    """(ind, F, alpha) of the battery's lkl call: 2 I points."""
    n = 2 * n_ind
    return np.arange(n) % n_ind, np.linspace(0.05, 0.9, n), np.geomspace(1e-3, 3.0, n)


def posterior_part(n_ind):
    """(first individual, number) of the battery's partial format_posteriors call."""
    return min(3, n_ind - 1), max(n_ind // 4, 1)


def info_points(n_ind):
    """(F, alpha) of the battery's obs_info call at given points."""
    return np.linspace(0.1, 0.8, n_ind), np.geomspace(0.01, 2.0, n_ind)


def members_agree(ch, which):
    """indF or alpha of a chain: member 0's, after checking that every member holds its bytes."""
    first = getattr(ch.handles[0], which)
    for r, m in enumerate(ch.handles[1:], 1):
        assert getattr(m, which).tobytes() == first.tobytes(), f"{which} of member {r} is not member 0's"
    return first


def battery(pkg, h, regions, arrays=False, estep_only=False, ranges=None, em_step=None, lengths=None):
    """On a handle that has parameters and emissions: iter_EM once, viterbi, then every output.
    regions: {name: [R][2]}; the per-cell outputs of geno_smooth and the site records are asked for
    with the first set only.  Returns an ordered dict of name -> bytes.
    arrays: name -> array instead (tests/layout_util.py compares within tolerances).
    estep_only: estep() in place of iter_EM() and no frequency step at the end, so that the
    parameters stay what the caller set (the L-BFGS-B M-step amplifies last-bit differences).
    ranges: hand-made records [n][3] for tract_support / tract_bounds besides the decode's tracts.
    em_step: {"freq", "ind_lkl"} of an EM step that the caller ran already (tests/chain_util.py's
    prepare, which sets the parameters again after it): no E-step here, these two keys are taken
    from it, and the frequency step at the end writes its frequencies alone.
    lengths: {"ibd_by_length" / "ibd_long": {unit: thresholds}} in place of bylength_util.COHORT_LEN
    (a chain refuses a threshold that reaches past a neighbouring shard).
    h may be a pkg.Chain (with em_step): every call that has a chain twin, under the same keys;
    Chain has no lkl, geno_posteriors, format_posteriors, gl or e_prob, and indF and alpha are
    member 0's (every member must hold the same bytes)."""
    out = _Arrays() if arrays else collections.OrderedDict()
    I, S = h.n_ind, h.n_sites
    chain = isinstance(h, pkg.Chain)
    assert em_step is not None or not chain, "a chain has no estep(): run chain_util.prepare first"
    lengths = {"ibd_by_length": bu.COHORT_LEN, "ibd_long": bu.COHORT_LEN} if lengths is None else lengths
    if em_step is not None:
        pass
    elif estep_only:
        h.estep()
    else:
        h.iter_EM()
    path = h.viterbi()
    _records(out, "indF", members_agree(h, "indF") if chain else h.indF)
    _records(out, "alpha", members_agree(h, "alpha") if chain else h.alpha)
    _records(out, "freq", h.freq if em_step is None else em_step["freq"])
    _records(out, "ind_lkl", h.ind_lkl if em_step is None else em_step["ind_lkl"])
    _records(out, "marg_prob", h.marg_prob)
    _records(out, "path", path)
    if not chain:
        _records(out, "e_prob", h.e_prob)
        _records(out, "gl", h.gl)
        _records(out, "geno_posteriors", h.geno_posteriors())
        _records(out, "geno_posteriors.chunk", h.geno_posteriors(S // 5 + 1, S // 7))
        _records(out, "format_posteriors", h.format_posteriors())
        _records(out, "format_posteriors.part", h.format_posteriors(*posterior_part(I)))
        _records(out, "lkl", h.lkl(*lkl_points(I)))

    tv = h.ibd_tracts("viterbi")
    _records(out, "ibd_tracts.viterbi", tv)
    _records(out, "ibd_tracts.posterior", h.ibd_tracts("posterior", 0.5, min_sites=3))
    _records(out, "sample_paths", h.sample_paths(3, seed=5, keep=2))
    _records(out, "tract_support", h.tract_support(tv))
    _records(out, "tract_bounds", h.tract_bounds(tv))
    if ranges is not None:
        _records(out, "tract_support.hand", h.tract_support(ranges))
        _records(out, "tract_bounds.hand", h.tract_bounds(ranges))
    _records(out, "freq_info", h.freq_info(fu.LEVELS, cavity=True))
    _records(out, "obs_info", h.obs_info())
    _records(out, "obs_info.at", h.obs_info(*info_points(I)))
    first = True
    for tag, reg in regions.items():
        _records(out, f"geno_smooth.{tag}", h.geno_smooth(reg, sites=first, post=first, call=first))
        _records(out, f"ibd_summary.{tag}", h.ibd_summary(reg, ("viterbi", "posterior"), 0.5, sites=first))
        _records(out, f"ibd_summary.posterior.{tag}", h.ibd_summary(reg, "posterior", 0.9, sites=False))
        _records(out, f"ibd_expect.{tag}", h.ibd_expect(reg, sites=first, viterbi=True))
        for u, L in bu.COHORT_LEN.items():
            _records(out, f"ibd_moments.{u}.{tag}", h.ibd_moments(reg, length=u))
            _records(out, f"ibd_by_length.{u}.{tag}", h.ibd_by_length(lengths["ibd_by_length"][u], unit=u, regions=reg))
            _records(out, f"ibd_longest.{u}.{tag}", h.ibd_longest(L, unit=u, regions=reg))
            _records(out, f"ibd_long.{u}.{tag}",
                     h.ibd_long(lengths["ibd_long"][u], unit=u, regions=reg, sites=first, post=first))
        first = False
    _records(out, "ibd_sharing", h.ibd_sharing(("viterbi", "posterior")))
    _records(out, "ibd_sharing.range", h.ibd_sharing(("viterbi", "posterior"), 0.7, *sharing_range(S)))
    if estep_only:
        return out
    # the frequency step on its own (it has a chain twin): from the posteriors of the iteration above
    h.mstep_freq(1)
    _records(out, "mstep_freq.freq", h.freq)
    if em_step is None:
        _records(out, "mstep_freq.e_prob", h.e_prob)
    return out


def probe(pkg, h):
    """What the handle's own state says, by calls that write none of it: parameters, posteriors,
    emissions, and outputs that read the frequencies, the decoded path and the posteriors.  A
    battery begins with iter_EM and viterbi, which rewrite all of that -- so state that a replica
    shared with its parent by mistake (its d_freq, say) is rewritten by each before it is read and
    the batteries alone cannot tell.  Two probes of one handle, taken before and after ANOTHER
    handle ran, can."""
    out = collections.OrderedDict()
    S = h.n_sites
    _records(out, "indF", h.indF)
    _records(out, "alpha", h.alpha)
    _records(out, "freq", h.freq)
    _records(out, "marg_prob", h.marg_prob)
    _records(out, "e_prob", h.e_prob)
    _records(out, "geno_posteriors.chunk", h.geno_posteriors(S // 5 + 1, S // 7))
    _records(out, "ibd_tracts.viterbi", h.ibd_tracts("viterbi"))
    _records(out, "freq_info", h.freq_info((0.5,)))
    _records(out, "obs_info", h.obs_info())
    _records(out, "ibd_sharing", h.ibd_sharing(("viterbi", "posterior")))
    return out


def run(pkg, h, start, regions, rounds=2):
    """reset to `start`, then `rounds` batteries one after the other: {"<round>:<name>": bytes}."""
    reset(h, start)
    out = collections.OrderedDict()
    for r in range(1, rounds + 1):
        for k, v in battery(pkg, h, regions).items():
            out[f"{r}:{k}"] = v
    return out


def independent(pkg, cohort, mode, packed, start, regions, rounds=2):
    """run() on a handle of its own, which is closed afterwards."""
    d = cohort[0]
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=mode) as h:
        load(pkg, h, cohort, packed)
        return run(pkg, h, start, regions, rounds)


def differing(a, b):
    """The keys at which two battery dicts differ (a missing key differs)."""
    return [k for k in list(a) + [k for k in b if k not in a] if a.get(k) != b.get(k)]


def in_threads(jobs):
    """Run the callables side by side, one host thread each; their results in order.  An
    exception of any is raised here."""
    got, err = [None] * len(jobs), []

    def work(k):
        try:
            got[k] = jobs[k]()
        except BaseException as e:          # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if err:
        raise err[0]
    return got


def is_data(key):
    return key.split(":", 1)[-1] in DATA_KEYS
