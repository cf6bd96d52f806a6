"""IBD per region and per site on the device (nghmm_ibd_summary / nghmm_chain_ibd_summary,
include/nghmm.h) against the numpy restatement of the definitions (tests/summary_util.py) applied
to the handle's own viterbi() and marg_prob.

Integers must be equal.  Doubles must be within 2 n 2^-53 relative, n the number of terms of that
sum: both sides add n non-negative terms, and either order is within (n - 1) 2^-53 of the exact
sum.  (n: the region's sites for a region's post_sum, the sites that continue an IBD run in it for
vit_mb, the individuals for a site's post_sum.)"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import cli_util
import summary_util
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# sites per lane of the pass: kSummarySeg of csrc/kernels_summary.hpp (tests/test_summary_cpu.py
# holds the two to each other)
SEG = importlib.import_module("ngsf-hmm_amd").SUMMARY_SEGMENT_SITES
U = 2.0 ** -53


def _within(got, want, n, what):
    """|got - want| <= 2 n u |want| element by element; prints the worst ratio to the bound."""
    got, want, n = np.asarray(got), np.asarray(want), np.asarray(n, dtype=np.float64)
    bound = 2.0 * n * U * np.abs(want)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), initial=0.0)
    print(f"{what}: worst error / bound = {worst:.3g}")
    assert (err <= bound).all(), (what, worst)


def _check(reg, sites, path, marg, dist, regions, thr=0.5, viterbi=True, posterior=True):
    want_reg, want_sites, n_mb = summary_util.summarize(path, marg, dist, regions if regions is not None else [],
                                                        thr, viterbi, posterior)
    I = path.shape[0]
    if regions is None or len(regions) == 0:
        assert reg is None
    else:
        assert reg.shape == want_reg.shape
        for f in ("vit_sites", "post_sites"):
            assert np.array_equal(reg[f], want_reg[f]), f
        n_sites = np.broadcast_to(np.diff(np.asarray(regions), axis=1).T, reg.shape)
        _within(reg["post_sum"], want_reg["post_sum"], n_sites, "region post_sum")
        _within(reg["vit_mb"], want_reg["vit_mb"], n_mb, "region vit_mb")
    if sites is not None:
        for f in ("vit_count", "post_count"):
            assert np.array_equal(sites[f], want_sites[f]), f
        _within(sites["post_sum"], want_sites["post_sum"], I, "site post_sum")
    return want_reg, want_sites


def _params(n):
    F = np.linspace(0.05, 0.95, n)
    A = np.full(n, 0.05)
    A[:min(5, n)] = 1e-3        # long IBD runs: across segments and region edges
    A[-min(5, n):] = 1e-3
    return F, A


def _decoded(pkg, n_ind, n_sites, mode, seed, packed=False, n_chrom=None):
    n_chrom = n_chrom or (2 if n_sites > 20 else 1)
    d = pkg.simulate.simulate(n_ind, n_sites, seed=seed, n_chrom=n_chrom, indF=0.7, alpha=0.05)
    h = pkg.NgsFHMM(n_ind, n_sites, mode=mode | (pkg.GENO_PACKED if packed else 0))
    if packed:
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=True)
    else:
        h.load(pkg.simulate.normalise_log_gl(d.gl), d.pos_dist_mb)
    F, A = _params(n_ind)
    h.set_params(F, A, 0.2)
    h.init_emission()
    h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
    return d, h


SITE_COUNTS = (7, 16, 17, SEG - 1, SEG, SEG + 1)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("n_ind", [1, 63, 64, 65, 130])
def test_lane_and_segment_shapes(pkg, n_ind, mode):
    """Individuals around the wave's 64 lanes, sites around the 16-site block and the segment."""
    for n_sites in SITE_COUNTS:
        d, h = _decoded(pkg, n_ind, n_sites, pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT,
                        seed=n_ind + n_sites)
        with h:
            path, marg = h.viterbi(), h.marg_prob
            regions = pkg.window_regions(d.pos_dist_mb, max(5, n_sites // 12))
            reg, sites = h.ibd_summary(regions)
            _check(reg, sites, path, marg, d.pos_dist_mb, regions)
            reg, sites = h.ibd_summary(np.array([[0, n_sites]]), threshold=0.9)
            _check(reg, sites, path, marg, d.pos_dist_mb, [[0, n_sites]], 0.9)
            assert sites["vit_count"].sum() == path.sum() and reg["vit_sites"].sum() == path.sum()


def test_packed_handle(pkg):
    d, h = _decoded(pkg, 65, SEG + 17, pkg.MODE_FAST, seed=3, packed=True)
    with h:
        path, marg = h.viterbi(), h.marg_prob
        regions = pkg.chromosome_regions(d.pos_dist_mb)
        reg, sites = h.ibd_summary(regions)
        _check(reg, sites, path, marg, d.pos_dist_mb, regions)
        assert path.any()


EDGE_I, EDGE_S = 40, 3 * SEG + 77


@pytest.fixture(scope="module")
def edge_cohort(pkg):
    d = pkg.simulate.simulate(EDGE_I, EDGE_S, seed=7, n_chrom=3, indF="r", alpha="r", missing_rate=0.02)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    cs = np.flatnonzero(np.isinf(d.pos_dist_mb))
    cs = cs[cs > 0]
    assert len(cs) == 2
    return d, gl, [int(c) for c in cs]


def _edge_handle(pkg, d, gl, mode, lo=0, hi=EDGE_S):
    h = pkg.NgsFHMM(EDGE_I, hi - lo, mode=mode)
    h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
    F, A = _params(EDGE_I)
    h.set_params(F, A, 0.2)
    h.init_emission()
    return h


def _edge_region_sets(c1, c2):
    S = EDGE_S
    return {
        # one site; two regions inside one segment; gaps; begin / end at a segment edge and one
        # next to it
        "edges": [(0, 1), (3, 40), (40, SEG), (SEG, SEG + 1), (SEG + 1, 2 * SEG - 1),
                  (2 * SEG + 1, 2 * SEG + 500), (2 * SEG + 600, S)],
        "everything": [(0, S)],
        "edge_pm1": [(SEG - 1, 2 * SEG + 1), (3 * SEG - 1, 3 * SEG), (3 * SEG, S - 1)],
        # across a chromosome start (c1, and c2 as the region's second site), the last site alone
        "chrom": [(7, SEG - 1), (c1 - 10, c1 + 10), (c2 - 1, c2 + 1), (S - 1, S)],
    }


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_region_edges(pkg, edge_cohort, mode):
    d, gl, (c1, c2) = edge_cohort
    dist = d.pos_dist_mb
    with _edge_handle(pkg, d, gl, pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) as h:
        h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
        path, marg = h.viterbi(), h.marg_prob
        sets = _edge_region_sets(c1, c2)
        # the two vit_mb exclusions are exercised: an IBD run goes on across a region's first
        # site, and one across a chromosome start inside a region
        run = (path[:, :-1] == 1) & (path[:, 1:] == 1)      # [:, s - 1]: sites s - 1 and s
        begins = [a for a, _ in sets["edges"] + sets["edge_pm1"] + sets["chrom"] if a > 0]
        assert any(run[:, a - 1].any() for a in begins)
        assert run[:, c1 - 1].any() or run[:, c2 - 1].any()     # (both lie inside a region of "chrom")
        for regions in sets.values():
            regions = np.array(regions)
            reg, sites = h.ibd_summary(regions)
            _check(reg, sites, path, marg, dist, regions)
        # n_regions == 0 with sites only; regions only with sites == NULL
        reg, sites = h.ibd_summary(None)
        assert reg is None
        _check(None, sites, path, marg, dist, None)
        reg, sites = h.ibd_summary(np.array(sets["edges"]), sites=False)
        assert sites is None
        _check(reg, None, path, marg, dist, sets["edges"])
        # windows: many regions, two or more per segment edge
        regions = pkg.window_regions(dist, 300)
        reg, sites = h.ibd_summary(regions, sites=False)
        _check(reg, None, path, marg, dist, regions)


def test_threshold_edge_and_single_sources(pkg, edge_cohort):
    d, gl, (c1, c2) = edge_cohort
    dist = d.pos_dist_mb
    with _edge_handle(pkg, d, gl, pkg.MODE_FAST) as h:
        h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
        path, marg = h.viterbi(), h.marg_prob
        regions = pkg.chromosome_regions(dist)
        # the exact value of one posterior cell: >= counts it
        inner = (marg > 0.2) & (marg < 0.8)
        i, s = [int(v[0]) for v in np.nonzero(inner)]
        thr = float(marg[i, s])
        reg, sites = h.ibd_summary(regions, threshold=thr)
        _check(reg, sites, path, marg, dist, regions, thr)
        above = int(np.count_nonzero(marg[:, s] > thr))
        assert sites["post_count"][s] == above + int(np.count_nonzero(marg[:, s] == thr)) > above
        reg, sites = h.ibd_summary(regions, threshold=np.nextafter(thr, 1.0))
        assert sites["post_count"][s] == int(np.count_nonzero(marg[:, s] > thr))
        reg, sites = h.ibd_summary(regions, threshold=1.0)
        _check(reg, sites, path, marg, dist, regions, 1.0)
        # each source alone: the other's fields are all zero
        reg, sites = h.ibd_summary(regions, what="viterbi", threshold=float("nan"))   # (not looked at)
        _check(reg, sites, path, marg, dist, regions, 0.5, posterior=False)
        assert not reg["post_sites"].any() and not reg["post_sum"].any()
        assert not sites["post_count"].any() and not sites["post_sum"].any() and reg["vit_sites"].any()
        reg, sites = h.ibd_summary(regions, what=("posterior",))
        _check(reg, sites, path, marg, dist, regions, 0.5, viterbi=False)
        assert not reg["vit_sites"].any() and not reg["vit_mb"].any() and not sites["vit_count"].any()
        assert reg["post_sum"].all()
        reg2, sites2 = h.ibd_summary(regions, what=pkg.SUMMARY_POSTERIOR)
        assert reg2.tobytes() == reg.tobytes() and sites2.tobytes() == sites.tobytes()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_chain_against_one_handle(pkg, edge_cohort, n_shards):
    """Site shards in fast mode, one boundary inside an IBD run and inside a region, one on a
    chromosome start.  The reference is the chain's own viterbi() and marg_prob.  The chain's
    posteriors are those of the handle over all sites only to 1e-9 (tests/test_gpu_siteshard.py),
    so "byte-identical to the single handle's" is held where it is defined: the Viterbi source's
    records against the handle over all sites (the decodes are bit-identical), and every
    source's records of a shard's sites against that shard asked as a single handle."""
    d, gl, (c1, c2) = edge_cohort
    dist = d.pos_dist_mb
    whole = _edge_handle(pkg, d, gl, pkg.MODE_FAST)
    whole.iter_EM(1, True, True)
    wpath = whole.viterbi()
    run = (wpath[:, :-1] == 1) & (wpath[:, 1:] == 1)
    # a boundary inside an IBD run, away from the segment edges and the chromosome starts
    cand = [s for s in range(SEG + 100, 2 * SEG - 100) if run[:, s - 1].any() and abs(s - c1) > 50]
    inside = next(s for s in cand[len(cand) // 2:] if s % 16 == 5)      # (not on a 16-site block edge)
    cuts = [0, inside, EDGE_S] if n_shards == 2 else [0, inside, c2, EDGE_S]
    hs = [_edge_handle(pkg, d, gl, pkg.MODE_FAST, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    ch = pkg.Chain(hs)
    ch.iter_EM(1, True, True)
    whole.set_params(hs[0].indF, hs[0].alpha, ch.freq)
    wpath = whole.viterbi()
    path, marg = ch.viterbi(), ch.marg_prob
    assert np.array_equal(path, wpath)
    assert ((path[:, inside - 1] == 1) & (path[:, inside] == 1)).any()
    region_sets = [
        [(0, 5), (inside - 40, inside + 60), (c2 - 3, c2 + 3), (EDGE_S - 9, EDGE_S)],   # across both boundaries
        [(0, EDGE_S)],
        [(inside - 1, inside), (inside, inside + 1), (c2, EDGE_S)],                      # begin at a boundary
    ]
    for regions in region_sets:
        regions = np.array(regions)
        reg, sites = ch.ibd_summary(regions)
        _check(reg, sites, path, marg, dist, regions)
        # the Viterbi source against the handle over all sites
        creg, csites = ch.ibd_summary(regions, what="viterbi")
        wreg, wsites = whole.ibd_summary(regions, what="viterbi")
        assert csites.tobytes() == wsites.tobytes()
        assert np.array_equal(creg["vit_sites"], wreg["vit_sites"])
        _, _, n_mb = summary_util.summarize(path, marg, dist, regions, posterior=False)
        _within(creg["vit_mb"], wreg["vit_mb"], n_mb, "chain vit_mb against one handle")
        # every shard's site records are those of the shard as a single handle
        for h, lo, hi in zip(hs, cuts[:-1], cuts[1:]):
            _, own = h.ibd_summary(None)
            assert sites[lo:hi].tobytes() == own.tobytes()
    reg, sites = ch.ibd_summary(None)
    assert reg is None
    _check(None, sites, path, marg, dist, None)
    a, b = ch.ibd_summary(np.array(region_sets[0])), ch.ibd_summary(np.array(region_sets[0]))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(pkg.NgsFHMMError) as ei:
        ch.ibd_summary(np.array([[0, EDGE_S + 1]]))
    assert ei.value.code == -10
    for h in hs:
        h.close()
    whole.close()


def _raw(h, what, thr, begin, end, regions=True, sites=True, n=None):
    u64 = C.POINTER(C.c_uint64)
    b = np.array(begin, dtype=np.uint64)
    e = np.array(end, dtype=np.uint64)
    n = len(b) if n is None else n
    rbuf = C.create_string_buffer(32 * h.n_ind * max(n, 1))
    sbuf = C.create_string_buffer(16 * h.n_sites)
    rc = h.lib.nghmm_ibd_summary(h.handle, what, thr, n, b.ctypes.data_as(u64) if len(b) else None,
                                 e.ctypes.data_as(u64) if len(e) else None,
                                 C.cast(rbuf, C.c_void_p) if regions else None,
                                 C.cast(sbuf, C.c_void_p) if sites else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_contract(pkg, edge_cohort):
    d, gl, (c1, c2) = edge_cohort
    dist = d.pos_dist_mb
    regions = pkg.window_regions(dist, 777)

    def run(with_summary):
        out = {}
        with _edge_handle(pkg, d, gl, pkg.MODE_FAST) as h:
            h.iter_EM(1)
            h.viterbi()
            if with_summary:
                a = h.ibd_summary(regions)
                b = h.ibd_summary(regions)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                h.ibd_summary(None, threshold=0.9)
                h.ibd_summary(regions[:2], what="viterbi", sites=False)
            out["params"] = (h.indF, h.alpha, h.freq, h.marg_prob)
            out["tracts"] = h.ibd_tracts("viterbi")
            h.iter_EM(1)
            out["after"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ind_lkl.copy())
        return out

    a, b = run(False), run(True)
    for k in ("params", "after"):
        for x, y in zip(a[k], b[k]):
            assert x.tobytes() == y.tobytes(), k
    assert a["tracts"].tobytes() == b["tracts"].tobytes()


def test_argument_errors(pkg, edge_cohort):
    d, gl, _ = edge_cohort
    S = EDGE_S
    V, P = pkg.SUMMARY_VITERBI, pkg.SUMMARY_POSTERIOR
    with pkg.NgsFHMM(EDGE_I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, P, 0.5, [0], [S])                     # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_summary(None)
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        F, A = _params(EDGE_I)
        h.set_params(F, A, 0.2)
        h.init_emission()
        # VITERBI before any decode is refused; POSTERIOR sees the zeros of no E-step
        for what in (V, V | P):
            rc, msg = _raw(h, what, 0.5, [0], [S])
            assert rc == -10 and "Viterbi" in msg
        reg, sites = h.ibd_summary(np.array([[0, S]]), what="posterior", threshold=1e-300)
        assert not reg["post_sites"].any() and not reg["post_sum"].any() and not sites["post_sum"].any()
        h.iter_EM(1, True, True)
        h.viterbi()
        assert _raw(h, V | P, 0.5, [0], [S])[0] == 0
        bad = [
            ((0, 0.5, [0], [S]), {}),                           # what == 0
            ((4, 0.5, [0], [S]), {}),                           # an unknown bit
            ((V | P | 8, 0.5, [0], [S]), {}),
            ((P, 0.0, [0], [S]), {}),                           # threshold outside (0, 1]
            ((P, -0.5, [0], [S]), {}),
            ((V | P, 1.5, [0], [S]), {}),
            ((P, float("nan"), [0], [S]), {}),
            ((V, 0.5, [10, 5], [20, 8]), {}),                   # unsorted
            ((V, 0.5, [0, 9], [10, 20]), {}),                   # overlapping
            ((V, 0.5, [0, 10], [10, 10]), {}),                  # empty
            ((V, 0.5, [5], [4]), {}),                           # end < begin
            ((V, 0.5, [0], [S + 1]), {}),                       # end > S
            ((V, 0.5, [0], [S]), {"regions": False}),           # NULL mismatch: regions missing
            ((V, 0.5, [], []), {"regions": True, "n": 0}),      # ... regions without n_regions
            ((V, 0.5, [], []), {"regions": False, "sites": False, "n": 0}),   # no output at all
        ]
        for args, kw in bad:
            rc, msg = _raw(h, *args, **kw)
            assert rc == -10 and msg, (args, kw, rc, msg)
        assert _raw(h, V, float("nan"), [0], [S])[0] == 0       # the threshold is POSTERIOR's
        assert _raw(h, V, 0.5, [0, 10], [10, S])[0] == 0        # touching regions do not overlap
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_summary(None, what="marginal")
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_summary(np.array([[0.0, 5.0]]))
        # a reload forgets the decode
        h.load(gl, d.pos_dist_mb)
        rc, msg = _raw(h, V, 0.5, [0], [S])
        assert rc == -10 and "Viterbi" in msg


CLI_I, CLI_S = 12, 3001


def test_cli_ibd_summary(pkg, tmp_path):
    """--ibd_summary in fast mode against the definitions applied to the same run's .ibd file and
    --pos file.  The .ibd file prints the posteriors with "%f": a printed value is within 5e-7
    of the value on the device, so the Viterbi columns are compared exactly (the doubles to the
    10 digits printed, plus the bound above), post_mean to 5e-7 plus the print, and post_sites /
    post_count between the counts of the printed values >= threshold + 1e-6 and >= threshold -
    1e-6."""
    tmp = str(tmp_path)
    d = pkg.simulate.simulate(CLI_I, CLI_S, seed=31, n_chrom=3, indF=0.6, alpha=0.05)
    paths = cli_util.write_inputs(tmp, d, d.gl)
    names = os.path.join(tmp, "names.txt")
    with open(names, "w") as fh:
        fh.write("".join(f"IND_{i:03d} pop{i % 2}\n" for i in range(CLI_I)))
    base = ["--geno", paths["glf_gz"], "--loglkl", "--pos", paths["pos_gz"], "--n_ind", CLI_I,
            "--n_sites", CLI_S, "--freq", 0.1, "--indF", "0.6,0.05", "--min_iters", 2, "--max_iters", 3,
            "--verbose", 0, "--mode", "fast"]
    plain, summ = os.path.join(tmp, "plain"), os.path.join(tmp, "summ")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", summ, "--ibd_summary", "--summary_window", 400, "--ind_names", names])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(summ + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".ibd.regions") and not os.path.exists(plain + ".ibd.sites")
    chrom, pos, dist = summary_util.read_pos(paths["pos_gz"])
    path, marg = summary_util.read_ibd(summ + ".ibd", CLI_I)
    regions = summary_util.chrom_regions(chrom, 400)
    reg, sites, n_mb = summary_util.summarize(path, marg, dist, regions, 0.5)
    hi_reg, hi_sites, _ = summary_util.summarize(path, marg, dist, regions, 0.5 - 1e-6)
    lo_reg, lo_sites, _ = summary_util.summarize(path, marg, dist, regions, 0.5 + 1e-6)
    assert path.any() and len(regions) >= 9

    lines = open(summ + ".ibd.regions").read().split("\n")
    assert lines[0] + "\n" == summary_util.REGIONS_HEADER and lines[-1] == "" and \
        len(lines) == 2 + CLI_I * len(regions)
    k = 1
    for i in range(CLI_I):
        for r, (a, b) in enumerate(regions):
            f = lines[k].split("\t")
            k += 1
            n = int(b - a)
            t = reg[i, r]
            assert f[:6] == [f"IND_{i:03d}", chrom[a], str(pos[a]), str(pos[b - 1]), str(n), str(int(t["vit_sites"]))]
            assert f[6] == "%.10g" % (int(t["vit_sites"]) / n)
            assert int(lo_reg["post_sites"][i, r]) <= int(f[7]) <= int(hi_reg["post_sites"][i, r])
            assert abs(float(f[8]) - float(t["post_sum"]) / n) <= 5e-7 + 1e-9
            mb = float(t["vit_mb"])
            assert abs(float(f[9]) - mb) <= (5e-10 + 2 * int(n_mb[i, r]) * U) * mb
    lines = open(summ + ".ibd.sites").read().split("\n")
    assert lines[0] + "\n" == summary_util.SITES_HEADER and lines[-1] == "" and len(lines) == 2 + CLI_S
    for s in range(CLI_S):
        f = lines[1 + s].split("\t")
        assert f[:3] == [chrom[s], str(pos[s]), str(int(sites["vit_count"][s]))]
        assert int(lo_sites["post_count"][s]) <= int(f[3]) <= int(hi_sites["post_count"][s])
        assert abs(float(f[4]) - float(sites["post_sum"][s]) / CLI_I) <= 5e-7 + 1e-9
