"""Pairwise IBD sharing on the device (nghmm_ibd_sharing / nghmm_chain_ibd_sharing,
include/nghmm.h) against the numpy restatement of the definitions (tests/sharing_util.py) applied
to the handle's own viterbi() and marg_prob.

Counts must be equal.  post_prod must be within 2 (n + 1) 2^-53 |want| element by element, n the
sites in the range: both sides add n non-negative products, and any order, fused or not, is
within (n + 1) 2^-53 relative of the exact sum."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import cli_util
import sharing_util
import summary_util
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# the least sites per K-split: kSharingSplit of csrc/kernels_sharing.hpp (tests/test_sharing_cpu.py
# holds the two to each other)
SPLIT = importlib.import_module("ngsf-hmm_amd").SHARING_SPLIT_SITES
U = 2.0 ** -53


def _within(got, want, n, what):
    """|got - want| <= 2 (n + 1) u |want| element by element; prints the worst ratio to the bound."""
    got, want = np.asarray(got), np.asarray(want)
    bound = 2.0 * (n + 1) * U * np.abs(want)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), initial=0.0)
    print(f"{what}: worst error / bound = {worst:.3g}")
    assert (err <= bound).all(), (what, worst)


def _check(got, path, marg, thr=0.5, begin=0, end=None, what=""):
    end = path.shape[1] if end is None else end
    vit, both, prod = sharing_util.sharing(path, marg, thr, begin, end)
    I = path.shape[0]
    for name, want in (("vit_both", vit), ("post_both", both)):
        if name in got:
            assert got[name].shape == (I, I) and got[name].dtype == np.uint64
            assert np.array_equal(got[name], want), (what, name, begin, end)
    if "post_prod" in got:
        assert got["post_prod"].shape == (I, I) and got["post_prod"].dtype == np.float64
        _within(got["post_prod"], prod, end - begin, f"{what} post_prod [{begin}, {end})")
        assert np.array_equal(got["post_prod"], got["post_prod"].T)
    return vit, both, prod


def _params(n):
    F = np.linspace(0.05, 0.95, n)
    A = np.full(n, 0.05)
    A[:min(5, n)] = 1e-3
    A[-min(5, n):] = 1e-3
    return F, A


def _decoded(pkg, n_ind, n_sites, mode, seed, packed=False):
    d = pkg.simulate.simulate(n_ind, n_sites, seed=seed, n_chrom=2 if n_sites > 20 else 1, indF=0.7,
                              alpha=0.05)
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


SITE_COUNTS = (3, 4, 5, 16, 17, 63, 64, 65)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("n_ind", [1, 15, 16, 17, 33, 130])
def test_tile_and_step_shapes(pkg, n_ind, mode):
    """Individuals around the 16 x 16 tile and the 64 x 64 block, sites around the f64
    instruction's 4, the 16-site block and the int8 instruction's 64."""
    for n_sites in SITE_COUNTS:
        d, h = _decoded(pkg, n_ind, n_sites, pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT,
                        seed=n_ind + n_sites)
        with h:
            path, marg = h.viterbi(), h.marg_prob
            got = h.ibd_sharing()
            assert sorted(got) == ["post_both", "post_prod", "vit_both"]
            vit, _, _ = _check(got, path, marg, what=f"{n_ind} x {n_sites}")
            assert np.array_equal(np.diag(got["vit_both"]), path.sum(axis=1).astype(np.uint64))
            if n_sites > 2:
                _check(h.ibd_sharing(site_begin=1, site_end=n_sites - 1), path, marg, 0.5, 1, n_sites - 1)


def test_packed_handle(pkg):
    d, h = _decoded(pkg, 33, SPLIT + 17, pkg.MODE_FAST, seed=3, packed=True)
    with h:
        path, marg = h.viterbi(), h.marg_prob
        vit, _, _ = _check(h.ibd_sharing(), path, marg, what="packed")
        assert vit.any()


EDGE_I, EDGE_S = 40, 2 * SPLIT + 5


@pytest.fixture(scope="module")
def edge_cohort(pkg):
    d = pkg.simulate.simulate(EDGE_I, EDGE_S, seed=7, n_chrom=3, indF="r", alpha="r", missing_rate=0.02)
    return d, pkg.simulate.normalise_log_gl(d.gl)


def _edge_handle(pkg, d, gl, mode, lo=0, hi=EDGE_S):
    h = pkg.NgsFHMM(EDGE_I, hi - lo, mode=mode)
    h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
    F, A = _params(EDGE_I)
    h.set_params(F, A, 0.2)
    h.init_emission()
    return h


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_range_edges_and_splits(pkg, edge_cohort, mode):
    """More than one K-split is added; the range begins and ends off the 4-site step, the 16-site
    block, the 64-site step and the split edge."""
    d, gl = edge_cohort
    S = EDGE_S
    first, length, n_splits = pkg.sharing_splits(EDGE_I, 0, S)
    assert n_splits > 1 and first == 0 and length % 64 == 0 and S % 16 != 0
    with _edge_handle(pkg, d, gl, pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) as h:
        h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
        path, marg = h.viterbi(), h.marg_prob
        vit, both, prod = _check(h.ibd_sharing(), path, marg, what="all sites")
        # a row / column swap inside an off-diagonal tile must not pass: the expected tile of the
        # individuals 0..15 x 16..31 is not symmetric
        tile = vit[0:16, 16:32].astype(np.int64)
        assert (tile != tile.T).any()
        a, b = [int(v[0]) for v in np.nonzero(tile != tile.T)]
        assert a != b and vit[a, 16 + b] != vit[b, 16 + a]
        tile = prod[0:16, 16:32]
        assert (tile != tile.T).any() and both.any() and (both != vit).any()
        for begin in (0, 1, 3, 15, 17):
            ends = {begin + 1, begin + 2, 63, 64, 65, length - 1, length, length + 1, S - 1, S}
            for end in sorted(e for e in ends if e > begin):
                _check(h.ibd_sharing(site_begin=begin, site_end=end), path, marg, 0.5, begin, end, mode)
        _check(h.ibd_sharing(site_begin=length + 3, site_end=2 * length + 70), path, marg, 0.5,
               length + 3, 2 * length + 70, "inside")


def test_single_outputs_and_threshold_edge(pkg, edge_cohort):
    d, gl = edge_cohort
    with _edge_handle(pkg, d, gl, pkg.MODE_FAST) as h:
        h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
        path, marg = h.viterbi(), h.marg_prob
        allthree = h.ibd_sharing(site_begin=3, site_end=EDGE_S - 1)
        _check(allthree, path, marg, 0.5, 3, EDGE_S - 1)
        # each source and each output alone: the same bytes
        for what, names in (("viterbi", ["vit_both"]), ("posterior", ["post_both", "post_prod"]),
                            ("vit_both", ["vit_both"]), ("post_both", ["post_both"]),
                            ("post_prod", ["post_prod"]), (("post_prod", "vit_both"), ["post_prod", "vit_both"])):
            # (the threshold is only looked at when post_both is asked for)
            thr = 0.5 if "post_both" in names else float("nan")
            got = h.ibd_sharing(what, threshold=thr, site_begin=3, site_end=EDGE_S - 1)
            assert sorted(got) == names
            for k in names:
                assert got[k].tobytes() == allthree[k].tobytes(), (what, k)
        # the exact value of one posterior cell: >= counts it
        inner = (marg > 0.2) & (marg < 0.8)
        i, s = [int(v[0]) for v in np.nonzero(inner)]
        thr = float(marg[i, s])
        got = h.ibd_sharing("posterior", threshold=thr)
        _check(got, path, marg, thr)
        at = h.ibd_sharing("post_both", threshold=thr, site_begin=s, site_end=s + 1)["post_both"]
        assert at[i, i] == 1
        up = h.ibd_sharing("post_both", threshold=np.nextafter(thr, 1.0), site_begin=s, site_end=s + 1)
        assert up["post_both"][i, i] == 0
        _check(up, path, marg, np.nextafter(thr, 1.0), s, s + 1)
        _check(h.ibd_sharing("posterior", threshold=1.0), path, marg, 1.0)


@pytest.mark.parametrize("n_shards", [2, 3])
def test_chain_against_one_handle(pkg, edge_cohort, n_shards):
    """Site shards in fast mode on one device; a range inside one shard, one from inside the first
    shard to inside the last, and all sites.  Against the restatement applied to the chain's own
    viterbi() and marg_prob: counts equal, post_prod within the bound.  Against the handle over
    all sites asked the same question: the counts equal (the decodes are bit-identical; no
    posterior of this cohort is within 1e-8 of the threshold), post_prod to 1e-8 -- the chain's
    posteriors are the whole handle's only to 1e-9 (tests/test_gpu_siteshard.py), so the bound,
    which is about the order of one sum's terms, is not defined across the two."""
    d, gl = edge_cohort
    S = EDGE_S
    cuts = [0, 1001, S] if n_shards == 2 else [0, 1001, 1500, S]
    whole = _edge_handle(pkg, d, gl, pkg.MODE_FAST)
    whole.iter_EM(1, True, True)
    hs = [_edge_handle(pkg, d, gl, pkg.MODE_FAST, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    ch = pkg.Chain(hs)
    ch.iter_EM(1, True, True)
    whole.set_params(hs[0].indF, hs[0].alpha, ch.freq)
    wpath, wmarg = whole.viterbi(), whole.marg_prob
    path, marg = ch.viterbi(), ch.marg_prob
    assert np.array_equal(path, wpath)
    assert (np.abs(wmarg - 0.5) > 1e-8).all() and (np.abs(marg - 0.5) > 1e-8).all()
    for begin, end in ((1100, 1400), (3, S - 7), (0, S), (1001, 1002), (1000, 1001)):
        got = ch.ibd_sharing(site_begin=begin, site_end=end)
        _check(got, path, marg, 0.5, begin, end, f"chain of {n_shards}")
        one = whole.ibd_sharing(site_begin=begin, site_end=end)
        assert got["vit_both"].tobytes() == one["vit_both"].tobytes()
        assert np.array_equal(got["post_both"], one["post_both"])
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.nanmax(np.abs(got["post_prod"] - one["post_prod"]) / one["post_prod"])
        print(f"chain of {n_shards} [{begin}, {end}): post_prod against one handle, worst relative {rel:.3g}")
        np.testing.assert_allclose(got["post_prod"], one["post_prod"], rtol=1e-8, atol=0)
    # a range inside one shard: that shard's own answer, the other shards are not asked
    own = hs[1].ibd_sharing(site_begin=1100 - 1001, site_end=1400 - 1001)
    got = ch.ibd_sharing(site_begin=1100, site_end=1400)
    for k in own:
        assert own[k].tobytes() == got[k].tobytes(), k
    a, b = ch.ibd_sharing(site_begin=3, site_end=S - 7), ch.ibd_sharing(site_begin=3, site_end=S - 7)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    with pytest.raises(pkg.NgsFHMMError) as ei:
        ch.ibd_sharing(site_end=S + 1)
    assert ei.value.code == -10
    for h in hs:
        h.close()
    with pytest.raises(pkg.NgsFHMMError) as ei:       # a chain that was not set up
        u64 = C.POINTER(C.c_uint64)
        arr = (C.c_void_p * 2)(whole.handle, whole.handle)
        buf = np.zeros((EDGE_I, EDGE_I), dtype=np.uint64)
        whole._check(whole.lib.nghmm_chain_ibd_sharing(arr, 2, pkg.SHARING_VITERBI, 0.5, 0, 5,
                                                       buf.ctypes.data_as(u64), None, None))
    assert ei.value.code == -10 and ei.value.message
    whole.close()


def test_contract(pkg, edge_cohort):
    """The same bits on a second call, which does not allocate; read-only."""
    import torch
    d, gl = edge_cohort

    def run(with_sharing):
        out = {}
        with _edge_handle(pkg, d, gl, pkg.MODE_FAST) as h:
            h.iter_EM(1)
            h.viterbi()
            if with_sharing:
                a = h.ibd_sharing()
                torch.cuda.synchronize()
                free = torch.cuda.mem_get_info()[0]
                b = h.ibd_sharing()
                assert torch.cuda.mem_get_info()[0] == free
                for k in a:
                    assert a[k].tobytes() == b[k].tobytes(), k
                h.ibd_sharing("posterior", threshold=0.9, site_begin=5, site_end=77)
                h.ibd_sharing("viterbi", site_begin=EDGE_S - 1)
            out["params"] = (h.indF, h.alpha, h.freq, h.marg_prob)
            h.iter_EM(1)
            out["after"] = (h.indF, h.alpha, h.freq, h.marg_prob, h.ind_lkl.copy())
        return out

    a, b = run(False), run(True)
    for k in ("params", "after"):
        for x, y in zip(a[k], b[k]):
            assert x.tobytes() == y.tobytes(), k


def _raw(h, what, thr, begin, end, vit=True, both=True, prod=True):
    u64 = C.POINTER(C.c_uint64)
    n = h.n_ind * h.n_ind
    v, b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    p = np.zeros(n, dtype=np.float64)
    rc = h.lib.nghmm_ibd_sharing(h.handle, what, thr, begin, end,
                                 v.ctypes.data_as(u64) if vit else None,
                                 b.ctypes.data_as(u64) if both else None,
                                 p.ctypes.data_as(C.POINTER(C.c_double)) if prod else None)
    return rc, h.lib.nghmm_last_error().decode()


def test_argument_errors(pkg, edge_cohort):
    d, gl = edge_cohort
    S = EDGE_S
    V, P = pkg.SHARING_VITERBI, pkg.SHARING_POSTERIOR
    with pkg.NgsFHMM(EDGE_I, S, mode=pkg.MODE_FAST) as h:
        rc, msg = _raw(h, P, 0.5, 0, S, vit=False)                      # a handle without data
        assert rc == -10 and "no data" in msg
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_sharing("posterior")
        assert ei.value.code == -10 and ei.value.message
        h.load(gl, d.pos_dist_mb)
        F, A = _params(EDGE_I)
        h.set_params(F, A, 0.2)
        h.init_emission()
        for what in (V, V | P):                                        # no decode since the load
            rc, msg = _raw(h, what, 0.5, 0, S, both=what & P, prod=what & P)
            assert rc == -10 and "Viterbi" in msg
        h.iter_EM(1, True, True)
        h.viterbi()
        assert _raw(h, V | P, 0.5, 0, S)[0] == 0
        nan = float("nan")
        bad = [
            ((0, 0.5, 0, S), {}),                                       # what == 0
            ((0, 0.5, 0, S), {"vit": False, "both": False, "prod": False}),
            ((4, 0.5, 0, S), {}),                                       # an unknown bit
            ((V | P | 8, 0.5, 0, S), {}),
            ((V | P, 0.5, 5, 5), {}),                                   # site_begin >= site_end
            ((V | P, 0.5, 6, 5), {}),
            ((V | P, 0.5, 0, S + 1), {}),                               # site_end > S
            ((P, 0.0, 0, S), {"vit": False}),                           # threshold outside (0, 1]
            ((P, -0.5, 0, S), {"vit": False}),
            ((V | P, 1.5, 0, S), {}),
            ((P, nan, 0, S), {"vit": False}),
            ((P, nan, 0, S), {"vit": False, "prod": False}),
            ((V, 0.5, 0, S), {}),                                       # NULL mismatch: an unselected source's pointer
            ((V, 0.5, 0, S), {"both": False}),
            ((P, 0.5, 0, S), {}),
            ((V, 0.5, 0, S), {"vit": False, "both": False, "prod": False}),   # a selected source without a pointer
            ((V | P, 0.5, 0, S), {"both": False, "prod": False}),
            ((V | P, 0.5, 0, S), {"vit": False}),
        ]
        for args, kw in bad:
            rc, msg = _raw(h, *args, **kw)
            assert rc == -10 and msg, (args, kw, rc, msg)
        assert _raw(h, P, nan, 0, S, vit=False, both=False)[0] == 0    # the threshold is post_both's
        assert _raw(h, V, nan, 0, S, both=False, prod=False)[0] == 0
        assert _raw(h, V | P, 1.0, S - 1, S)[0] == 0
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_sharing("marginal")
        h.load(gl, d.pos_dist_mb)                                       # a reload forgets the decode
        rc, msg = _raw(h, V, 0.5, 0, S, both=False, prod=False)
        assert rc == -10 and "Viterbi" in msg


CLI_I, CLI_S = 6, 300


def test_cli_ibd_sharing(pkg, tmp_path):
    """--ibd_sharing in fast mode against the definitions applied to the same run's .ibd file.
    The .ibd file prints the posteriors with "%f": a printed value is within 5e-7 of the value on
    the device, so vit_both is compared exactly, post_both between the counts of the printed
    values >= threshold + 1e-6 and >= threshold - 1e-6, and post_prod to the sum of the products'
    errors, 1e-6 + 2.5e-13 a site, plus the 10 digits printed."""
    tmp = str(tmp_path)
    d = pkg.simulate.simulate(CLI_I, CLI_S, seed=31, n_chrom=2, indF=0.6, alpha=0.05)
    paths = cli_util.write_inputs(tmp, d, d.gl)
    base = ["--geno", paths["glf_gz"], "--loglkl", "--pos", paths["pos_gz"], "--n_ind", CLI_I,
            "--n_sites", CLI_S, "--freq", 0.1, "--indF", "0.6,0.05", "--min_iters", 2, "--max_iters", 3,
            "--verbose", 0, "--mode", "fast"]
    plain, shar = os.path.join(tmp, "plain"), os.path.join(tmp, "shar")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", shar, "--ibd_sharing"])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(shar + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".ibd.sharing")
    path, marg = summary_util.read_ibd(shar + ".ibd", CLI_I)
    vit, _, prod = sharing_util.sharing(path, marg, 0.5)
    _, lo, _ = sharing_util.sharing(path, marg, 0.5 + 1e-6)
    _, hi, _ = sharing_util.sharing(path, marg, 0.5 - 1e-6)
    ids, gvit, gboth, gprod = sharing_util.parse_sharing(open(shar + ".ibd.sharing").read(), CLI_I)
    assert ids == [f"ind{i}" for i in range(CLI_I)] and path.any()
    assert np.array_equal(gvit, vit)
    assert (lo <= gboth).all() and (gboth <= hi).all()
    assert (np.abs(gprod - prod) <= CLI_S * (1e-6 + 2.5e-13) + 5e-10 * prod).all()
