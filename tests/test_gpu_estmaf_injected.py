"""est_maf (the allele-frequency step) on likelihoods and posteriors of the test's choosing, at
both ends of every size class of its dispatch, in the site-major layout every individual-sharded
run uses (nghmm_mstep_freq_sites_dev) -- against the double oracle AND the binary128 anchor.

Inputs: tests/estmaf_cases.py (all families side by side in one launch).  Per cohort size three
runs on the same inputs: estmaf_interp 1 (the product's path), 0 (every pass exact), and up to
8192 individuals the exact-mode kernel, which must give the `det` oracle's bits.  Sizes up to 128
run with estmaf_no_rows 0 (four sites per wave) and 1 (the (1, 64) and (2, 64) register kernels).

With a the anchor, o the oracle, g the GPU and rel(x, y) = |x - y| / max(y, 1e-3):
  * always: g finite and in [0, 1];
  * estmaf_interp 0: rel(g, a) <= max(rel(o, a), 1e-12) where the anchor was computed (every site
    up to 1025 individuals, a fixed subsample holding every recipe above), rel(g, o) <= 1e-12
    elsewhere, except in the one_minus_eps families (anchor only: the oracle's own doubles cancel
    there);
  * estmaf_interp 1: the same with INTERP_BOUND, 1e-10 or 1e-12 by family (see there);
  * log-space sites (a called heterozygote at posterior exactly 1) against the oracle, which takes
    the same route in the same order: LOG_SPACE_BOUND;
  * a site whose stopping decision is marginal in the reference itself (a pass with |delta| within
    1e-6 relative of the threshold, or -- outside the one_minus_eps families -- oracle and anchor
    disagreeing on the pass count) only has to be within 1e-5 absolute of the oracle; at most
    0.5 % of a size's sites (test_estmaf_cases_cpu.py shows from the reference alone that the
    seeds keep to that; no site of the committed seeds is marginal);
  * routes: second_interval, third_interval and log_space are taken at every size the register
    kernels hold;
  * the site-major kernels reproduce the tile-major ones (the path the benchmark times) on the
    E-step's own posteriors bit for bit (measured so at all 50 runs up to 8192; asserted);
  * posterior blocks [I_tot / I_blk][S][I_blk] are addressing only: bit-identical results.

MEASURED on an MI355X, maxima over all sizes of the distance from the judging reference,
estmaf_interp 0 / 1:
  all_missing 1.5e-13 / 1.5e-13   flat 1.3e-13 / 1.3e-13   mono_ref 9.8e-16 / 9.8e-16
  mono_alt 1.1e-15 / 3.6e-15   one_minus_eps_mono 1.2e-15 / 1.2e-15
  one_minus_eps_sharp 8.0e-16 / 2.1e-13          -- these six: interpolated passes held to 1e-12
  called 7.3e-14 / 6.4e-13   one_first 1.2e-13 / 3.0e-13   one_edge_m1 1.2e-13 / 3.8e-13
  one_edge 1.5e-13 / 3.4e-13   one_last 1.3e-13 / 4.2e-13   one_minus_eps 3.1e-15 / 6.4e-13
  post_half 3.4e-15 / 5.9e-13   post_snapped 1.2e-15 / 6.3e-13   post_tiny 1.0e-15 / 6.0e-13
  sharp 2.3e-14 / 5.7e-13   sim_d2 9.0e-13 / 9.0e-13   sim_d5 5.5e-13 / 1.0e-12
  sim_d20 1.8e-13 / 5.5e-13                      -- these stay at 1e-10 with interpolation
  log-space sites (called_het1, called_snapped) against the oracle: 3.4e-12 either way.
The oracle itself against the anchor: up to 4.8e-12 outside the one_minus_eps families (serial
double sums over thousands of equal terms; hence ec.ANCHOR_EVERY_SITE), up to 8.9e-4 inside them.
Routes: second_interval 39 ... 61 sites, third_interval 3 ... 26, log_space 21 ... 29 at every size
up to 8192 (nothing is counted above: the streaming kernel).  check_failed was taken by 1 ... 4
sites at 1, 2, 3, 17 and 33 individuals only, and exact_tail by none at any size, with the sharp,
mono_* and one_minus_eps* families all present: exact_tail is unexercised by this module.

Two findings went into the kernels with this module: the log-space route took log 0 = -inf for a
dense one-hot likelihood where the reference has -1e15 (frequencies off by up to 0.5 on such
sites), and the streaming kernel formed the heterozygote's weight as the reference does,
2 b - 2 b F, which cancels for posteriors next to 1 (now 2 b (1 - F), as the register kernels).
"""
import ctypes as C
import importlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import estmaf_cases as ec
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

EXACT_TOL = 1e-12        # the project's number for est_maf fed the same posteriors
# estmaf_interp 1: 1e-10 is what test_est_maf_interpolated_passes_equal_exact_passes holds the
# interpolant to; families whose measured maximum (all sizes) was <= 2.5e-13 are held to 1e-12
INTERP_BOUND = {f: 1e-10 for f in ec.FAMILIES}
for _f in ("all_missing", "flat", "mono_ref", "mono_alt", "one_minus_eps_mono", "one_minus_eps_sharp"):
    INTERP_BOUND[_f] = 1e-12
# log-space sites against the oracle (terms of magnitude 1e15 on both sides): four times the
# measured maximum of 3.4e-12 (1e-9, what the frequencies are held to everywhere, is larger)
LOG_SPACE_BOUND = 4 * 3.4e-12
ANCHOR_ALL_UP_TO = 1025  # the anchor on every site up to here, on ec.anchor_sites above
THREADS = min(16, os.cpu_count() or 1)

_refs = {}


def rel(x, y):
    return np.abs(x - y) / np.maximum(y, 1e-3)


def references(I, orc_libm):
    """Inputs and CPU references of one cohort size (computed once per session)."""
    if I in _refs:
        return _refs[I]
    import orclib
    gl, post, labels = ec.cases(I)
    S = len(labels)
    anchor = orclib.HpAnchor()
    logsp = ec.log_space_sites(gl, post)
    a_sites = np.arange(S) if I <= ANCHOR_ALL_UP_TO else ec.anchor_sites(labels)

    def oracle(s):
        f, n, d = orc_libm.est_maf_trace(gl[s], post[s])
        return f, n, ec.marginal(d)

    def anch(s):
        return anchor.est_maf(gl[s], post[s])

    with ThreadPoolExecutor(THREADS) as pool:
        fa = [pool.submit(anch, s) for s in a_sites]     # the long ones first
        fo = [pool.submit(oracle, s) for s in range(S)]
        o = [f.result() for f in fo]
        a = [f.result() for f in fa]
    r = dict(gl=gl, post=post, labels=labels, logsp=logsp,
             o=np.array([x[0] for x in o]), on=np.array([x[1] for x in o]),
             marginal=np.array([x[2] for x in o]),
             a=np.full(S, np.nan), an=np.zeros(S, dtype=int), has_a=np.zeros(S, dtype=bool))
    r["a"][a_sites] = [x[0] for x in a]
    r["an"][a_sites] = [x[1] for x in a]
    r["has_a"][a_sites] = True
    r["has_a"] &= ~logsp      # (the anchor evaluates the model, not the reference's -1e15 stand-in)
    _refs.clear()             # one size at a time: the arrays of 9000 individuals are 65 MB
    _refs[I] = r
    return r


class Injected:
    """A handle whose frequency step runs on buffers of the test's choosing."""

    def __init__(self, pkg, I_tot, S, I_blk, mode, gl):
        import torch
        self.torch = torch
        dd = importlib.import_module("ngsf-hmm_amd.distributed")
        self.I_tot, self.S, self.I_blk = I_tot, S, I_blk
        self.be = dd.GpuBackend(pkg, I_blk, S, 0, mode)
        self.hmm = self.be.hmm
        self.dev = torch.device("cuda", 0)
        self.gl = gl
        self.configured = False

    def load_own(self):
        """The handle's own individuals (the first block) and site distances."""
        pos = np.full(self.S, 0.01)
        pos[0] = np.inf
        self.hmm.load(np.ascontiguousarray(self.gl[:, :self.I_blk]), pos)

    def configure(self):
        self.be.shard_config(self.I_tot, 0, 0, self.S)
        self.be.load_site_shard_device(self.torch.from_numpy(self.gl).to(self.dev))
        self.configured = True

    def run(self, post):
        """post [S][I_tot] -> frequencies [S]."""
        if not self.configured:
            self.configure()
        nb = self.I_tot // self.I_blk
        blocks = np.ascontiguousarray(post.reshape(self.S, nb, self.I_blk).transpose(1, 0, 2))
        out = self.be.empty(self.S)
        self.torch.cuda.synchronize()
        self.be.mstep_freq_sites(self.torch.from_numpy(blocks).to(self.dev), out)
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def close(self):
        self.hmm.close()


def _sizes():
    for I in ec.SIZES:
        yield pytest.param(I, 0, id=f"{I}")
        if I <= 128:
            yield pytest.param(I, 1, id=f"{I}-no_rows")


@pytest.mark.parametrize("I,no_rows", list(_sizes()))
def test_est_maf_on_injected_posteriors(pkg, orc_libm, orc_det, capsys, I, no_rows):
    r = references(I, orc_libm)
    gl, post, labels = r["gl"], r["post"], r["labels"]
    S = len(labels)
    o, a, has_a, logsp = r["o"], r["a"], r["has_a"], r["logsp"]
    assert np.all(np.isfinite(a[has_a])), "the anchor is finite wherever no cell's weights vanish"
    ome = np.isin(labels, ec.ONE_MINUS_EPS)
    # the reference's own stopping decision is marginal: value comparison replaced by 1e-5 absolute.
    # (Pass counts that differ inside the one_minus_eps families excuse nothing: the oracle is up
    # to 1e-4 from the anchor there, the counts differ often, and the anchor judges those sites
    # anyway -- the bound max(rel(o, a), tol) already holds the oracle's own distance.)
    left_out = r["marginal"] | (has_a & ~ome & (r["an"] != r["on"]))
    assert left_out.sum() <= 0.005 * S, (I, np.flatnonzero(left_out))
    judge = np.where(has_a & ome, np.where(has_a, a, 0.0), o)   # whom a left-out site stays near

    inj = Injected(pkg, I, S, I, pkg.MODE_FAST, gl)
    got, tile = {}, None
    try:
        inj.hmm.set_switch("estmaf_no_rows", no_rows)
        inj.load_own()
        if I <= 8192:
            # the tile-major kernels on the E-step's own posteriors, then the site-major ones on
            # exactly those
            inj.hmm.set_params(0.1, 0.2, 0.1)
            inj.hmm.init_emission()
            inj.hmm.estep()
            inj.hmm.mstep_freq(1)
            tile = inj.hmm.freq
            own_post = np.ascontiguousarray(inj.hmm.marg_prob.T)
            site = inj.run(own_post)
            assert np.all(np.isfinite(tile)) and np.all(np.isfinite(site))
            d_layout = rel(site, tile).max()
            assert np.array_equal(site, tile), (I, d_layout)
        inj.hmm.estmaf_counts(reset=True)
        got[1] = inj.run(post)
        counts = inj.hmm.estmaf_counts()
        inj.hmm.set_switch("estmaf_interp", 0)
        got[0] = inj.run(post)
    finally:
        inj.close()

    if I <= 8192:
        # exact mode: k_estmaf_exact keeps the reference's serial sum, the det oracle's bits
        ex = Injected(pkg, I, S, I, pkg.MODE_EXACT, gl)
        try:
            exact = ex.run(post)
        finally:
            ex.close()
        with ThreadPoolExecutor(THREADS) as pool:
            det = np.array(list(pool.map(lambda s: orc_det.est_maf(gl[s], post[s])[0], range(S))))
        assert np.array_equal(exact, det), (I, np.flatnonzero(exact != det)[:10])

    report = [f"est_maf injected I={I} no_rows={no_rows} layout_vs_tile="
              f"{'-' if tile is None else '%.1e' % d_layout} routes={counts}"]
    failures = []
    for interp in (0, 1):
        g = got[interp]
        assert np.all(np.isfinite(g)) and np.all((g >= 0) & (g <= 1)), \
            (I, interp, labels[~(np.isfinite(g) & (g >= 0) & (g <= 1))])
        # distance from the reference that judges the site, and the bound
        dist = np.where(has_a, rel(g, np.where(has_a, a, 0.0)), rel(g, o))
        tol = np.array([EXACT_TOL if interp == 0 else INTERP_BOUND[f] for f in labels])
        bound = np.where(has_a, np.maximum(rel(o, np.where(has_a, a, o)), tol), tol)
        bound[logsp] = LOG_SPACE_BOUND
        judged = ~left_out & (has_a | ~ome)
        bad = judged & ~(dist <= bound)
        for s in np.flatnonzero(bad):
            failures.append(f"interp={interp} site {s} {labels[s]}: g={g[s]!r} o={o[s]!r} a={a[s]!r} "
                            f"dist={dist[s]:.3e} bound={bound[s]:.3e}")
        lo = left_out & (has_a | ~ome)
        assert np.all(np.abs(g[lo] - judge[lo]) <= 1e-5), (I, interp, np.flatnonzero(lo))
        line = []
        for f in ec.FAMILIES:
            m = (labels == f) & judged
            line.append(f"{f}:{dist[m].max():.1e}" if m.any() else f"{f}:-")
        info = ""
        if interp == 0 and has_a.any():
            info = f" | oracle_vs_anchor one_minus_eps={rel(o, np.where(has_a, a, o))[has_a & ome].max():.1e}" \
                   f" others={rel(o, np.where(has_a, a, o))[has_a & ~ome].max():.1e}"
        report.append(f"  interp={interp} max dist by family: " + " ".join(line) + info)
    with capsys.disabled():
        print("\n" + "\n".join(report))
    assert not failures, "\n".join(failures[:20])
    if I <= 8192:   # the register kernels: the families are built to leave the common route
        assert counts["second_interval"] > 0 and counts["third_interval"] > 0, counts
        assert counts["log_space"] > 0, counts
    else:           # the streaming kernel takes the log-space route per cell, nothing is counted
        assert counts["second_interval"] == 0 and counts["third_interval"] == 0, counts


@pytest.mark.parametrize("I,n_blocks,no_rows", [(64, 2, 0), (128, 4, 0), (128, 4, 1), (1025, 25, 0),
                                                (4096, 8, 0), (9000, 9, 0)])
def test_posterior_blocks_are_addressing_only(pkg, I, n_blocks, no_rows):
    """The rank blocks [I_tot / I_blk][S][I_blk] the all-to-all delivers, against one block of
    all individuals: the same bits, with interpolated and with exact passes."""
    gl, post, labels = ec.cases(I)
    S = len(labels)
    out = {}
    for nb in (1, n_blocks):
        inj = Injected(pkg, I, S, I // nb, pkg.MODE_FAST, gl)
        try:
            inj.hmm.set_switch("estmaf_no_rows", no_rows)
            inj.load_own()
            out[nb, 1] = inj.run(post)
            inj.hmm.set_switch("estmaf_interp", 0)
            out[nb, 0] = inj.run(post)
        finally:
            inj.close()
    for interp in (0, 1):
        assert np.all(np.isfinite(out[1, interp]))
        assert np.array_equal(out[1, interp], out[n_blocks, interp]), (I, n_blocks, interp)
