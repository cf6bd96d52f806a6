"""BASELINE.json configs[3] and configs[4] at their SHARDED shape, on the one GPU a test box
has: eight handles on cuda:0 play the eight GPUs of the node.

* configs[3] (1000 individuals x 1 M sites sharded by individual over 8 GPUs): 8 handles of
  125 x 1 M through nghmm_group_setup / nghmm_group_iter_em -- the posterior exchange (peer
  copies here between buffers of one device, xGMI on a node), est_maf per site range over all
  1000 individuals in global order, the frequency exchange -- against ONE handle that owns all
  1000 individuals.  What is split: EM.cpp:147-272.
* configs[4] (5000 x 5 M, 25 chromosomes, --call_geno, 100 iterations, 8 GPUs): 8 packed
  handles of 625 individuals x 625 000 sites (config 5's individuals per GPU and chromosome
  count, an eighth of its sites so that the cohort fits one device), against one packed handle
  of 5000 x 625 000; and the 100 iterations the config asks for at 625 x 500 000.
* the same job through bench.py's process-per-rank path with four ranks (gloo on one GPU).

The optimizer's finite differences amplify last-bit differences of the objective (SURVEY
finding 4), and a 125-individual handle cuts the site axis into other lane-chunks than a
1000-individual one, so free-parameter runs are compared TEACHER-FORCED: every iteration starts
from the single handle's parameters.  With fixed parameters nothing is forced.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _iterate_pair(whole, grp, parts, n_iter, fixed, force):
    """n_iter EM iterations of both; returns the worst relative differences seen."""
    I_loc = parts[0].n_ind
    worst = dict(lkl=0.0, freq=0.0, indF=0.0)
    for it in range(n_iter):
        if force:
            F, A, f = whole.indF, whole.alpha, whole.freq
            for r, h in enumerate(parts):
                h.set_params(F[r * I_loc:(r + 1) * I_loc], A[r * I_loc:(r + 1) * I_loc], f)
                h.init_emission()
        whole.iter_EM(1, fixed, fixed)
        st = grp.iter_EM(1, fixed, fixed)
        assert fixed or st.rounds > 0
        lk_w, lk_g = whole.ind_lkl, grp.ind_lkl
        assert np.isfinite(lk_w).all()
        worst["lkl"] = max(worst["lkl"], float(np.max(np.abs(lk_g - lk_w) / np.abs(lk_w))))
        fw, fg = whole.freq, parts[0].freq
        assert np.array_equal(fg, parts[-1].freq)            # everybody holds the same frequencies
        worst["freq"] = max(worst["freq"], float(np.max(np.abs(fg - fw) / fw)))
        gF = np.concatenate([h.indF for h in parts])
        worst["indF"] = max(worst["indF"], float(np.max(np.abs(gF - whole.indF))))
    return worst


def test_config4_eight_shards_of_1000_x_1M(pkg):
    import torch
    I, S, n = 1000, 1_000_000, 8
    I_loc = I // n
    dev = torch.device("cuda", 0)
    gl, pos = pkg.simulate.simulate_torch(I, S, dev, seed=2025)
    pos[S // 3] = float("inf")
    pos[2 * S // 3] = float("inf")               # three chromosomes
    torch.cuda.synchronize()

    whole = pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST)
    whole.load_device(gl.data_ptr(), pos.data_ptr())
    parts = []
    for r in range(n):
        h = pkg.NgsFHMM(I_loc, S, mode=pkg.MODE_FAST)
        cols = gl[:, r * I_loc:(r + 1) * I_loc, :].contiguous()
        torch.cuda.synchronize()
        h.load_device(cols.data_ptr(), pos.data_ptr())
        del cols
        parts.append(h)
    del gl
    torch.cuda.empty_cache()
    for h in parts + [whole]:
        h.set_params(0.1, 0.2, 0.1)
        h.init_emission()
    grp = pkg.Group(parts)                         # builds the site-shard copies (peer copies)

    free = _iterate_pair(whole, grp, parts, 3, fixed=False, force=True)
    print("config 4 shape, free parameters (teacher-forced):", free)
    assert free["lkl"] < 1e-12 and free["freq"] < 1e-9 and free["indF"] < 1e-4

    for h in parts + [whole]:
        h.set_params(0.3, 0.05, 0.15)
        h.init_emission()
    fix = _iterate_pair(whole, grp, parts, 3, fixed=True, force=False)
    print("config 4 shape, fixed parameters:", fix)
    assert fix["lkl"] < 1e-12 and fix["freq"] < 1e-9 and fix["indF"] == 0.0
    # decoding with the frequencies each side arrived at on its own (they agree to 1e-9, the
    # decoder takes the argmax of sums of their logs): identical paths
    path_w = whole.viterbi()
    for r, h in enumerate(parts):
        p = h.viterbi()
        assert np.array_equal(p, path_w[r * I_loc:(r + 1) * I_loc]), r
        del p
    for h in parts + [whole]:
        h.close()


def test_config4_as_a_chain_of_eight_site_shards(pkg):
    """The same job cut along the SITE axis (what bench.py --gpus 8 and the host's --n_gpus 8 do
    in fast mode): eight handles of 1000 x 125 000 through nghmm_chain_setup / _iter_em /
    _viterbi against ONE handle of 1000 x 1 M."""
    import importlib
    import torch
    dd = importlib.import_module("ngsf-hmm_amd.distributed")
    I, S, n = 1000, 1_000_000, 8
    dev = torch.device("cuda", 0)
    gl, pos = pkg.simulate.simulate_torch(I, S, dev, seed=2025)
    pos[S // 3] = float("inf")
    pos[2 * S // 3] = float("inf")               # three chromosomes, none starting at a cut
    torch.cuda.synchronize()
    whole = pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST)
    whole.load_device(gl.data_ptr(), pos.data_ptr())
    ranges = dd.site_ranges_ragged(S, n)
    parts = []
    for lo, hi in ranges:
        h = pkg.NgsFHMM(I, hi - lo, mode=pkg.MODE_FAST)
        h.load_device(gl[lo:hi].data_ptr(), pos[lo:hi].data_ptr())     # contiguous slices
        parts.append(h)
    del gl
    torch.cuda.empty_cache()
    ch = pkg.Chain(parts)

    def set_all(F, A, f):
        whole.set_params(F, A, f)
        whole.init_emission()
        for (lo, hi), h in zip(ranges, parts):
            h.set_params(F, A, np.broadcast_to(f, (S,))[lo:hi])
            h.init_emission()
    worst = dict(lkl=0.0, freq=0.0, indF=0.0)
    F, A, f = 0.1, 0.2, 0.1
    for it in range(3):                            # free parameters, teacher-forced
        set_all(F, A, f)
        whole.iter_EM(1)
        st = ch.iter_EM(1)
        assert st.rounds > 0
        for h in parts[1:]:
            assert np.array_equal(h.indF, parts[0].indF) and np.array_equal(h.alpha, parts[0].alpha)
        worst["lkl"] = max(worst["lkl"], float(np.max(np.abs(ch.ind_lkl - whole.ind_lkl) / np.abs(whole.ind_lkl))))
        worst["freq"] = max(worst["freq"], float(np.max(np.abs(ch.freq - whole.freq) / whole.freq)))
        worst["indF"] = max(worst["indF"], float(np.max(np.abs(parts[0].indF - whole.indF))))
        F, A, f = whole.indF, whole.alpha, whole.freq
    print("config 4 as a chain, free parameters (teacher-forced):", worst)
    assert worst["lkl"] < 1e-12 and worst["freq"] < 1e-9 and worst["indF"] < 1e-4
    set_all(0.3, 0.05, 0.15)
    for it in range(3):
        whole.iter_EM(1, True, True)
        ch.iter_EM(1, True, True)
    lk = float(np.max(np.abs(ch.ind_lkl - whole.ind_lkl) / np.abs(whole.ind_lkl)))
    fr = float(np.max(np.abs(ch.freq - whole.freq) / whole.freq))
    print("config 4 as a chain, fixed parameters:", dict(lkl=lk, freq=fr))
    assert lk < 1e-12 and fr < 1e-9
    # posteriors of a few hundred individuals (the whole matrix twice on the host is 16 GB)
    pw = whole.marg_prob[::4]
    pc = np.concatenate([h.marg_prob[::4] for h in parts], axis=1)
    assert float(np.max(np.abs(pc - pw))) < 1e-9
    del pw, pc
    set_all(0.3, 0.05, whole.freq)                 # one set of frequencies for both decoders
    assert np.array_equal(ch.viterbi(), whole.viterbi())
    for h in parts + [whole]:
        h.close()


def test_config5_eight_packed_shards(pkg):
    import torch
    I, S, n, nchr = 5000, 625_000, 8, 25
    I_loc = I // n
    dev = torch.device("cuda", 0)
    mode = pkg.MODE_FAST | pkg.GENO_PACKED
    whole = pkg.NgsFHMM(I, S, mode=mode)
    parts = [pkg.NgsFHMM(I_loc, S, mode=mode) for _ in range(n)]
    pos, chunks = pkg.simulate.simulate_torch_chunks(I, S, dev, seed=9, n_chrom=nchr,
                                                     chunk_sites=25_000)
    # one pass over the generated blocks feeds all nine handles (begin / sites / end by hand)
    import ctypes as C
    lib = whole.lib
    for h in parts + [whole]:
        h._check(lib.nghmm_load_begin_dev(h._h, C.c_void_p(pos.data_ptr())))
    for s0, c in chunks:
        torch.cuda.synchronize()
        whole._check(lib.nghmm_load_gl_raw_sites_dev(whole._h, int(s0), c.shape[0],
                                                     C.c_void_p(c.data_ptr()), 0, 1, 0))
        for r, h in enumerate(parts):
            cols = c[:, r * I_loc:(r + 1) * I_loc, :].contiguous()
            torch.cuda.synchronize()
            h._check(lib.nghmm_load_gl_raw_sites_dev(h._h, int(s0), c.shape[0],
                                                     C.c_void_p(cols.data_ptr()), 0, 1, 0))
            del cols
        del c
    for h in parts + [whole]:
        h._check(lib.nghmm_load_end(h._h))
        h.set_params(0.1, 0.2, 0.1)
        h.init_emission()
    torch.cuda.empty_cache()
    grp = pkg.Group(parts)                         # site shards from exchanged genotype codes
    free = _iterate_pair(whole, grp, parts, 2, fixed=False, force=True)
    print("config 5 shape (an eighth of the sites), free parameters (teacher-forced):", free)
    assert free["lkl"] < 1e-12 and free["freq"] < 1e-9 and free["indF"] < 1e-4
    for h in parts + [whole]:
        h.set_params(0.3, 0.05, 0.15)
        h.init_emission()
    fix = _iterate_pair(whole, grp, parts, 2, fixed=True, force=False)
    print("config 5 shape, fixed parameters:", fix)
    assert fix["lkl"] < 1e-12 and fix["freq"] < 1e-9
    path_w = whole.viterbi()
    for r in (0, n - 1):
        assert np.array_equal(parts[r].viterbi(), path_w[r * I_loc:(r + 1) * I_loc]), r
    for h in parts + [whole]:
        h.close()


def test_config5_hundred_iterations(pkg):
    """--max_iters 100 --min_iters 99 of configs[4] on one GPU's number of individuals (625,
    25 chromosomes, called genotypes, packed) at 500 000 sites: every array finite and in
    range throughout, the total log-likelihood never drops by more than rounding once the
    first iterations are over, and the run settles."""
    import torch
    I, S, nchr, n_iter = 625, 500_000, 25, 100
    dev = torch.device("cuda", 0)
    h = pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST | pkg.GENO_PACKED)
    pos, chunks = pkg.simulate.simulate_torch_chunks(I, S, dev, seed=11, n_chrom=nchr,
                                                     chunk_sites=50_000)

    def feed():
        for s0, c in chunks:
            torch.cuda.synchronize()
            yield s0, c.shape[0], c.data_ptr()
    h.load_chunks_device(pos.data_ptr(), feed(), space=0, call_geno=True)
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    tot = []
    for it in range(n_iter):
        h.iter_EM()
        tot.append(float(h.ind_lkl.sum()))
        assert np.isfinite(tot[-1]), it
    tot = np.array(tot)
    f, F, A = h.freq, h.indF, h.alpha
    assert np.isfinite(f).all() and (f >= 0).all() and (f < 1).all()
    assert np.isfinite(F).all() and (F >= 1e-15).all() and (F <= 1 - 1e-15).all()
    assert np.isfinite(A).all() and (A >= 1e-15).all() and (A <= 10).all()
    post = h.marg_prob[:4]
    assert ((post >= 0) & (post <= 1)).all()
    rel_step = np.abs(np.diff(tot)) / np.abs(tot[1:])
    print(f"100 iterations of {I} x {S}: total lkl {tot[0]:.3f} -> {tot[-1]:.3f}; relative change "
          f"per iteration after the 20th: max {rel_step[20:].max():.2e}")
    assert tot[-1] > tot[0]
    assert rel_step[20:].max() < 1e-6          # settled
    assert np.diff(tot)[10:].min() > -1e-6 * abs(tot[-1])
    h.close()


def test_bench_four_ranks_on_the_full_workload_reproduce_the_one_gpu_job(pkg):
    """`python bench.py --gpus 4 --workload c3` as the driver starts it: four rank processes,
    the collectives' known-answer preflight, the exchanges of every iteration (gloo through the
    host here: one GPU; nccl = RCCL on a node), and the accounting the scaling line carries --
    in BOTH layouts from one invocation: the site shards the line is about (all 1000 individuals
    for 250 000 sites each, one small all-gather per E-step and objective round) and, embedded as
    `alt_sharding`, the individual shards of BASELINE configs[3]'s wording (250 of the 1000 for
    all 10^6 sites, the all-to-all of posteriors and the all-gather of frequencies).

    Every rank holds a slice of the data set the one-GPU job processes (simulate.IndexedSim), so
    the line's `check` -- two EM iterations from the starting values -- must equal the --gpus 1
    line's: total log-likelihood to 1e-12, frequencies to 1e-9, the same number of L-BFGS-B
    rounds.  The reference's "results do not depend on the number of workers"
    (EM.cpp:151-161,198-201), asserted on the run that is timed."""
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NGHMM_BENCH_BACKEND")}

    def run(*extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c3", "--steps", "2",
               "--warmup", "1", "--full", "--no_cpu_baseline", "--no_exact_line", *extra]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    one = run()
    out = run("--gpus", "4")
    assert one["n_gpus"] == 1 and one["check"]["iterations"] == 2 and len(one["first_iterations_ms"]) == 1
    assert out["n_gpus"] == 4 and out["ranks"] == 4 and out["scaling"] == "strong"
    cfg = out["config"]
    assert cfg["n_ind_total"] == 1000 and cfg["n_sites"] == 1_000_000
    assert out["preflight"]["world"] == 4 and "all_to_all_single float64" in out["preflight"]["checked"]
    assert len(out["per_rank"]) == 4 and sorted(p["rank"] for p in out["per_rank"]) == [0, 1, 2, 3]
    for p in out["per_rank"]:
        assert p["kernel_ms_per_iter"]["lkl_batch"] > 0 and p["kernel_ms_per_iter"]["est_maf"] > 0
    # -- the line's own layout: site shards
    cb = out["collective_bytes_per_iter"]
    assert cfg["n_ind_per_gpu"] == 1000 and cfg["n_sites_per_gpu"] == 250_000
    assert cfg["sharding"].startswith("sites:")
    # <= 5 points x 1000 individuals x 48 B per round and rank, a handful of rounds
    assert cb["all_to_all_out"] == 0 and 0 < cb["all_gather_out"] < 3 * 5e6 and cb["all_gathers"] >= 2
    assert len({p["rounds_per_iter"] for p in out["per_rank"]}) == 1     # the same steps everywhere
    assert out["check"]["rounds_equal_on_all_ranks"] is True
    d = bench.compare_checks(out["check"], one["check"])
    print("sites vs N=1:", json.dumps(d))
    assert d["tot_lkl_max_rel_diff"] <= 1e-12 and d["freq_probe_max_rel_diff"] <= 1e-9
    assert d["freq_weighted_sum_rel_diff"] <= 1e-9 and d["rounds_equal"], d
    assert d["indF_sum_rel_diff"] < 1e-6 and d["alpha_sum_rel_diff"] < 1e-5
    # -- the other layout, same process group, same data set
    alt = out["alt_sharding"]
    assert alt["sharding"] == "individuals" and "skipped" not in alt, alt
    assert alt["n_ind_per_gpu"] == 250 and alt["n_sites_per_gpu"] == 1_000_000 and alt["ms_per_step"] > 0
    acb = alt["collective_bytes_per_iter"]
    assert acb["all_to_all_out"] == 8 * 250_000 * 250 * 3 and acb["all_gather_out"] == 8 * 250_000 * 3
    for p in alt["per_rank"]:
        assert p["exchange_ms_per_iter"]["all_to_all"] > 0
    assert alt["exchange_ms"]["all_to_all"] > 0
    d = bench.compare_checks(alt["check"], one["check"])
    print("individuals vs N=1:", json.dumps(d))
    assert d["tot_lkl_max_rel_diff"] <= 1e-12 and d["freq_probe_max_rel_diff"] <= 1e-9
    assert d["freq_weighted_sum_rel_diff"] <= 1e-9 and d["rounds_equal"], d
    assert alt["vs_main_sharding"]["ok"] is True
    # (the line says at which chain length fast-vs-oracle posteriors hold 1e-9, and that the timed size is beyond it)
    assert out["value"] > 0 and "10^4 sites" in out["parity"]["per_call"] and "NOT" in out["parity"]["per_call"]
    print(json.dumps({k: out[k] for k in ("value", "ms_per_step", "exchange_ms", "collectives")}),
          json.dumps({k: alt[k] for k in ("value", "ms_per_step", "exchange_ms")}))


@pytest.mark.parametrize("ranks,n_sites", [(2, 200_000), (4, 102_400)])
def test_bench_config5_shape_ranks_reproduce_the_one_gpu_job(pkg, ranks, n_sites):
    """BASELINE configs[4]'s shape through bench.py -- 5000 individuals, 25 chromosomes, --call_geno
    (2-bit packed handles, the called genotypes' closed-form frequency step over all 5000) -- at
    200 000 sites on two ranks and at 102 400 on four (whole 16-site code words per rank; gloo on one GPU; a box admits six
    processes on its card and this test process is one of them, so four ranks leave a margin): as
    site shards and, embedded, as individual shards (genotype codes
    exchanged once, posteriors every iteration) the ranks give the one-GPU line's `check` --
    launcher, IndexedSim slicing over the 25 chromosomes (ragged site ranges: 25 chromosomes do
    not split evenly over four ranks' ranges) and the cross-N comparison for the packed layout."""
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NGHMM_BENCH_BACKEND")}

    def run(*extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c5", "--n_sites", str(n_sites),
               "--steps", "2", "--warmup", "1", "--full", "--no_cpu_baseline", *extra]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    one, two = run(), run("--gpus", str(ranks))
    assert "packed" in one["config"]["workload"] and one["config"]["n_ind_total"] == 5000
    assert two["config"]["n_sites_per_gpu"] == n_sites // ranks and two["config"]["sharding"].startswith("sites:")
    assert two["all_gather_rounds"]["calls_per_iteration"] >= 2          # every round's all-gather, side by side
    assert len(two["per_rank"]) == ranks
    alt = two["alt_sharding"]
    assert alt["sharding"] == "individuals" and alt["n_ind_per_gpu"] == 5000 // ranks and "skipped" not in alt
    for name, chk in (("site shards", two["check"]), ("individual shards", alt["check"])):
        d = bench.compare_checks(chk, one["check"])
        print(name, "vs N=1:", json.dumps(d))
        assert d["tot_lkl_max_rel_diff"] <= 1e-12 and d["freq_probe_max_rel_diff"] <= 1e-9
        assert d["freq_weighted_sum_rel_diff"] <= 1e-9 and d["rounds_equal"], d
