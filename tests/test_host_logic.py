"""Host-side logic of the product that needs no GPU: the lock-step batched L-BFGS-B
(ngsf-hmm_amd/csrc/bfgs_batch.cpp) must reproduce, per individual, exactly what the
reference's blocking findmax_bfgs does with the same objective -- same final
(indF, alpha) to the last bit and the same count of forward passes -- and the
simulator must produce well-formed inputs."""
import ctypes as C
import importlib
import json
import math

import numpy as np
import pytest

import orclib
from orclib import LklData, _dp, run_findmax


def _scalar_findmax(orc, impl, e_i, pos, x0, fixed=(False, False)):
    lb, ub = [1 / 1e15, 1 / 1e15], [1 - 1 / 1e15, 10.0]
    for k in range(2):
        if fixed[k]:
            lb[k] = ub[k] = x0[k]
    ei = np.ascontiguousarray(e_i)
    data = LklData(_dp(ei), _dp(pos), len(pos), 0, 0)
    x, _ = run_findmax(impl, C.cast(orc.lib.orc_lkl, C.c_void_p), x0, lb, ub,
                       C.cast(C.byref(data), C.c_void_p))
    return x, data.n_calls


@pytest.mark.parametrize("fixed", [(False, False), (True, False), (False, True)])
def test_batched_bfgs_equals_blocking_findmax(pkg, orc_libm, small_sim, fixed):
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    d, gl = small_sim
    em = orclib.OracleEM(orc_libm, gl, d.pos_dist_mb)
    em.set_params(0.1, 0.2, 0.1)
    em.init_emission()
    e = em.e_prob
    pos = np.ascontiguousarray(d.pos_dist_mb)
    x0F = np.linspace(0.05, 0.9, d.n_ind)
    x0A = np.linspace(0.01, 2.0, d.n_ind)

    def objective(i, F, a):          # forward log-likelihood (EM.cpp:463 returns its negative)
        return -orc_libm.lkl([F, a], e[i], pos)

    F, A, st = hm.bfgs_batch_host(x0F, x0A, objective, indF_fixed=fixed[0], alpha_fixed=fixed[1])
    calls = 0
    for i in range(d.n_ind):
        x, n = _scalar_findmax(orc_libm, orc_libm.lib.orc_findmax_bfgs, e[i], pos,
                               [x0F[i], x0A[i]], fixed)
        assert x[0] == F[i] and x[1] == A[i], f"individual {i}"
        calls += n
    assert st.ref_forward_calls == calls
    assert st.points < calls          # duplicates and fixed-parameter probes are not re-evaluated
    assert st.rounds >= 2


def scalar_runs_from_03_005(orc, impl, d, gl):
    """A blocking findmax_bfgs `impl` per individual of `d` from (0.3, 0.05), the emissions of
    (0.3, 0.05, 0.2): final (indF, alpha) [I][2]."""
    em = orclib.OracleEM(orc, gl, d.pos_dist_mb)
    em.set_params(0.3, 0.05, 0.2)
    em.init_emission()
    e = em.e_prob
    pos = np.ascontiguousarray(d.pos_dist_mb)
    return np.array([_scalar_findmax(orc, impl, e[i], pos, [0.3, 0.05])[0] for i in range(d.n_ind)])


def test_batched_bfgs_against_reference_object(pkg, orc_libm, ref_golden, small_sim):
    """Same, against the reference's own compiled findmax_bfgs (its results on this data:
    tests/golden/ref_bfgs.npz, tests/golden/make_golden.py)."""
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    d, gl = small_sim
    assert gl.sum() == ref_golden["small_sim_gl_sum"]         # the data the reference ran on
    em = orclib.OracleEM(orc_libm, gl, d.pos_dist_mb)
    em.set_params(0.3, 0.05, 0.2)
    em.init_emission()
    e = em.e_prob
    pos = np.ascontiguousarray(d.pos_dist_mb)
    x0F = np.full(d.n_ind, 0.3)
    x0A = np.full(d.n_ind, 0.05)
    F, A, st = hm.bfgs_batch_host(x0F, x0A, lambda i, f, a: -orc_libm.lkl([f, a], e[i], pos))
    x = ref_golden["batched_x"]
    for i in range(d.n_ind):
        assert x[i, 0] == F[i] and x[i, 1] == A[i]


@pytest.mark.parametrize("fixed", [(False, False), (True, False), (False, True)])
def test_device_solver_type_takes_the_host_machines_steps(pkg, orc_libm, small_sim, fixed):
    """The solver the GPU runs between two objective rounds (kernels_bfgs.hip: LbfgsbT<PtrStore>,
    lbfgsb_core.hpp, around bfgs_problem.hpp's plan / consume) is the same code as the host's
    class Lbfgsb over other storage.  Here both on the CPU, on the real objective and on a
    rough one that drives the line search into its safeguards and the memory around its ring:
    same final (indF, alpha) to the last bit, same number of rounds, points and reference
    forward calls -- with libm's pow (exact mode's) and with detmath's (fast mode's)."""
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    d, gl = small_sim
    em = orclib.OracleEM(orc_libm, gl, d.pos_dist_mb)
    em.set_params(0.1, 0.2, 0.1)
    em.init_emission()
    e = em.e_prob
    pos = np.ascontiguousarray(d.pos_dist_mb)
    x0F = np.linspace(0.05, 0.9, d.n_ind)
    x0A = np.linspace(0.01, 2.0, d.n_ind)

    def real(i, F, a):
        return -orc_libm.lkl([F, a], e[i], pos)

    def rough(i, F, a):     # many iterations: a curved valley with a ripple on it
        return -(100.0 * (a - 3.0 * F * F) ** 2 + (0.7 - F) ** 2 + 1e-3 * math.sin(40.0 * F + i))

    for objective in (real, rough):
        for det in (False, True):
            Fh, Ah, sh = hm.bfgs_batch_host(x0F, x0A, objective, fixed[0], fixed[1], det_pow=det)
            Fd, Ad, sd = hm.bfgs_batch_host(x0F, x0A, objective, fixed[0], fixed[1], det_pow=det,
                                            device_solver=True)
            assert np.array_equal(Fh, Fd) and np.array_equal(Ah, Ad)
            assert (sh.rounds, sh.points, sh.ref_forward_calls, sh.ind_rounds) == \
                   (sd.rounds, sd.points, sd.ref_forward_calls, sd.ind_rounds)
        # libm's pow and detmath's differ by at most a few ulp in the step: the same optimum
        Fl, Al, _ = hm.bfgs_batch_host(x0F, x0A, objective, fixed[0], fixed[1], det_pow=False)
        np.testing.assert_allclose(Fd, Fl, atol=2e-4)
    # and without flags the entry point is the round-1..4 one
    F0, A0, s0 = hm.bfgs_batch_host(x0F, x0A, rough, fixed[0], fixed[1])
    assert np.array_equal(F0, Fl) and np.array_equal(A0, Al)
    assert sd.rounds >= 10 if not any(fixed) else sd.rounds >= 2


def test_nonfinite_parameters_take_the_reference_branch(pkg):
    """EM.cpp:454-456: NaN/Inf parameters make the objective -1e15 without a forward pass."""
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    seen = []

    def objective(i, F, a):
        seen.append((F, a))
        return -((F - 0.4) ** 2 + (a - 2.0) ** 2)
    F, A, st = hm.bfgs_batch_host([0.2], [1.0], objective)
    assert all(math.isfinite(f) and math.isfinite(a) for f, a in seen)
    assert abs(F[0] - 0.4) < 1e-3 and abs(A[0] - 2.0) < 1e-3


def test_both_fixed_is_a_no_op(pkg):
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    F, A, st = hm.bfgs_batch_host([0.2, 0.3], [1.0, 2.0], lambda i, f, a: 0.0, True, True)
    assert F.tolist() == [0.2, 0.3] and A.tolist() == [1.0, 2.0] and st.rounds == 0


def test_simulator_shapes_and_model(pkg):
    sim = pkg.simulate
    d = sim.simulate(7, 500, seed=3, n_chrom=3, missing_rate=0.1)
    assert d.gl.shape == (500, 7, 3) and d.path.shape == (7, 500) and d.geno.shape == (500, 7)
    np.testing.assert_allclose(np.exp(d.gl).sum(axis=2), 1.0, atol=1e-8)   # rounded to 10 decimals
    assert np.isinf(d.pos_dist_mb).sum() == 2                              # two chromosome changes
    assert d.pos_dist_mb[0] == d.pos[0] / 1e6                              # first site: absolute position
    assert np.all(d.pos_dist_mb[np.isfinite(d.pos_dist_mb)] >= 1e-6)
    gl = sim.normalise_log_gl(d.gl)
    np.testing.assert_allclose(np.exp(gl).sum(axis=2), 1.0, atol=1e-12)
    cg = sim.called_genotype_gl(d.geno)
    assert cg.shape == d.gl.shape and np.all(cg.max(axis=2) == 0.0)
    # IBD sites are homozygous
    assert np.all(d.geno.T[d.path == 1] != 1)
    # same seed, same data
    d2 = sim.simulate(7, 500, seed=3, n_chrom=3, missing_rate=0.1)
    assert np.array_equal(d.gl, d2.gl) and np.array_equal(d.path, d2.path)


def test_indexed_simulator_slices_are_slices_of_the_whole(pkg):
    """simulate.IndexedSim (what bench.py generates its data with): every random field is a hash
    of the GLOBAL (individual, site) indices and the IBD chain is resumed exactly by looking back
    to its last redraw site, so any (individual range) x (site range) slice, generated in chunks
    of any size, is bit for bit the slice of the whole data set -- the N-rank benchmark job holds
    pieces of the one-GPU job's data whatever the sharding (EM.cpp:151-161: results do not depend
    on the number of workers).  On the CPU device here; element-wise torch operations only."""
    import torch
    dev = torch.device("cpu")
    I, S = 18, 3000
    for kw in (dict(n_chrom=3), dict(n_chrom=1, freq="r", indF="r", alpha="r"), dict(alpha=1e-4)):
        whole = pkg.simulate.IndexedSim(I, S, dev, seed=77, **kw)
        full, pd = whole.gl(chunk_sites=1111), whole.pos_dist(0, S)
        assert full.shape == (S, I, 3) and torch.isfinite(full).all()
        assert torch.allclose(torch.exp(full).sum(-1), torch.ones(S, I, dtype=torch.float64), atol=1e-12)
        assert int(torch.isinf(pd).sum()) == kw.get("n_chrom", 1) - 1
        for i0, i1, s0, s1, cs in ((0, I, 0, S, S), (0, I, 1024, 2048, 333), (5, 11, 0, S, 777),
                                   (12, 18, 1776, S, 100), (3, 4, S - 1, S, 7), (0, 9, 16, 17, 1)):
            part = pkg.simulate.IndexedSim(I, S, dev, seed=77, **kw)
            part.LOOKBACK = 32          # the look-back recursion itself (alpha = 1e-4: long tracts)
            sl = part.gl((i0, i1), (s0, s1), chunk_sites=cs)
            assert torch.equal(sl, full[s0:s1, i0:i1]), (kw, i0, i1, s0, s1)
            assert torch.equal(part.pos_dist(s0, s1), pd[s0:s1])
    other = pkg.simulate.IndexedSim(I, S, dev, seed=78, n_chrom=3).gl()
    assert not torch.equal(other, pkg.simulate.IndexedSim(I, S, dev, seed=77, n_chrom=3).gl())
    # the data model: depth ~ Poisson(2) (13.5 % uniform cells), allele frequency 0.2
    big = torch.exp(pkg.simulate.IndexedSim(200, 20000, dev, seed=5).gl())
    uniform = ((big - 1.0 / 3).abs().amax(-1) < 1e-6).double().mean().item()
    assert abs(uniform - math.exp(-2.0)) < 2e-3
    assert abs(big[..., 0].mean().item() - 0.561) < 5e-3


def test_bench_check_comparison():
    """bench.compare_checks: what decides that an N-rank line reproduces the one-GPU line."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    a = {"tot_lkl": [-9.0e8, -8.5e8], "rounds": [18, 11], "freq_probes": [0.2, 0.19], "freq_sum": 2e5,
         "freq_weighted_sum": 1e5, "indF_sum": 499.0, "alpha_sum": 10.0}
    assert bench.compare_checks(a, a)["ok"] is True
    b = dict(a, tot_lkl=[-9.0e8 * (1 + 5e-13), -8.5e8])
    assert bench.compare_checks(b, a)["ok"] is True            # 1e-12 on the log-likelihoods
    assert bench.compare_checks(dict(a, tot_lkl=[-9.0e8 * (1 + 5e-12), -8.5e8]), a)["ok"] is False
    assert bench.compare_checks(dict(a, freq_probes=[0.2 * (1 + 5e-9), 0.19]), a)["ok"] is False
    assert bench.compare_checks(dict(a, rounds=[18, 12]), a)["ok"] is False
    ref = json.load(open(bench.CHECK_REF))                     # the committed one-GPU reference
    key = "c3:fast:1000x1000000:gl"
    assert key in ref and ref[key]["iterations"] == 2 and len(ref[key]["freq_probes"]) == 16


def test_bench_shard_shapes_cover_the_job_exactly_once(pkg):
    """bench.shard_shapes: what every rank of an N-rank job holds under either layout -- the
    ranks' slices of IndexedSim(I_tot, S_job) tile the one-GPU job's data set exactly (strong
    scaling), or N times the workload (weak), and a size that does not divide is refused."""
    import importlib
    import os
    import sys
    import types
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    dd = importlib.import_module("ngsf-hmm_amd.distributed")

    def shapes(world, shard, scaling="strong", I=1000, S=1_000_000, V=1, call_geno=False):
        out = []
        for rank in range(world):
            ctx = types.SimpleNamespace(
                args=types.SimpleNamespace(emulate_ranks=V, scaling=scaling, workload="c3"),
                wl=dict(n_ind=I, n_sites=S), world=world, rank=rank, dd=dd, call_geno=call_geno)
            out.append(bench.shard_shapes(ctx, shard))
        return out

    for world in (1, 2, 4, 8):
        for shard in ("sites", "individuals"):
            sh = shapes(world, shard if world > 1 else None)
            assert all(s["I_tot"] == 1000 and s["S_job"] == 1_000_000 for s in sh)
            for s in sh:
                (i0, i1), (s0, s1) = s["ind_range"], s["site_range"]
                assert s["I"] == i1 - i0 and s["S"] == s1 - s0 and s["I"] > 0 and s["S"] > 0
            if shard == "sites" and world > 1:      # contiguous site ranges, all individuals each
                assert [s["ind_range"] for s in sh] == [(0, 1000)] * world
                cuts = [s["site_range"] for s in sh]
                assert cuts[0][0] == 0 and cuts[-1][1] == 1_000_000
                assert all(a[1] == b[0] for a, b in zip(cuts[:-1], cuts[1:]))
            else:                                   # contiguous individual ranges, all sites each
                assert [s["site_range"] for s in sh] == [(0, 1_000_000)] * world
                cuts = [s["ind_range"] for s in sh]
                assert cuts[0][0] == 0 and cuts[-1][1] == 1000
                assert all(a[1] == b[0] for a, b in zip(cuts[:-1], cuts[1:]))
    weak = shapes(4, "sites", "weak")
    assert weak[0]["S_job"] == 4_000_000 and weak[3]["site_range"][1] == 4_000_000 and weak[0]["I"] == 1000
    weak = shapes(4, "individuals", "weak")
    assert weak[0]["I_tot"] == 4000 and weak[3]["ind_range"] == (3000, 4000) and weak[0]["S"] == 1_000_000
    with pytest.raises(ValueError):
        shapes(2, "individuals", I=63, S=20_000)
    with pytest.raises(ValueError):                          # 5000 x 5M unpacked does not fit one GPU
        shapes(1, None, I=5000, S=5_000_000)
    assert abs(shapes(8, "sites", I=5000, S=5_000_000, call_geno=True)[0]["S"] - 625_000) <= 16
    # an emulated rank of eight: the first range of eight, not an eighth of one rank's
    em = shapes(1, "sites", V=8)[0]
    assert em["site_range"][0] == 0 and abs(em["S"] - 125_000) <= 16 and em["S_job"] == 1_000_000
