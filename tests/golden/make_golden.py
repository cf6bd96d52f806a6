"""Generates tests/golden/*.npz: small seeded inputs and the outputs of the CPU oracle
(both builds; the libm build run with the REFERENCE'S OWN optimizer object from
oracle/_ref when it is available), and (ref_bfgs.npz, which needs that object) what the
reference's optimizer computes on the L-BFGS-B tests' cases.  Run from the repo root:

    python tests/golden/make_golden.py

The reference itself cannot be executed for these routines in this image (GSL is
missing; see oracle/ngsfhmm_oracle.h), so the vectors are the oracle's."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orclib  # noqa: E402

pkg = importlib.import_module("ngsf-hmm_amd")


def em_fixture(name, n_ind, n_sites, iters, **sim):
    d = pkg.simulate.simulate(n_ind, n_sites, **sim)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    out = dict(n_ind=n_ind, n_sites=n_sites, iters=iters, gl=gl, pos_dist=d.pos_dist_mb,
               indF0=np.full(n_ind, 0.1), alpha0=np.full(n_ind, 0.2), freq0=np.full(n_sites, 0.1),
               true_path=d.path)
    for kind in ("libm", "det"):
        orc = orclib.Oracle(kind)
        em = orclib.OracleEM(orc, gl, d.pos_dist_mb)
        em.set_params(out["indF0"], out["alpha0"], out["freq0"])
        if kind == "libm" and orclib.RefBfgs.available():
            em.use_reference_optimizer(orclib.RefBfgs())
        assert em.init_emission() == 0
        out[f"{kind}_eprob0"] = em.e_prob
        for _ in range(iters):
            assert em.iterate() == 0
        out[f"{kind}_indF"] = em.indF
        out[f"{kind}_alpha"] = em.alpha
        out[f"{kind}_freq"] = em.freq
        out[f"{kind}_marg"] = em.marg
        out[f"{kind}_ind_lkl"] = em.ind_lkl
        out[f"{kind}_path"] = em.viterbi()
    path = os.path.join(ROOT, "tests", "golden", name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def ref_bfgs_fixture(name):
    """The reference's own L-BFGS-B object (oracle/_ref/libref_bfgs.so, which oracle/Makefile
    builds where the reference sources are at hand) on the cases of tests/test_lbfgsb_ref.py and
    tests/test_host_logic.py: every evaluation point, final x and return value of the traced
    cases, and on tests/conftest.py's `small_sim` the per-individual optima and three EM
    iterations with it plugged into the oracle."""
    import test_host_logic
    import test_lbfgsb_ref as T
    ref, orc = orclib.RefBfgs(), orclib.Oracle("libm")
    out = {}
    for case, (fn, x0, lb, ub) in T.golden_cases().items():
        x, r, trace = T.run_traced(ref.findmax, fn, x0, lb, ub)
        out.update({case + "_x": x, case + "_r": np.float64(r), case + "_trace": np.array(trace)})
    # tests/conftest.py: small_sim
    d = pkg.simulate.simulate(10, 600, seed=4242, n_chrom=2, missing_rate=0.05, indF="r", alpha=0.5,
                              freq="r")
    gl = pkg.simulate.normalise_log_gl(d.gl)
    out["small_sim_gl_sum"] = np.float64(gl.sum())
    out["hmm_x"], out["hmm_r"], out["hmm_calls"] = T.hmm_objective_runs(ref.findmax, orc, d, gl)
    for k, v in T.em_state(orc, d, gl, ref).items():
        out["em_" + k] = v
    out["batched_x"] = test_host_logic.scalar_runs_from_03_005(orc, ref.findmax, d, gl)
    path = os.path.join(ROOT, "tests", "golden", name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    orclib.build_oracle()
    em_fixture("em_small.npz", 8, 300, 3, seed=2024, n_chrom=2, missing_rate=0.05)
    ref_bfgs_fixture("ref_bfgs.npz")
