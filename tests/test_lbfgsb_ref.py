"""The product's L-BFGS-B core (ngsf-hmm_amd/csrc/lbfgsb.cpp, driven by the oracle's
restatement of findmax_bfgs) against the REFERENCE'S OWN OBJECT CODE: shared/bfgs.cpp
compiled by oracle/Makefile into oracle/_ref/libref_bfgs.so, whose results on the cases
below are stored in tests/golden/ref_bfgs.npz (tests/golden/make_golden.py).

Both are handed the same objective; every point at which the objective is evaluated,
in order, and the final x must agree bit for bit.  This pins SURVEY.md section 8 rows
a8/a9 (findmax_bfgs, getgradient, setulb_ ... dtrsl_)."""
import ctypes as C

import numpy as np
import pytest

from orclib import OBJECTIVE, LklData, _dp, run_findmax


def _traced(fn):
    trace = []

    def cb(xp, _):
        n = cb.n
        x = [xp[i] for i in range(n)]
        trace.append(tuple(x))
        return fn(x)
    return cb, trace


def run_traced(impl, fn, x0, lb, ub):
    """(final x, return value, evaluation points in order) of a findmax_bfgs-shaped `impl`."""
    cb, trace = _traced(fn)
    cb.n = len(x0)
    x, r = run_findmax(impl, OBJECTIVE(cb), x0, lb, ub)
    return x, r, trace


def _against_reference(ref_golden, orc, name):
    """The oracle's optimizer on case `name` against the reference object's stored run."""
    fn, x0, lb, ub = golden_cases()[name]
    xo, ro, to = run_traced(orc.lib.orc_findmax_bfgs, fn, x0, lb, ub)
    tr = ref_golden[name + "_trace"]
    assert len(to) == len(tr) and np.array(to).tobytes() == tr.tobytes(), "evaluation-point traces differ"
    assert xo.tobytes() == ref_golden[name + "_x"].tobytes()
    rr = float(ref_golden[name + "_r"])
    assert (rr == ro) or (np.isnan(rr) and np.isnan(ro))
    return xo, to


def rosen(x):
    return sum(100.0 * (x[i + 1] - x[i] ** 2) ** 2 + (1 - x[i]) ** 2 for i in range(len(x) - 1))


CASES_2D = [
    (rosen, [0.1, 0.2]), (rosen, [0.9, 5.0]), (rosen, [1e-15, 1e-15]),
    (lambda x: np.sin(3 * x[0]) * np.cos(2 * x[1]) + 0.1 * (x[0] - 0.3) ** 2 + 0.05 * (x[1] - 2) ** 2,
     [0.5, 1.0]),
    (lambda x: -np.log(x[0] * (1 - x[0])) + (x[1] - 11) ** 2, [0.2, 3.0]),   # optimum on a bound
    (lambda x: (x[0] - 2) ** 2 + (x[1] + 1) ** 2, [0.5, 0.5]),                 # both bounds active
    (lambda x: abs(x[0] - 0.3) ** 1.5 + abs(x[1] - 0.7) ** 1.5, [0.9, 0.1]),   # non-smooth: long line searches
    (lambda x: 1e6 * (x[0] - 0.5) ** 2 + 1e-6 * (x[1] - 5) ** 2, [0.1, 0.1]),  # badly scaled
]


BOUNDS = [1e-15, 1e-15], [1 - 1e-15, 10.0]           # the bounds of EM.cpp:425-427
WRAP = dict(x0=[-1.2, 1.0, -0.5, 0.8, 0.3, -0.9], lb=[-2.0, -0.5, -1.0, 0.0, -2.0, -2.0],
            ub=[0.9, 2.0, 2.0, 0.7, 2.0, 0.95])


def golden_cases():
    """name -> (objective, x0, lb, ub) of every traced case of this file."""
    cases = {f"box_2d_{k}": (fn, x0) + BOUNDS for k, (fn, x0) in enumerate(CASES_2D)}
    for fixed in (0, 1):
        fn, x0 = CASES_2D[3]
        lb, ub = list(BOUNDS[0]), list(BOUNDS[1])
        lb[fixed] = ub[fixed] = x0[fixed]
        cases[f"fixed_{fixed}"] = (fn, x0, lb, ub)
    cases["memory_wrap"] = (rosen, WRAP["x0"], WRAP["lb"], WRAP["ub"])
    cases["infeasible_start"] = (rosen, [3.0, -4.0], [0.0, 0.0], [2.0, 2.0])
    return cases


@pytest.mark.parametrize("k", range(len(CASES_2D)))
def test_box_2d_bitwise(ref_golden, orc_libm, k):
    _against_reference(ref_golden, orc_libm, f"box_2d_{k}")


@pytest.mark.parametrize("fixed", [0, 1])
def test_fixed_parameter(ref_golden, orc_libm, fixed):
    """--indF_fixed / --alpha_fixed: lower == upper bound (EM.cpp:429-436)."""
    xo, _ = _against_reference(ref_golden, orc_libm, f"fixed_{fixed}")
    assert xo[fixed] == CASES_2D[3][1][fixed]


def test_more_variables_and_memory_wrap(ref_golden, orc_libm):
    """n = 6 Rosenbrock chain: > 10 BFGS updates, so the limited memory wraps
    (iupdat > m branches of matupd_/formk_) and several variables hit bounds."""
    _, to = _against_reference(ref_golden, orc_libm, "memory_wrap")
    assert len(to) > 13 * 20


def test_infeasible_start_is_projected(ref_golden, orc_libm):
    _against_reference(ref_golden, orc_libm, "infeasible_start")


def hmm_objective_runs(impl, orc, d, gl):
    """findmax_bfgs on the real objective, every individual of `d` from (0.1, 0.2): final
    (indF, alpha) [I][2], return values [I] and forward-pass counts [I]."""
    import orclib
    em = orclib.OracleEM(orc, gl, d.pos_dist_mb)
    em.set_params(0.1, 0.2, 0.1)
    assert em.init_emission() == 0
    e = em.e_prob
    pos = np.ascontiguousarray(d.pos_dist_mb)
    xs, rs, calls = np.empty((d.n_ind, 2)), np.empty(d.n_ind), np.empty(d.n_ind)
    for i in range(d.n_ind):
        ei = np.ascontiguousarray(e[i])
        data = LklData(_dp(ei), _dp(pos), d.n_sites, 0, 0)
        xs[i], rs[i] = run_findmax(impl, C.cast(orc.lib.orc_lkl, C.c_void_p), [0.1, 0.2],
                                   [1e-15, 1e-15], [1 - 1e-15, 10.0], C.cast(C.byref(data), C.c_void_p))
        calls[i] = data.n_calls
    return xs, rs, calls


def em_state(orc, d, gl, ref_bfgs=None):
    """Three whole EM iterations of the oracle from (0.1, 0.2, 0.1), with the reference's
    optimizer object plugged in when one is given."""
    import orclib
    em = orclib.OracleEM(orc, gl, d.pos_dist_mb)
    em.set_params(0.1, 0.2, 0.1)
    if ref_bfgs is not None:
        em.use_reference_optimizer(ref_bfgs)
    em.init_emission()
    for _ in range(3):
        assert em.iterate() == 0
    return dict(indF=em.indF, alpha=em.alpha, freq=em.freq, marg=em.marg, ind_lkl=em.ind_lkl,
                lkl_calls=np.float64(em.lkl_calls))


def test_hmm_objective_bitwise(ref_golden, orc_libm, small_sim):
    """The real objective (EM.cpp:449-464) on simulated data: same forward-pass
    count and the same (indF, alpha) to the last bit, for every individual."""
    d, gl = small_sim
    assert gl.sum() == ref_golden["small_sim_gl_sum"]         # the data the reference ran on
    xs, rs, calls = hmm_objective_runs(orc_libm.lib.orc_findmax_bfgs, orc_libm, d, gl)
    for i in range(d.n_ind):
        assert (xs[i].tobytes(), rs[i], calls[i]) == (ref_golden["hmm_x"][i].tobytes(),
                                                      ref_golden["hmm_r"][i], ref_golden["hmm_calls"][i])


def test_em_with_reference_optimizer_identical(ref_golden, orc_libm, small_sim):
    """Three whole EM iterations of the oracle with the reference's optimizer object
    plugged in give bit-identical state to the oracle with the restated optimizer."""
    d, gl = small_sim
    assert gl.sum() == ref_golden["small_sim_gl_sum"]
    for name, v in em_state(orc_libm, d, gl).items():
        assert np.asarray(v).tobytes() == ref_golden["em_" + name].tobytes(), name
