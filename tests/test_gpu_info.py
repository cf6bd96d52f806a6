"""Observed information on the device (nghmm_obs_info / nghmm_chain_obs_info, include/nghmm.h)
against the 50-digit mpmath evaluation of tests/info_util.py under the handle's own emissions:
every field of every individual of every case within the bounds stated there (lkl 1e-12 |l|,
gradient 1e-9 (|g| + |h_kk| x_k), Hessian 1e-9 max(|h_kl|, sqrt|h_kk h_ll|)); lkl against
nghmm_lkl_batch; identical bits on a second call; chains of 2 and 3 shards against one handle;
nothing else moves; the error paths; the host's --indF_se against obs_info + std_errors.
Each comparison prints its worst |error| / bound per field before it asserts (run with -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import cli_util
import info_util as iu
from conftest import has_gpu
from layout_util import forced_layout

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def _data(pkg, n_ind, n_sites, seed):
    d = pkg.simulate.simulate(n_ind, n_sites, seed=seed, n_chrom=3 if n_sites > 20 else 1, indF="r",
                              alpha="r", missing_rate=0.05)
    rng = np.random.default_rng(seed + 1)
    return d, rng.uniform(0.02, 0.9, n_ind), rng.uniform(0.01, 2.0, n_ind)


def _handle(pkg, d, pos, F, A, mode, packed=False, iters=2, fast_c=None):
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | (pkg.GENO_PACKED if packed else 0)
    with forced_layout(fast_c):
        h = pkg.NgsFHMM(d.n_ind, d.n_sites, mode=m)
    if packed:
        h.load_raw(d.gl, pos, space=0, call_geno=True)
    else:
        h.load(pkg.simulate.normalise_log_gl(d.gl), pos)
    h.set_params(F, A, 0.15)
    h.init_emission()
    for _ in range(iters):
        h.iter_EM()
    return h


def _far_points(n_ind):
    """Caller-supplied points far from the optimum, F = 1e-15 and alpha = 10 among them."""
    pts = [(1e-15, 10.0), (1e-15, 0.3), (0.5, 10.0), (0.97, 1e-3), (0.3, 4.0)]
    F = np.array([pts[i % len(pts)][0] for i in range(n_ind)])
    A = np.array([pts[i % len(pts)][1] for i in range(n_ind)])
    return F, A


# (individuals, sites, mode, packed, waves per individual, EM iterations, seed)
# The reference evaluates under the emissions the handle EXPORTS (rounded logarithms), the device
# under the ratios it holds: inputs that agree to 1e-16, so every case must be conditioned well
# below 1e7 with respect to its emissions.  Seven sites are not: EM runs their parameters into
# the bounds and their frequencies to the floor, where e1 / e0 - 1 ~ 1e-8 and the alpha-derivatives
# are that difference times 1e-15 -- the exported logarithms do not determine them to 1e-9.  The
# seven-site case therefore takes the parameters as set (no EM iteration); the others run two.
CASES = [
    (5, 5003, "fast", False, None, 2, 11),     # the layout's own C (4 waves, lane-chunks of 24 sites)
    (3, 2500, "fast", False, 2, 2, 12),        # fast_c = 2
    (4, 1500, "fast", True, None, 2, 13),      # packed handle (called genotypes); C = 1
    (3, 7, "fast", False, None, 0, 14),        # fewer sites than lane-chunks; C = 1
    (5, 1201, "exact", False, None, 2, 15),
]


@pytest.mark.parametrize("n_ind,n_sites,mode,packed,fast_c,iters,seed", CASES)
def test_records_match_the_50_digit_reference(pkg, n_ind, n_sites, mode, packed, fast_c, iters, seed):
    d, F0, A0 = _data(pkg, n_ind, n_sites, seed)
    pos = d.pos_dist_mb.copy()
    if mode == "fast" and n_sites > 100:
        # chromosome starts at a lane-chunk boundary, two adjacent ones and, with more than one
        # wave per individual, one at a wave-chunk boundary (the first site of wave 1).  More than
        # 64 waves per individual (k_info_finish with K > 1 chunks per lane) need more sites than
        # the per-call contract covers: no case here reaches that branch.
        with _handle(pkg, d, pos, F0, A0, mode, packed, iters=0, fast_c=fast_c) as probe:
            c_waves, T = probe.layout()
        assert c_waves == (fast_c or c_waves) and T * 3 + 2 < n_sites
        pos[3 * T] = np.inf
        pos[5 * T + 3] = pos[5 * T + 4] = np.inf
        if c_waves > 1:
            assert 64 * T < n_sites
            pos[64 * T] = np.inf
    with _handle(pkg, d, pos, F0, A0, mode, packed, iters=iters, fast_c=fast_c) as h:
        if mode == "fast":
            print(f"\n  layout (C, T) = {h.layout()}")
        le = h.e_prob
        # the current parameters: near the optimum after two EM iterations
        F, A = h.indF, h.alpha
        got = h.obs_info()
        assert got.dtype == pkg.INFO_DTYPE and got.shape == (n_ind,)
        iu.check_records(got, iu.ref_records(le, pos, F, A), F, A, label=f"{mode} current")
        again = h.obs_info()
        assert again.tobytes() == got.tobytes()
        assert h.obs_info(F, A).tobytes() == got.tobytes()
        lk = h.lkl(np.arange(n_ind), F, A)
        assert np.all(np.abs(got["lkl"] - lk) <= 1e-12 * np.abs(lk))
        # far from it
        F, A = _far_points(n_ind)
        got = h.obs_info(F, A)
        iu.check_records(got, iu.ref_records(le, pos, F, A), F, A, label=f"{mode} far")
        assert h.obs_info(F, A).tobytes() == got.tobytes()
        lk = h.lkl(np.arange(n_ind), F, A)
        assert np.all(np.abs(got["lkl"] - lk) <= 1e-12 * np.abs(lk))


def test_chains_of_two_and_three_shards_equal_one_handle(pkg):
    n_ind, S = 3, 2400
    d, F, A = _data(pkg, n_ind, S, 21)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    pos = d.pos_dist_mb
    chrom = int(np.flatnonzero(np.isinf(pos))[1])

    def make(lo, hi):
        h = pkg.NgsFHMM(n_ind, hi - lo, mode=pkg.MODE_FAST)
        h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(pos[lo:hi]))
        h.set_params(F, A, 0.15)
        h.init_emission()
        return h

    for cuts in ([0, 1003, S], [0, 603, chrom, S]):     # (a shard boundary that is a chromosome start)
        hs = [make(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
        whole = make(0, S)
        try:
            ch = pkg.Chain(hs)
            for _ in range(2):
                ch.iter_EM()
            Fc, Ac = hs[0].indF, hs[0].alpha
            whole.set_params(Fc, Ac, ch.freq)
            le = whole.e_prob
            for pF, pA in ((None, None), _far_points(n_ind)):
                got = ch.obs_info(pF, pA)
                one = whole.obs_info(pF, pA)
                xF, xA = (Fc, Ac) if pF is None else (pF, pA)
                ref = iu.ref_records(le, pos, xF, xA)
                iu.check_records(got, ref, xF, xA, label=f"chain of {len(hs)}")
                iu.check_records(one, ref, xF, xA, label="one handle")
                assert ch.obs_info(pF, pA).tobytes() == got.tobytes()
            # without nghmm_chain_setup
            arr = (C.c_void_p * 2)(hs[0].handle, whole.handle)
            out = np.zeros(n_ind, dtype=pkg.INFO_DTYPE)
            assert whole.lib.nghmm_chain_obs_info(arr, 2, None, None, C.c_void_p(out.ctypes.data)) == -10
        finally:
            for h in hs:
                h.close()
            whole.close()


@pytest.mark.parametrize("decode", [True, False])
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_nothing_else_moves(pkg, mode, decode):
    """With a Viterbi decode before the call (which has refreshed the emissions) and without one
    (the call is the first after iter_EM's new frequencies and refreshes them itself)."""
    d, F, A = _data(pkg, 20, 2000, 8)
    with _handle(pkg, d, d.pos_dist_mb, F, A, mode) as a, _handle(pkg, d, d.pos_dist_mb, F, A, mode) as b:
        if decode:
            for h in (a, b):
                h.viterbi()
        a.obs_info()
        a.obs_info(*_far_points(20))
        for f in ("indF", "alpha", "freq", "marg_prob"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
        if decode:
            assert a.ibd_tracts("viterbi").tobytes() == b.ibd_tracts("viterbi").tobytes()
        for h in (a, b):
            h.iter_EM()
        for f in ("indF", "alpha", "freq", "marg_prob", "ind_lkl"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_argument_errors(pkg):
    d, F, A = _data(pkg, 4, 200, 3)
    dp = C.POINTER(C.c_double)
    out = np.zeros(4, dtype=pkg.INFO_DTYPE)
    po = C.c_void_p(out.ctypes.data)
    with pkg.NgsFHMM(4, 200, mode=pkg.MODE_FAST) as h:
        with pytest.raises(pkg.NgsFHMMError) as ei:         # no data loaded
            h.obs_info()
        assert ei.value.code == -10 and "no data" in ei.value.message
        h.load(pkg.simulate.normalise_log_gl(d.gl), d.pos_dist_mb)
        h.set_params(F, A, 0.15)
        h.init_emission()
        L = h.lib
        assert L.nghmm_obs_info(h.handle, F.ctypes.data_as(dp), None, po) == -10     # exactly one NULL
        assert L.nghmm_obs_info(h.handle, None, A.ctypes.data_as(dp), po) == -10
        assert L.nghmm_obs_info(h.handle, None, None, None) == -10
        assert L.nghmm_obs_info(None, None, None, po) == -10
        assert L.nghmm_chain_obs_info(None, 1, None, None, po) == -10
        assert L.nghmm_last_error() != b""
        for bad_F, bad_A in ((0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 10.5), (np.nan, 0.5), (0.5, np.nan),
                             (-0.1, 0.5), (0.5, np.inf)):
            pF, pA = F.copy(), A.copy()
            pF[2], pA[2] = bad_F, bad_A
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.obs_info(pF, pA)
            assert ei.value.code == -10 and "individual 2" in ei.value.message
        h.obs_info(np.full(4, 1 - 1e-15), np.full(4, 1e-15))       # the box's corners are inside
        h.obs_info(1e-15, 10.0)


@pytest.mark.parametrize("tag,extra", [
    ("exact", ["--mode", "exact"]),
    ("chain", ["--mode", "fast", "--n_gpus", 2, "--devices", "0,0"]),
])
def test_cli_indF_se(pkg, tmp_path, tag, extra):
    """ngsF-HMM --indF_se: the numbers of PREFIX.indF.se are obs_info + std_errors from Python on
    the same data at the run's final parameters and frequencies -- a run with all three held fixed
    (--indF_fixed --alpha_fixed --freq_est 0), so that Python has them exactly.  The file prints 10
    significant digits (5e-10 relative) and the two evaluations may differ by the per-call contract
    (1e-9): lkl, the standard errors and the correlation within 2e-9 relative, the gradient within
    2e-9 (|g| + |h_kk| x_k).  The other output files do not change."""
    I, S = 6, 2001
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=3, indF=0.4, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--freq_est", 0, "--indF", "0.4,0.05", "--indF_fixed", "--alpha_fixed",
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0] + extra
    plain, a = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"a_{tag}")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a, "--indF_se"])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".indF.se")
    lines = open(a + ".indF.se").read().split("\n")
    assert lines[0].split("\t") == ["ind", "indF", "se_indF", "alpha", "se_alpha", "corr", "lkl",
                                    "grad_indF", "grad_alpha"]
    assert lines[-1] == "" and len(lines) == I + 2
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == [f"ind{i}" for i in range(I)]
    tab = np.array([[np.nan if x == "NA" else float(x) for x in r[1:]] for r in rows])
    F, A = np.full(I, 0.4), np.full(I, 0.05)
    assert np.array_equal(tab[:, 0], F) and np.array_equal(tab[:, 2], A)
    mode = pkg.MODE_EXACT if tag == "exact" else pkg.MODE_FAST
    with pkg.NgsFHMM(I, S, mode=mode) as h:
        h.load_raw(d.gl, d.pos_dist_mb, space=0)
        h.set_params(F, A, 0.1)
        h.init_emission()
        info = h.obs_info()
    se_F, se_A, corr = pkg.std_errors(info, F, A)
    print("\n  se_indF", se_F, "\n  se_alpha", se_A, "\n  corr", corr)
    assert np.isfinite(se_F).sum() >= I // 2            # (records that are mostly NA show nothing)
    for col, want, tol in ((1, se_F, 2e-9), (3, se_A, 2e-9), (4, corr, 2e-9), (5, info["lkl"], 2e-9)):
        assert np.array_equal(np.isnan(tab[:, col]), np.isnan(want)), col
        ok = ~np.isnan(want)
        assert np.all(np.abs(tab[ok, col] - want[ok]) <= tol * np.abs(want[ok])), (col, tab[:, col], want)
    assert np.all(np.abs(tab[:, 6] - info["g_F"]) <= 2e-9 * (np.abs(info["g_F"]) + np.abs(info["h_FF"]) * F))
    assert np.all(np.abs(tab[:, 7] - info["g_A"]) <= 2e-9 * (np.abs(info["g_A"]) + np.abs(info["h_AA"]) * A))
