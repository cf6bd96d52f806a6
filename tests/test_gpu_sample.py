"""IBD paths sampled on the device (nghmm_sample_paths / nghmm_chain_sample_paths,
include/nghmm.h) against the sequential restatement of tests/sample_util.py from the same random
numbers: the same paths bit for bit, the records against numpy on the returned paths, independence
from how the call is made, a chain of site shards against one handle, and the sample means
against the E-step's posteriors.

Bit-for-bit equality needs a precondition ON THE INPUT: a device forward vector differs from the
restatement's in the last bits, so a site whose u lies within tol of its threshold n1 / (n0 + n1)
may fall either way, and everything to its left with it.  Every comparison therefore first
asserts, from the restatement alone, that no (draw, individual, site, l) lies within tol (1e-9 in
fast mode, 1e-8 in exact mode), and then demands equality everywhere.  The seeds below are fixed;
the smallest |u - p| each met is printed by the test (run with -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cli_util
import sample_util as su
from conftest import has_gpu
from test_sample_cpu import check_calibration

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

TOL = {"fast": 1e-9, "exact": 1e-8}


def _data(pkg, n_ind, n_sites, seed, packed=False):
    n_chrom = 3 if n_sites >= 900 else (2 if n_sites > 20 else 1)
    d = pkg.simulate.simulate(n_ind, n_sites, seed=seed, n_chrom=n_chrom, indF="r", alpha="r",
                              missing_rate=0.03)
    rng = np.random.default_rng(seed + 1)
    F, A = rng.uniform(0.02, 0.95, n_ind), rng.uniform(0.01, 2.0, n_ind)
    return d, F, A


def _handle(pkg, d, F, A, mode, packed=False, iters=2):
    m = (pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) | (pkg.GENO_PACKED if packed else 0)
    h = pkg.NgsFHMM(d.n_ind, d.n_sites, mode=m)
    if packed:
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=True)
    else:
        h.load(pkg.simulate.normalise_log_gl(d.gl), d.pos_dist_mb)
    h.set_params(F, A, 0.15)
    h.init_emission()
    for _ in range(iters):
        h.iter_EM()
    return h


def _restate(h, pos, seed, draws, tol, site0=0):
    """(paths, smallest |u - p|) of the restatement at the handle's current parameters."""
    e = h.e_prob
    F, A = h.indF, h.alpha
    a = su.forward_filter(e, pos, F, A)
    thr = su.thresholds(a, pos, F, A)
    u = su.uniforms(seed, draws, h.n_ind, h.n_sites, site0)
    margin = su.min_margin(thr, u)
    print(f"\n  {h.n_ind} x {h.n_sites}: smallest |u - p| = {margin:.3e} (tol {tol:g})")
    assert margin > tol, "a fragile cell: choose another seed"
    return su.backward_draw(thr, u), margin


def _check_stats(stats, paths, pos):
    want = su.path_stats(paths, pos)
    for f in ("ibd_sites", "n_tracts", "longest_sites"):
        np.testing.assert_array_equal(stats[f][:len(paths)], want[f], err_msg=f)
    np.testing.assert_allclose(stats["ibd_mb"][:len(paths)], want["ibd_mb"], rtol=1e-12, atol=0)


# seed: fixed per shape, each the first one tried; the smallest |u - p| it met on an MI355X
@pytest.mark.parametrize("n_ind,n_sites,mode,packed,seed", [
    (70, 5003, "fast", False, 101),       # 1.804e-07
    (1, 900, "fast", False, 102),         # 6.341e-05
    (5, 10, "fast", False, 103),          # 3.078e-03
    (64, 16, "fast", False, 104),         # 1.478e-05
    (64, 100000, "fast", False, 105),     # 1.781e-08
    (33, 2500, "fast", True, 106),        # 8.367e-07 (packed)
    (3, 7, "exact", False, 107),          # 4.941e-03
    (130, 4099, "exact", False, 108),     # 9.362e-08
])
def test_paths_equal_the_restatement_bit_for_bit(pkg, n_ind, n_sites, mode, packed, seed):
    d, F, A = _data(pkg, n_ind, n_sites, seed)
    with _handle(pkg, d, F, A, mode, packed) as h:
        want, _ = _restate(h, d.pos_dist_mb, seed, range(4), TOL[mode])
        stats, paths = h.sample_paths(4, seed=seed, keep=4)
        assert paths.shape == (4, n_ind, n_sites) and stats.shape == (4, n_ind)
        assert np.array_equal(paths, want)
        _check_stats(stats, paths, d.pos_dist_mb)
        if n_sites >= 900 and n_ind >= 30:      # (one individual may well be all 0)
            assert 0 < paths.mean() < 1 and (stats["n_tracts"] > 1).any()
        # the same bits on a second call; records of draws that are not kept
        stats2, paths2 = h.sample_paths(4, seed=seed, keep=1)
        assert stats2.tobytes() == stats.tobytes() and np.array_equal(paths2[0], paths[0])
        stats3, none = h.sample_paths(4, seed=seed)
        assert stats3.tobytes() == stats.tobytes() and none.shape == (0, n_ind, n_sites)


def test_draws_do_not_depend_on_the_call(pkg):
    d, F, A = _data(pkg, 40, 6000, 5)
    with _handle(pkg, d, F, A, "fast") as h:
        s19, p19 = h.sample_paths(19, seed=9, keep=19)     # three batches, the last one partial
        s3, p3 = h.sample_paths(3, seed=9, keep=3)
        assert np.array_equal(p19[:3], p3) and s19[:3].tobytes() == s3.tobytes()
        s8, p8 = h.sample_paths(8, seed=9, keep=2)
        assert np.array_equal(p8, p19[:2]) and s8.tobytes() == s19[:8].tobytes()
        _check_stats(s19, p19, d.pos_dist_mb)
        assert len({p19[k].tobytes() for k in range(19)}) == 19
        _, other = h.sample_paths(3, seed=10, keep=3)
        assert not np.array_equal(other, p3)
        # a seed above 32 bits reaches the key's high word
        _, hi = h.sample_paths(1, seed=9 + (1 << 32), keep=1)
        assert not np.array_equal(hi[0], p3[0])
        want = su.backward_draw(
            su.thresholds(su.forward_filter(h.e_prob, d.pos_dist_mb, h.indF, h.alpha), d.pos_dist_mb,
                          h.indF, h.alpha), su.uniforms(9 + (1 << 32), [0], 40, 6000))
        assert (hi != want).mean() < 1e-3    # (no fragility precondition here: near equality)
        summ = pkg.path_stats_summary(s19)
        assert summ["ibd_sites"].shape == (3, 40)
        assert np.all(summ["ibd_sites"][0] <= summ["ibd_sites"][2])


def test_chain_of_three_shards_equals_one_handle(pkg):
    n_ind, S, seed = 24, 9000, 201                         # smallest |u - p| met: 2.590e-07
    d, F, A = _data(pkg, n_ind, S, 21)
    F[:4], A[:4] = 0.9, 0.01                               # long tracts: across every cut
    gl = pkg.simulate.normalise_log_gl(d.gl)
    chrom = int(np.flatnonzero(np.isinf(d.pos_dist_mb))[1])
    cuts = [0, 2501, chrom, S]                             # an odd first site; a chromosome start at a first site

    def make(lo, hi):
        h = pkg.NgsFHMM(n_ind, hi - lo, mode=pkg.MODE_FAST)
        h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
        h.set_params(F, A, 0.15)
        h.init_emission()
        return h

    hs = [make(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    whole = make(0, S)
    try:
        ch = pkg.Chain(hs)
        for _ in range(2):
            ch.iter_EM()
        whole.set_params(hs[0].indF, hs[0].alpha, ch.freq)
        want, _ = _restate(whole, d.pos_dist_mb, seed, range(4), 1e-9)
        ws, wp = whole.sample_paths(4, seed=seed, keep=4)
        assert np.array_equal(wp, want)
        cs, cp = ch.sample_paths(4, seed=seed, keep=4)
        assert cp.shape == (4, n_ind, S)
        assert np.array_equal(cp, wp)
        for f in ("ibd_sites", "n_tracts", "longest_sites"):
            np.testing.assert_array_equal(cs[f], ws[f], err_msg=f)
        np.testing.assert_allclose(cs["ibd_mb"], ws["ibd_mb"], rtol=1e-12)
        _check_stats(cs, cp, d.pos_dist_mb)
        # tracts across both shard boundaries (the second one is a chromosome start: cut there)
        assert (cp[:, :, 2500] & cp[:, :, 2501]).any()
        assert (cp[:, :, chrom - 1] & cp[:, :, chrom]).any()
        cs2, _ = ch.sample_paths(4, seed=seed)
        assert cs2.tobytes() == cs.tobytes()
        with pytest.raises(pkg.NgsFHMMError) as ei:
            ch.sample_paths(0)
        assert ei.value.code == -10
    finally:
        for h in hs:
            h.close()
        whole.close()


def test_sample_means_match_the_posteriors(pkg):
    """256 draws against the E-step's posteriors at the same parameters, on the cohort and with
    the seed the bounds were calibrated with on the restatement (test_sample_cpu.py)."""
    d, gl, F, A, freq, R, seed = su.calibration_case(pkg)
    with pkg.NgsFHMM(d.n_ind, d.n_sites, mode=pkg.MODE_FAST) as h:
        h.load(gl, d.pos_dist_mb)
        h.set_params(F, A, freq)
        h.init_emission()
        h.estep()
        p = h.marg_prob                                     # snapped to 0 / 1 within 1e-5
        _, paths = h.sample_paths(R, seed=seed, keep=R)
        z2, N = check_calibration(paths, p)
        print(f"\n  mean z^2 = {z2:.4f} over {N} cells")


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_nothing_else_moves(pkg, mode):
    d, F, A = _data(pkg, 30, 3000, 8)
    with _handle(pkg, d, F, A, mode) as a, _handle(pkg, d, F, A, mode) as b:
        for h in (a, b):
            h.viterbi()
        a.sample_paths(9, seed=4, keep=1)
        assert a.ibd_tracts("viterbi").tobytes() == b.ibd_tracts("viterbi").tobytes()
        assert a.marg_prob.tobytes() == b.marg_prob.tobytes()
        assert a.geno_posteriors().tobytes() == b.geno_posteriors().tobytes()
        a.sample_paths(2, seed=5)
        for h in (a, b):
            h.iter_EM()
        for f in ("indF", "alpha", "freq", "marg_prob", "ind_lkl"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_argument_errors(pkg):
    d, F, A = _data(pkg, 4, 200, 3)
    u8p = C.POINTER(C.c_uint8)
    with pkg.NgsFHMM(4, 200, mode=pkg.MODE_FAST) as h:
        with pytest.raises(pkg.NgsFHMMError) as ei:         # no data loaded
            h.sample_paths(1)
        assert ei.value.code == -10 and "no data" in ei.value.message
        h.load(pkg.simulate.normalise_log_gl(d.gl), d.pos_dist_mb)
        h.set_params(F, A, 0.15)
        h.init_emission()
        for n, k in ((0, 0), (2, 3)):
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.sample_paths(n, keep=k)
            assert ei.value.code == -10 and "n_draws" in ei.value.message
        buf = np.zeros((1, 4, 200), dtype=np.uint8)
        L = h.lib
        assert L.nghmm_sample_paths(h.handle, 0, 2, None, 1, None) == -10          # keep without paths
        assert L.nghmm_sample_paths(h.handle, 0, 2, None, 0, buf.ctypes.data_as(u8p)) == -10
        assert L.nghmm_last_error() != b""
        assert L.nghmm_sample_paths(None, 0, 2, None, 0, None) == -10
        assert L.nghmm_chain_sample_paths(None, 1, 0, 2, None, 0, None) == -10
        assert L.nghmm_sample_paths(h.handle, 0, 2, None, 0, None) == 0            # stats may be NULL


@pytest.mark.parametrize("tag,extra", [
    ("exact", ["--mode", "exact"]),
    ("chain", ["--mode", "fast", "--n_gpus", 2, "--devices", "0,0"]),
])
def test_cli_sample_paths(pkg, tmp_path, tag, extra):
    """ngsF-HMM --sample_paths: the records of PREFIX.ibd.samples are those of the kept path files,
    a second run writes the same bytes, and the other output files do not change."""
    I, S = 12, 3001
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=3, indF=0.6, alpha=0.05)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    base = ["--geno", p["glf_gz"], "--loglkl", "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S,
            "--freq", 0.1, "--indF", "0.6,0.05", "--min_iters", 2, "--max_iters", 3, "--verbose", 0] + extra
    flag = ["--sample_paths", 5, "--sample_keep", 5, "--sample_seed", 42]
    plain, a, b = [str(tmp_path / f"{n}_{tag}") for n in ("plain", "a", "b")]
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", a] + flag)
    cli_util.run_cli(base + ["--out", b] + flag)
    rows = [ln.split("\t") for ln in open(a + ".ibd.samples").read().split("\n")[:-1]]
    assert [(r[0], int(r[1])) for r in rows] == [(f"ind{i}", k + 1) for i in range(I) for k in range(5)]
    seen = set()
    for k in range(5):
        text = open(f"{a}.sample_{k + 1:02d}.ibd").read().split("\n")
        assert text[0] == "//" and len(text) == I + 2
        z = np.array([[int(c) for c in ln] for ln in text[1:-1]], dtype=np.uint8)
        assert z.shape == (I, S)
        seen.add(z.tobytes())
        want = su.path_stats(z, d.pos_dist_mb)
        for i in range(I):
            r = rows[i * 5 + k]
            assert (int(r[2]), int(r[3]), int(r[4])) == \
                (want["ibd_sites"][i], want["n_tracts"][i], want["longest_sites"][i])
            assert re.fullmatch(r"\d+\.\d{6}", r[5]) and abs(float(r[5]) - want["ibd_mb"][i]) <= 1e-6
    assert len(seen) == 5
    for ext in [".ibd.samples"] + [f".sample_{k:02d}.ibd" for k in range(1, 6)]:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(a + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".ibd.samples")
