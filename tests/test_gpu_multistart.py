"""Multi-start (ngsF-HMM.sh:77-101 runs 20 replicates from random
starts and keeps the best likelihood): replicas share the likelihoods on the device
(nghmm_create_replica) and run concurrently, one host thread and one HIP stream each.
A replica must behave exactly like an independent handle loaded with the same data:
bit-identical results in exact AND fast mode (both are deterministic), whatever runs next
to it."""
import os
import re
import threading

import numpy as np
import pytest

import cli_util
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def _run(h, start, iters):
    h.set_params(*start)
    h.init_emission()
    lk = []
    for _ in range(iters):
        h.iter_EM()
        lk.append(h.ind_lkl.sum())
    return dict(lk=np.array(lk), indF=h.indF.copy(), alpha=h.alpha.copy(), freq=h.freq.copy(),
                post=h.marg_prob.copy(), path=h.viterbi())


@pytest.mark.parametrize("mode_name,packed", [("exact", False), ("fast", False), ("fast", True)])
def test_replicas_equal_independent_handles(pkg, mode_name, packed):
    I, S, R, iters = 24, 3000, 4, 3
    d = pkg.simulate.simulate(I, S, seed=77, n_chrom=3, missing_rate=0.03, indF="r")
    mode = (pkg.MODE_EXACT if mode_name == "exact" else pkg.MODE_FAST) | (pkg.GENO_PACKED if packed else 0)
    rng = np.random.default_rng(1)
    starts = [(rng.uniform(0.01, 0.9, I), rng.uniform(0.01, 2.0, I), rng.uniform(0.02, 0.48, S))
              for _ in range(R)]

    def load(h):
        h.load_raw(d.gl, d.pos_dist_mb, space=0, call_geno=packed)

    want = []
    for r in range(R):                      # R independent handles, one after the other
        with pkg.NgsFHMM(I, S, mode=mode) as h:
            load(h)
            want.append(_run(h, starts[r], iters))

    parent = pkg.NgsFHMM(I, S, mode=mode)
    load(parent)
    hs = [parent] + [parent.replica() for _ in range(R - 1)]
    got = [None] * R
    err = []

    def work(r):
        try:
            got[r] = _run(hs[r], starts[r], iters)
        except BaseException as e:          # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for r in range(R):
        for k in want[r]:
            assert np.array_equal(got[r][k], want[r][k]), (r, k)
    # the parent cannot go before its replicas, nor be reloaded under them
    with pytest.raises(pkg.NgsFHMMError):
        parent.close()
    with pytest.raises(pkg.NgsFHMMError):
        load(parent)
    for h in hs[1:]:
        h.close()
    parent.close()


def test_cli_n_starts_keeps_the_best_replicate(pkg, tmp_path):
    """--n_starts 3 --seed 5 with random starts = the three runs --seed 5, 6, 7; the output
    files are those of the run with the largest final log-likelihood (ngsF-HMM.sh:93-101)."""
    I, S = 10, 1500
    d = pkg.simulate.simulate(I, S, seed=12345, n_chrom=2)
    paths = cli_util.write_inputs(str(tmp_path), d, d.gl)
    common = ["--geno", paths["glf_bin"], "--loglkl", "--pos", paths["pos_gz"], "--n_ind", I,
              "--n_sites", S, "--freq", "r", "--indF", "r", "--min_iters", 3, "--max_iters", 6,
              "--mode", "fast", "--verbose", 1]
    singles = []
    for seed in (5, 6, 7):
        out = str(tmp_path / f"single_{seed}")
        cli_util.run_cli(common + ["--seed", seed, "--out", out])
        singles.append((float(open(out + ".indF").readline()), out))
    best = max(singles, key=lambda t: t[0])
    out = str(tmp_path / "multi")
    r = cli_util.run_cli(common + ["--seed", 5, "--n_starts", 3, "--keep_starts", "--out", out])
    assert "Best replicate: %d (seed %d)" % (singles.index(best) + 1, 5 + singles.index(best)) in r.stdout
    for ext in (".indF", ".ibd", ".geno"):
        assert open(out + ext, "rb").read() == open(best[1] + ext, "rb").read()
        for k, (_, single) in enumerate(singles):       # --keep_starts: every replicate's files
            assert open(f"{out}.REP_{k + 1:02d}{ext}", "rb").read() == open(single + ext, "rb").read()
    out2 = str(tmp_path / "multi2")
    cli_util.run_cli(common + ["--seed", 5, "--n_starts", 3, "--out", out2])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(out2 + ext, "rb").read() == open(best[1] + ext, "rb").read()
    assert not os.path.exists(out2 + ".REP_01.indF")


# every optional output of the multi-start branch of main, and the files they make
ALL_OUTPUTS = ["--ibd_bed", "--sample_paths", 4, "--sample_keep", 2, "--indF_se", "--ibd_summary",
               "--ibd_sharing", "--ibd_support", "--ibd_bounds", "--freq_info", "--geno_smooth",
               "--geno_summary", "--ibd_expect", "--ibd_moments", "--ibd_by_length", "0.05,0.5",
               "--ibd_longest", "0,0.5,2"]
ALL_EXTS = [".indF", ".ibd", ".geno", ".ibd.bed", ".ibd.samples", ".sample_01.ibd", ".sample_02.ibd",
            ".indF.se", ".ibd.regions", ".ibd.sites", ".ibd.sharing", ".ibd.support", ".ibd.bounds",
            ".freq.info", ".geno.smooth", ".geno.regions", ".geno.sites", ".ibd.expect", ".ibd.breaks",
            ".ibd.moments", ".ibd.bylength", ".ibd.longest"]
# base seeds at which replicate 1 does not win (the test asserts it), chosen by trying 1 .. 6 on
# the device (replicate 1 wins at 3 and 4 in both modes): the third replicate wins in fast mode,
# the second in exact mode
BASE_SEED = {"fast": 1, "exact": 2}


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_cli_n_starts_outputs_come_from_a_replica(pkg, tmp_path, mode):
    """--n_starts 3 --keep_starts with every optional output switched on: main calls finish_run on
    the winning replicate's handle, which is a replica (nghmm_create_replica) unless replicate 1
    wins -- so the base seed is one at which it does not.  Every file under the output prefix is
    byte for byte the file of the single run --seed <winner's> with the same flags, which runs on
    a handle of its own.

    As measured on an MI355X (final log-likelihoods of replicates 1, 2, 3):
      fast,  base seed 1: -12087.6374074095, -12087.6374132318, -12087.6374056064 (replicate 3 wins)
      exact, base seed 2: -12087.6374132311, -12087.6374056072, -12087.6374095789 (replicate 2 wins)
    All replicates reach the same optimum to 1e-5; both modes are deterministic, so the order of
    the last digits, and with it the winner, is fixed."""
    I, S = 10, 1500
    d = pkg.simulate.simulate(I, S, seed=12345, n_chrom=2)
    paths = cli_util.write_inputs(str(tmp_path), d, d.gl)
    common = ["--geno", paths["glf_bin"], "--loglkl", "--pos", paths["pos_gz"], "--n_ind", I,
              "--n_sites", S, "--freq", "r", "--indF", "r", "--min_iters", 3, "--max_iters", 6,
              "--mode", mode, "--verbose", 1] + ALL_OUTPUTS
    base = BASE_SEED[mode]
    out = str(tmp_path / "multi")
    r = cli_util.run_cli(common + ["--seed", base, "--n_starts", 3, "--keep_starts", "--out", out])
    m = re.search(r"Best replicate: (\d+) \(seed (\d+)\), logLkl (\S+)", r.stdout)
    assert m, r.stdout[-2000:]
    best, seed = int(m.group(1)), int(m.group(2))
    lkl = [float(open(f"{out}.REP_{k:02d}.indF").readline()) for k in (1, 2, 3)]
    print(f"{mode}: base seed {base}, final log-likelihoods {lkl}, best replicate {best}")
    assert best == int(np.argmax(lkl)) + 1 and seed == base + best - 1
    assert best != 1, "replicate 1 won: the outputs came from the parent, not from a replica"
    single = str(tmp_path / "single")
    cli_util.run_cli(common + ["--seed", seed, "--out", single])
    for ext in ALL_EXTS:
        want = open(single + ext, "rb").read()
        assert len(want) > 0, ext
        assert open(out + ext, "rb").read() == want, ext
        assert open(f"{out}.REP_{best:02d}{ext}", "rb").read() == want, ext
    made = sorted(f[len("single"):] for f in os.listdir(tmp_path) if f.startswith("single."))
    assert made == sorted(ALL_EXTS), "a file of the single run that the comparison does not know"
