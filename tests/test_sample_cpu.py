"""The yardstick of the sampled-path tests checked before it is used (tests/sample_util.py), and
the C ABI surface of nghmm_sample_paths; no GPU."""
import ctypes as C
import importlib
import itertools
import math
import os
import random
import re

import numpy as np

import pyref
import sample_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_restatements_agree_and_match_the_published_vectors():
    # Random123's known-answer file (kat_vectors), philox4x32 10 rounds: counter and key all
    # zero, all ones, and the digits of pi
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        assert su.philox_py(key, ctr) == want
        got = su.philox_np(key[0], key[1], *ctr)
        assert tuple(int(v) for v in got) == want
    rng = random.Random(5)
    n = 10000
    v = np.array([[rng.getrandbits(32) for _ in range(6)] for _ in range(n)], dtype=np.uint64)
    got = np.stack(su.philox_np(*[v[:, k] for k in range(6)]), axis=1)
    for k in range(n):
        r = [int(x) for x in v[k]]
        assert su.philox_py((r[0], r[1]), tuple(r[2:])) == tuple(int(x) for x in got[k])


def test_uniforms_follow_the_definition():
    seed = 0x123456789abcdef0
    u = su.uniforms(seed, [0, 3], 3, 9, site0=5)
    for di, d in enumerate([0, 3]):
        for i in range(3):
            for s in range(9):
                g = 5 + s
                x = su.philox_py((seed & 0xffffffff, seed >> 32), ((g >> 1) & 0xffffffff, (g >> 1) >> 32, i, d))
                lo, hi = (x[2], x[3]) if g & 1 else (x[0], x[1])
                assert u[di, i, s] == (((hi << 32) | lo) >> 11) * 2.0 ** -53
    assert 0 <= u.min() and u.max() < 1


def _tiny(S, seed):
    rng = np.random.default_rng(seed)
    gl = np.log(rng.dirichlet([0.6, 0.6, 0.6], size=(S, 1)))
    gl[S // 2, 0] = math.log(1 / 3)                     # a missing cell
    pos = rng.uniform(0.01, 2.0, S)
    pos[0] = np.inf
    pos[S // 2 + 1] = np.inf                            # a second chromosome
    freq = rng.uniform(0.05, 0.5, S)
    return gl, pos, freq


def test_conditionals_equal_enumeration_over_all_paths():
    for S, F, alpha, seed in ((12, 0.3, 0.7, 1), (9, 0.85, 0.05, 2), (5, 0.02, 3.0, 3), (3, 0.5, 1.0, 4)):
        gl, pos, freq = _tiny(S, seed)
        e = su.emissions_np(gl, freq)
        for s in range(S):                              # the vectorised emissions are the model's
            for k in range(2):
                assert abs(e[0, s, k] - pyref.calc_emission(list(gl[s, 0]), freq[s], k)) < 1e-12
        a = su.forward_filter(e, pos, [F], [alpha])
        p = su.cond_probs(su.thresholds(a, pos, [F], [alpha]))[0]
        # explicit sum over all paths z_0 (the virtual site) .. z_S
        q = (1 - F, F)
        w = {}
        for z in itertools.product((0, 1), repeat=S + 1):
            pr = q[z[0]]
            for s in range(1, S + 1):
                pr *= math.exp(pyref.calc_trans(z[s - 1], z[s], q[z[s]], alpha, pos[s - 1]) + e[0, s - 1, z[s]])
            w[z[1:]] = w.get(z[1:], 0.0) + pr
        for s in range(S):
            for l in range(2):
                if s == S - 1:
                    num = sum(v for z, v in w.items() if z[s] == 1)
                    den = sum(w.values())
                else:
                    num = sum(v for z, v in w.items() if z[s] == 1 and z[s + 1] == l)
                    den = sum(v for z, v in w.items() if z[s + 1] == l)
                assert abs(p[s, l] - num / den) <= 1e-12, (S, s, l)
        # and the posterior helper
        post = su.posterior(a, e, pos, [F], [alpha])[0]
        want = pyref.brute_force_posterior(q, alpha, [list(r) for r in e[0]], list(pos))
        np.testing.assert_allclose(post, want, rtol=0, atol=1e-12)


def check_calibration(paths, p):
    """The statistical bounds of the sampled-path tests: per cell |k - R p| <= 6 sqrt(R p (1 - p))
    + 12 (k = draws in state 1), and the mean squared z-score over the cells with R p (1 - p) >= 5
    within 1 +- 6 sqrt(2 / N)."""
    R = paths.shape[0]
    k = paths.sum(axis=0).astype(np.float64)
    var = R * p * (1 - p)
    assert np.all(np.abs(k - R * p) <= 6 * np.sqrt(var) + 12)
    big = var >= 5
    N = int(big.sum())
    assert N > 1000
    z2 = ((k - R * p) ** 2 / np.where(big, var, 1.0))[big].sum() / N
    assert abs(z2 - 1) <= 6 * math.sqrt(2 / N), (z2, N)
    return z2, N


def test_restatement_is_calibrated():
    """The statistical test of tests/test_gpu_sample.py on the restatement alone, same cohort,
    parameters, draws and seed (mean z^2 = 1.0164 over 82436 cells; other seeds 0.989 .. 1.005)."""
    pkg = importlib.import_module("ngsf-hmm_amd")
    d, gl, F, A, freq, R, seed = su.calibration_case(pkg)
    I, S = d.n_ind, d.n_sites
    e = su.emissions_np(gl, np.full(S, freq))
    a = su.forward_filter(e, d.pos_dist_mb, F, A)
    paths = su.backward_draw(su.thresholds(a, d.pos_dist_mb, F, A), su.uniforms(seed, range(R), I, S))
    check_calibration(paths, su.posterior(a, e, d.pos_dist_mb, F, A))


def test_path_stats_on_a_hand_made_path():
    pos = np.array([np.inf, 1, 2, 4, np.inf, 8, 16, 32.0])
    x = np.array([[1, 1, 0, 1, 1, 1, 0, 1], [0] * 8, [1] * 8], dtype=np.uint8)
    st = su.path_stats(x, pos)
    assert [tuple(r) for r in st] == [(6, 4, 2, 1.0 + 8.0), (0, 0, 0, 0.0), (8, 2, 4, 7.0 + 56.0)]


def test_header_binding_and_library_have_the_entries():
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    text = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(hm.library_path())
    for name in ("nghmm_sample_paths", "nghmm_chain_sample_paths"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in hm.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "typedef struct nghmm_path_stats" in text
    assert hm.PATH_STATS_DTYPE.itemsize == 32 and hm.PATH_STATS_DTYPE == su.STATS_DTYPE
    s = np.zeros((5, 2), dtype=hm.PATH_STATS_DTYPE)
    s["n_tracts"] = np.arange(10).reshape(5, 2)
    out = hm.path_stats_summary(s, q=(0.0, 0.5, 1.0))
    assert out["n_tracts"].tolist() == [[0, 1], [4, 5], [8, 9]] and set(out) == set(hm.PATH_STATS_DTYPE.names)


def _asan_build(tmp, stubs):
    import subprocess
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    exe = str(tmp / "ngsF-HMM_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", host,
                    *[os.path.join(ROOT, "tests", "stub", f) for f in stubs], "-o", exe, "-lz", "-lpthread"],
                   check=True)
    return exe


def test_cli_sample_files_under_address_sanitizer(tmp_path_factory, tmp_path):
    """--sample_paths 3 --sample_keep 2 writes PREFIX.ibd.samples and PREFIX.sample_01/02.ibd in
    the stated format (the statistics of draws 1-2 recomputed from the kept path files), one
    handle, a chain of three, multi-start replicates; .indF / .ibd / .geno are byte-identical with
    and without the flag; against the old stubs alone the flag stops with a message and a run
    without it works."""
    import subprocess

    import cli_util
    pkg = importlib.import_module("ngsf-hmm_amd")
    new = _asan_build(tmp_path_factory.mktemp("asan_sample"),
                      ("nghmm_stub.cpp", "nghmm_tracts_stub.cpp", "nghmm_sample_stub.cpp"))
    old = _asan_build(tmp_path_factory.mktemp("asan_old"), ("nghmm_stub.cpp",))
    I, S, R, K = 5, 301, 3, 2
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "x", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k}\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        return r

    flag = ["--sample_paths", R, "--sample_keep", K, "--sample_seed", 12345678901]
    runs = [("one", [], None),
            ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--ind_names",
                       tmp_path / "names.txt"], names),
            ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3], None)]
    for tag, extra, ids in runs:
        plain, smp = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"smp_{tag}")
        run(new, plain, extra)
        run(new, smp, extra + flag)
        ids = ids or [f"ind{i}" for i in range(I)]
        for pre in [smp] + ([smp + ".REP_01", smp + ".REP_02"] if tag == "starts" else []):
            lines = open(pre + ".ibd.samples").read().split("\n")
            assert lines[-1] == "" and len(lines) == I * R + 1
            rows = [ln.split("\t") for ln in lines[:-1]]
            assert [(r[0], int(r[1])) for r in rows] == [(ids[i], k + 1) for i in range(I) for k in range(R)]
            assert all(len(r) == 6 and re.fullmatch(r"\d+\.\d{6}", r[5]) for r in rows)
            for k in range(K):
                text = open(f"{pre}.sample_{k + 1:02d}.ibd").read().split("\n")
                assert text[0] == "//" and text[-1] == "" and len(text) == I + 2
                assert all(re.fullmatch("[01]{%d}" % S, ln) for ln in text[1:-1])
                z = np.array([[int(c) for c in ln] for ln in text[1:-1]], dtype=np.uint8)
                want = su.path_stats(z, d.pos_dist_mb)
                assert want["n_tracts"].min() > 10
                for i in range(I):
                    r = rows[i * R + k]
                    assert (int(r[2]), int(r[3]), int(r[4])) == \
                        (want["ibd_sites"][i], want["n_tracts"][i], want["longest_sites"][i])
                    assert abs(float(r[5]) - want["ibd_mb"][i]) <= 1e-6
            assert not os.path.exists(f"{pre}.sample_{K + 1:02d}.ibd")
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(smp + ext, "rb").read(), (tag, ext)
        assert not os.path.exists(plain + ".ibd.samples")
    # a library without the entries: the flag stops with a message, a run without it works
    r = run(old, str(tmp_path / "old_flag"), flag, ok=False)
    assert "--sample_paths: the library has no nghmm_chain_sample_paths" in r.stderr
    run(old, str(tmp_path / "old_plain"), [])
    r = run(new, str(tmp_path / "bad_keep"), ["--sample_paths", 1, "--sample_keep", 2], ok=False)
    assert "--sample_keep" in r.stderr
