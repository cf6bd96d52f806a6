"""The per-site frequency likelihood without a GPU: the two numpy yardsticks of
tests/freqinfo_util.py against enumeration (the cavity), against differences of whole-chain
log-likelihoods (ll and the curve) and against the quadratic that three whole-chain evaluations
fix (score and info); their spread on the cohort of tests/test_gpu_freqinfo.py, the figure that
test's tolerance is made of; and the host's --freq_info writer under AddressSanitizer / UBSan
against the CPU stand-in of the library (tests/stub/).

Tolerances: 64 eps times the sum of the absolute values of the entry's terms, which the yardsticks
return (for a cavity weight: the two normalised products, sum 1); where the other side subtracts
whole-chain log-likelihoods, 64 eps times the sum of their absolute values is added."""
import math
import os
import subprocess

import numpy as np
import pytest

import cli_util
import freqinfo_util as fu
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS = float(np.finfo(np.float64).eps)
YARDSTICKS = (("A", fu.freq_info_a), ("B", fu.freq_info_b))


def _log_emissions(gl_i, freq):
    """pyref's log emissions of one individual: [S][2]."""
    return [[pyref.calc_emission(list(gl_i[s]), float(freq[s]), k) for k in range(2)]
            for s in range(len(freq))]


def test_cavity_equals_enumeration():
    """3 x 10 with a chromosome start inside: site s given the emissions (1, 1), the brute-force
    posterior at s is the cavity probability; both weights of both yardsticks at every cell."""
    rng = np.random.default_rng(5)
    I, S = 3, 10
    gl = np.log(rng.dirichlet(np.ones(3), size=(S, I)))
    pos = rng.uniform(0.01, 0.6, S)
    pos[0] = pos[6] = np.inf
    freq = rng.uniform(0.1, 0.6, S)
    F, A = np.array([0.3, 0.6, 0.85]), np.array([0.4, 1.5, 0.05])
    want = np.empty((I, S))
    for i in range(I):
        e = _log_emissions(gl[:, i], freq)
        for s in range(S):
            e1 = [row[:] for row in e]
            e1[s] = [0.0, 0.0]
            want[i, s] = pyref.brute_force_posterior([1 - F[i], F[i]], A[i], e1, list(pos))[s]
    for name, fn in YARDSTICKS:
        got = fn(np.exp(gl), pos, F, A, freq)
        assert np.abs(got["cavity"] - want).max() <= 64 * EPS, name
        assert np.abs(got["w0"] - (1 - want)).max() <= 64 * EPS, name
        assert np.abs(got["w0"] + got["cavity"] - 1).max() <= 4 * EPS, name
    # a chromosome start: the prediction is the stationary vector, so the cavity there is what the
    # sites to the right alone say
    assert want[0, 6] != pytest.approx(F[0], abs=1e-3)


@pytest.fixture(scope="module")
def chain_case(pkg):
    """6 x 48, depth 1, alpha 2, freq = "r" data at a frequency vector that is not the truth, and
    per individual pyref's emissions and whole-chain log-likelihood."""
    d = pkg.simulate.simulate(6, 48, seed=7, freq="r", depth=1.0, indF=0.3, alpha=2.0)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    F, A = np.full(6, 0.3), np.full(6, 2.0)
    freq = 0.8 * d.freq + 0.05
    pos = list(d.pos_dist_mb)
    e = [_log_emissions(gl[:, i], freq) for i in range(6)]
    lkl = [pyref.forward([1 - F[i], F[i]], A[i], e[i], pos)[0] for i in range(6)]
    return d, gl, F, A, freq, pos, e, lkl


LEVELS = (0.0, 0.05, 0.3, 0.9, 1.0)


def test_ll_and_curve_equal_whole_chain_differences(chain_case):
    """ll_s = sum_i [lkl_i - lkl_i with site s given the emissions (1, 1)]; curve[s][k] = sum_i
    [lkl_i with the site's emission at the level - lkl_i]: pyref.forward with the one site's
    emission replaced by pyref.calc_emission."""
    d, gl, F, A, freq, pos, e, lkl = chain_case
    I, S = 6, 48
    ll = np.zeros(S)
    curve = np.zeros((S, len(LEVELS)))
    mag = np.zeros(S)                                  # of the whole-chain numbers subtracted
    for s in range(S):
        for i in range(I):
            q = [1 - F[i], F[i]]
            e1 = [row[:] for row in e[i]]
            e1[s] = [0.0, 0.0]
            ll[s] += lkl[i] - pyref.forward(q, A[i], e1, pos)[0]
            mag[s] += abs(lkl[i])
            for k, x in enumerate(LEVELS):
                e1[s] = [pyref.calc_emission(list(gl[s, i]), x, z) for z in range(2)]
                curve[s, k] += pyref.forward(q, A[i], e1, pos)[0] - lkl[i]
    worst = {}
    for name, fn in YARDSTICKS:
        got = fn(np.exp(gl), d.pos_dist_mb, F, A, freq, LEVELS)
        assert np.isfinite(got["ll"]).all() and np.isfinite(got["curve"]).all()
        tol_ll = 64 * EPS * (got["abs_ll"] + mag)
        tol_cv = 64 * EPS * (got["abs_curve"] + mag[:, None])
        worst[name] = (np.abs(got["ll"] - ll).max(), np.abs(got["curve"] - curve).max())
        assert (np.abs(got["ll"] - ll) <= tol_ll).all(), name
        assert (np.abs(got["curve"] - curve) <= tol_cv).all(), name
    print(f"\n  largest |local - whole chain| (ll, curve): A {worst['A'][0]:.1e} {worst['A'][1]:.1e}, "
          f"B {worst['B'][0]:.1e} {worst['B'][1]:.1e}; curve values up to {np.abs(curve).max():.2f}")
    assert np.abs(curve).max() > 1.0


def _chain_likelihood(p_i, pos, F, alpha, freq):
    """Z_i of one individual in linear space, np.longdouble: q prod_s (c I + (1 - c) 1 q^T) diag(e_s) 1."""
    ld = np.longdouble
    q = np.array([1 - F, F], dtype=ld)
    v = q.copy()
    for s in range(len(pos)):
        c = ld(0) if math.isinf(pos[s]) else np.exp(-ld(alpha) * ld(pos[s]))
        f = ld(freq[s])
        om = 1 - f
        p0, p1, p2 = (ld(x) for x in p_i[s])
        e = np.array([p0 * om * om + 2 * p1 * f * om + p2 * f * f, p0 * om + p2 * f], dtype=ld)
        v = (c * v + (1 - c) * q * v.sum()) * e
    return v.sum()


def test_score_and_info_equal_the_quadratic(chain_case):
    """Z_i is a quadratic in f_s: three whole-chain evaluations (f = 0, 1/2, 1) fix a + b f + c f^2,
    and the derivatives of sum_i ln(a + b f + c f^2) at freq[s] are score and -info."""
    d, gl, F, A, freq, pos, e, lkl = chain_case
    I, S = 6, 48
    p = np.exp(gl)
    ld = np.longdouble
    score, info = np.zeros(S, dtype=ld), np.zeros(S, dtype=ld)
    for s in range(S):
        for i in range(I):
            z = []
            for x in (0.0, 0.5, 1.0):
                fr = np.array(freq, dtype=np.float64)
                fr[s] = x
                z.append(_chain_likelihood(p[:, i], pos, F[i], A[i], fr))
            a = z[0]
            c2 = 2 * (z[2] + z[0] - 2 * z[1])
            b = z[2] - z[0] - c2
            f = ld(freq[s])
            Q, dQ = a + b * f + c2 * f * f, b + 2 * c2 * f
            score[s] += dQ / Q
            info[s] -= 2 * c2 / Q - (dQ / Q) ** 2
    for name, fn in YARDSTICKS:
        got = fn(p, d.pos_dist_mb, F, A, freq)
        es, ei = np.abs(got["score"] - score.astype(np.float64)), np.abs(got["info"] - info.astype(np.float64))
        print(f"\n  {name}: largest |score - quadratic| {es.max():.1e}, |info - quadratic| {ei.max():.1e}")
        assert (es <= 64 * EPS * got["abs_score"]).all(), name
        assert (ei <= 64 * EPS * got["abs_info"]).all(), name
    assert np.abs(score).max() > 1.0 and (info > 0).mean() > 0.5


def test_yardstick_spread_on_the_gpu_cohort(pkg):
    """|A - B| on the cohort of the GPU test at its eight levels, per field, in the measure of
    freqinfo_util.spread (printed; freqinfo_util.SPREAD quotes it, the GPU tolerance is 16 x it).
    Every entry is finite in both, and the scores are far from 0."""
    d, gl, F, A, freq = fu.gpu_cohort(pkg)
    p = np.exp(gl)
    a = fu.freq_info_a(p, d.pos_dist_mb, F, A, freq, fu.LEVELS)
    b = fu.freq_info_b(p, d.pos_dist_mb, F, A, freq, fu.LEVELS)
    for r in (a, b):
        for f in fu.FIELDS:
            assert np.isfinite(r[f]).all(), f
    s = fu.spread(a, b)
    print("\n  spread |A - B| / scale: " + ", ".join(f"{k} {v:.3e}" for k, v in s.items()))
    assert np.median(np.abs(b["score"])) > 5.0
    assert b["cavity"].min() < 1e-6 and b["cavity"].max() > 0.999     # both ends are there
    # what the GPU test quotes is what is measured here (within a factor of two: libm versions)
    for k, v in s.items():
        assert v <= 2 * fu.SPREAD[k], (k, v, fu.SPREAD[k])
        assert fu.SPREAD[k] <= 4 * v, (k, v, fu.SPREAD[k])


@pytest.fixture(scope="module")
def asan_freqinfo_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp with and without the frequency-information entries."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_freqinfo")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_freqinfo_stub.cpp")), ("without", ("nghmm_stub.cpp",))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "NA" if v != v else "-inf" if v == -math.inf else "%.10g" % v


def test_freq_info_writer_under_address_sanitizer(pkg, tmp_path, asan_freqinfo_host):
    """--freq_info writes PREFIX.freq.info: the header with one dll_<level> column per level (%g),
    then one line per site with its chromosome and position and the stub's formula in the other
    columns -- NaN as NA, -inf as -inf, se = 1 / sqrt(info) only where info > 0 and 0 < freq < 1;
    one handle or a chain of three, multi-start replicates (the winning one's only); without the
    flag the set of output files and their bytes do not change; bad --freq_levels and a library
    without the entry stop the run with a message."""
    I, S = 5, 301
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]
    runs = [("one", [], (0.0,)),
            ("levels", ["--freq_levels", "0,0.25,1"], (0.0, 0.25, 1.0)),
            ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--freq_levels", "0.5"], (0.5,)),
            ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], (0.0,))]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                              if f.startswith(os.path.basename(pre) + "."))
    for tag, extra, levels in runs:
        plain, fi = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"fi_{tag}")
        k = extra.index("--freq_levels") if "--freq_levels" in extra else len(extra)
        run(asan_freqinfo_host["full"], plain, extra[:k] + extra[k + 2:])      # (without the levels too)
        run(asan_freqinfo_host["full"], fi, extra + ["--freq_info"])
        got = open(fi + ".freq.info").read().split("\n")
        assert got[-1] == "" and len(got) == S + 2
        assert got[0] == "\t".join(["chr", "pos", "freq", "se", "ll", "score", "info"] + ["dll_%g" % x for x in levels])
        n_na = n_inf = 0
        for s in range(S):
            dead = s % 11 == 0
            freq = 0.0 if s % 13 == 0 else 0.1 + (s % 50) / 100.0
            ll = -math.inf if dead else -(s + 1) / 4.0
            score = math.nan if dead else 3.0 - s / 8.0
            info = math.nan if dead else (-1.0 if s % 3 == 0 else 4.0 + s)
            se = 1.0 / math.sqrt(info) if (info > 0 and 0 < freq < 1) else math.nan
            curve = [math.nan if dead else (-math.inf if (s % 7 == 0 and k == 0) else -(s + k) / 8.0 - x)
                     for k, x in enumerate(levels)]
            want = [f"chr{int(d.chrom[s])}", str(int(d.pos[s]))] + [_g10(v) for v in [freq, se, ll, score, info] + curve]
            assert got[1 + s].split("\t") == want, (tag, s, got[1 + s])
            n_na += want.count("NA")
            n_inf += want.count("-inf")
        assert n_na > 50 and n_inf > 20
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(fi + ext, "rb").read(), (tag, ext)
        new = [e for e in made(fi) if e not in made(plain)]
        assert ".freq.info" in new and all(e.endswith(".freq.info") for e in new), (tag, new)
        assert len(new) == (2 if tag == "starts" else 1)          # (the winning replicate's only)
    for bad in ("0,1.5", "0.1,,0.2", "x", "0,0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8"):
        r = run(asan_freqinfo_host["full"], str(tmp_path / "bad"), ["--freq_info", "--freq_levels", bad], ok=False)
        assert "invalid --freq_levels" in r.stderr, (bad, r.stderr[-500:])
    r = run(asan_freqinfo_host["without"], str(tmp_path / "none"), ["--freq_info"], ok=False)
    assert "--freq_info: the library has no nghmm_chain_freq_info!" in r.stderr
    run(asan_freqinfo_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_one") + ext, "rb").read(), ext


def test_stub_handle_is_the_stand_ins():
    """tests/stub/nghmm_freqinfo_stub.cpp restates the stand-in's handle (a second translation
    unit must see the same layout): its text is that of tests/stub/nghmm_stub.cpp, token for token,
    so an edit of one that forgets the other fails here instead of corrupting memory."""
    import re

    def handle(name):
        text = open(os.path.join(ROOT, "tests", "stub", name)).read()
        m = re.search(r"struct nghmm_handle \{.*?\n\};", text, flags=re.S)
        assert m, name
        return m.group(0).split()

    assert handle("nghmm_freqinfo_stub.cpp") == handle("nghmm_stub.cpp")
