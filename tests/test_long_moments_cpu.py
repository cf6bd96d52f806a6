"""Mean and variance of IBD in long tracts without a GPU: the two numpy yardsticks of
tests/long_moments_util.py against brute-force enumeration, their spread on the cohort of
tests/test_gpu_long_moments.py (the figure that test's tolerance is made of), the long chain (what
float64 costs the centred recursion, and that the uncentred one misses 16 x that), the condition of
the test against the sampler, long_moment_sd, the binding against the header, and the host's
--ibd_long_moments writer, a program of its own under AddressSanitizer / UBSan, against the CPU
stand-in of the library (tests/stub/)."""
import os
import re
import subprocess

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import expect_util as xu
import long_moments_util as mu
import longest_util as lu
import sample_util as su
import summary_util
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sums of at most 2^12 path probabilities times second moments of at most 12^2 against products of
# at most 12 factors: a few hundred roundings of 1.1e-16 at a scale of 144
ENUM_ATOL = 2e-12


def _small_sets(S):
    return {"whole": np.array([[0, S]]), "chrom": np.array([[0, 7], [7, S]]), "across": np.array([[2, 10]]),
            "single": xu.single_site_regions(S)}


def test_yardsticks_equal_enumeration():
    """A and B (np.longdouble and float64, centred and not) against all 2^12 paths, sites and Mb:
    the whole data (two chromosomes, so a chromosome start inside), the chromosomes, a region
    across the chromosome start, regions of one site; a called heterozygote whose IBD state is
    excluded (a blocked step inside; five exact zeros on that cell); a threshold of 20 sites that
    nothing reaches (exact zeros)."""
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    ca, cb = lu.cells_a(e, pos, F, A), lu.cells_b(e, pos, F, A)
    assert np.isneginf(cb[2][:, ~xu.chrom_start(pos)]).any()                # a blocked step inside
    worst = 0.0
    lens = {"sites": bu.SMALL_LEN["sites"] + (20,), "mb": bu.SMALL_LEN["mb"] + (1.2,)}
    for unit, L in lens.items():
        for tag, reg in _small_sets(S).items():
            want = mu.enumerate_long_moments(e, pos, F, A, L, unit, reg)
            assert want.shape == (e.shape[0], len(reg), len(L))
            for name, rec in (("A", mu.records_a(ca, pos, L, unit, reg)),
                              ("B", mu.records_b(cb, pos, L, unit, reg)),
                              ("B float64", mu.records_b(cb, pos, L, unit, reg, np.float64)),
                              ("B raw", mu.records_b(cb, pos, L, unit, reg, np.float64, False))):
                for f in mu.FIELDS:
                    assert np.isfinite(rec[f]).all(), (name, unit, tag, f)
                    worst = max(worst, np.abs(rec[f] - want[f]).max())
                    np.testing.assert_allclose(rec[f], want[f], rtol=0, atol=ENUM_ATOL,
                                               err_msg=f"{name} {unit} {tag} {f}")
                    if tag == "single":   # no run on the excluded cell, exactly
                        assert (rec[f][1, 4] == 0.0).all(), (name, unit, f)
                    if unit == "sites":   # 20 sites exceed both chromosomes
                        assert (rec[f][:, :, -1] == 0.0).all(), (name, tag, f)
                assert (rec["var_a"] >= 0).all() and (rec["var_t"] >= 0).all()
    print(f"\n  yardsticks against enumeration: largest difference {worst:.2e}")


def test_path_long_moments():
    pos = np.array([np.inf, 0.5, 0.5, 0.25, np.inf, 1.0, 0.5])
    z = np.array([[1, 1, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1]])
    # runs of path 0: [0, 1] 0.5 Mb, [3] 0 Mb, [4, 6] 1.5 Mb (cut at the chromosome start)
    A, Cn = mu.path_long_moments(z, pos, "sites", 1)
    assert A.tolist() == [6, 0, 4] and Cn.tolist() == [3, 0, 4]
    A, Cn = mu.path_long_moments(z, pos, "sites", 2)
    assert A.tolist() == [5, 0, 0] and Cn.tolist() == [2, 0, 0]
    A, Cn = mu.path_long_moments(z, pos, "mb", 0.0)
    assert A.tolist() == [2.0, 0, 0] and Cn.tolist() == [3, 0, 4]
    A, Cn = mu.path_long_moments(z, pos, "mb", (0.5, 1.5, 2.0))
    assert A.tolist() == [[2.0, 1.5, 0], [0, 0, 0], [0, 0, 0]] and Cn.tolist() == [[2, 1, 0], [0, 0, 0], [0, 0, 0]]


@pytest.fixture(scope="module")
def cohort_cells(pkg):
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    pos = d.pos_dist_mb
    return d, e, F, A, lu.cells_a(e, pos, F, A), lu.cells_b(e, pos, F, A)


def test_yardstick_spread_on_the_gpu_cohort(cohort_cells):
    """rel_err(A, B) per unit and field on the cohort, thresholds and region sets of the GPU test
    (printed; long_moments_util.SPREAD holds the figures, and the GPU tolerance is 16 x them).  To
    re-measure: pytest -s tests/test_long_moments_cpu.py -k spread, and copy the printed maxima."""
    d, e, F, A, ca, cb = cohort_cells
    pos = d.pos_dist_mb
    for unit, L in bu.COHORT_LEN.items():
        worst = {f: 0.0 for f in mu.FIELDS}
        for name, reg in xu.region_sets(d.n_sites, pos, xu.SPREAD_LANE_SITES).items():
            a, b = mu.records_a(ca, pos, L, unit, reg), mu.records_b(cb, pos, L, unit, reg)
            r = mu.rel_err(a, b)
            worst = {f: max(worst[f], r[f]) for f in mu.FIELDS}
            for f in mu.FIELDS:
                assert np.isfinite(a[f]).all() and np.isfinite(b[f]).all(), (unit, name, f)
                if unit == "sites":   # 2000 sites exceed every chromosome: exactly nothing
                    assert (a[f][:, :, -1] == 0).all() and (b[f][:, :, -1] == 0).all()
        print(f"\n  spread of A against B in {unit}: " + ", ".join(f"{f} {v:.3e}" for f, v in worst.items()))
        # what the GPU test uses is what is measured here (within a factor of two: libm versions)
        for f in mu.FIELDS:
            assert 0 < mu.SPREAD[unit][f] and worst[f] <= 2 * mu.SPREAD[unit][f], (unit, f, worst[f])
    # the means far inside the project's own bound on posteriors (1e-9 per site); the second moments
    # carry yardstick A's raw moments, E[A]^2 / Var(A) roundings
    assert max(mu.TOL[u][f] for u in mu.UNITS for f in ("mean_a", "mean_t")) <= 1e-9
    assert max(mu.TOL[u][f] for u in mu.UNITS for f in mu.FIELDS) <= 1e-7


def test_long_chain(pkg):
    """3 x 50 000 on one chromosome at 50 sites and 0.5 Mb: rel_err(B(float64, centred),
    B(np.longdouble)) is SPREAD_LONG (printed; within a factor of two of the recorded figures);
    B(float64, NOT centred) misses TOL_LONG = 16 x SPREAD_LONG in var_t in both units, so a device
    kernel without the offsets cannot pass the GPU test; and tests/golden holds B(np.longdouble) to
    4 roundings of a double (the libm's long-double exp and log; the rounding of the result)."""
    anchor, cells, pos = mu.long_chain_anchor(pkg)
    S = len(pos)
    assert S == mu.LONG_SITES >= 50000 and int(xu.chrom_start(pos).sum()) == 1
    gold = np.load(mu.GOLDEN_LONG)
    assert gold.dtype == mu.DTYPE and gold.shape == anchor.shape == (2, 3, 1, 1)
    for n, unit in enumerate(mu.UNITS):
        assert mu.within(gold[n], anchor[n], {f: 4 * 2.0 ** -53 for f in mu.FIELDS}), unit
        centred = mu.records_b(cells, pos, mu.LONG_LEN[unit], unit, [[0, S]], np.float64, True)
        raw = mu.records_b(cells, pos, mu.LONG_LEN[unit], unit, [[0, S]], np.float64, False)
        rc, rr = mu.rel_err(centred, anchor[n]), mu.rel_err(raw, anchor[n])
        print(f"\n  long chain {unit}: centred " + ", ".join(f"{f} {v:.3e}" for f, v in rc.items()))
        print(f"  long chain {unit}: raw     " + ", ".join(f"{f} {v:.3e}" for f, v in rr.items()))
        for f in mu.FIELDS:
            assert 0 < mu.SPREAD_LONG[unit][f] and rc[f] <= 2 * mu.SPREAD_LONG[unit][f], (unit, f, rc[f])
        assert rr["var_t"] > mu.TOL_LONG[unit]["var_t"], (unit, rr["var_t"])
        assert not mu.within(raw, anchor[n], mu.TOL_LONG[unit])


def test_sampler_condition_on_the_gpu_cohort(cohort_cells):
    """The restatement of the sampler (sample_util) against yardstick B on the GPU test's cohort,
    draws (R = 400) and seed, at the thresholds SAMPLER_LEN: both conditions of
    long_moments_util.sampler_check hold before the device is asked."""
    d, e, F, A, ca, cb = cohort_cells
    pos = d.pos_dist_mb
    assert mu.SAMPLER_DRAWS == xu.SAMPLER_DRAWS
    f = su.forward_filter(e, pos, F, A)
    thr = su.thresholds(f, pos, F, A)
    u = su.uniforms(xu.SAMPLER_SEED, range(mu.SAMPLER_DRAWS), d.n_ind, d.n_sites)
    paths = su.backward_draw(thr, u)
    for unit, L in bu.SAMPLER_LEN.items():
        exact = mu.records_b(cb, pos, L, unit, [[0, d.n_sites]])[:, 0]
        worst = mu.sampler_check(*mu.path_long_moments(paths, pos, unit, L), exact, mu.sampler_var_k(unit), unit)
        print(f"\n  sampler restatement against yardstick B in {unit}: largest |z| = {worst:.2f}")


def test_long_moment_sd(pkg):
    s = np.zeros(3, dtype=pkg.LONG_MOMENT_DTYPE)
    s[0] = (40.0, 2.0, 16.0, 3.0, 1.0)
    s[1] = (0.0, 0.0, 0.0, 0.0, 0.0)
    s[2] = (5.0, 1.0, 0.0, 0.0, 0.25)
    out = pkg.long_moment_sd(s)
    assert set(out) == {"sd_a", "sd_t", "corr", "tract_length", "tract_length_sd"}
    assert out["sd_a"].tolist() == [4.0, 0.0, 0.0] and out["sd_t"].tolist() == [1.0, 0.0, 0.5]
    assert out["corr"][0] == 0.75 and np.isnan(out["corr"][1:]).all()
    assert out["tract_length"][0] == 20.0 and np.isnan(out["tract_length"][1]) and out["tract_length"][2] == 5.0
    assert out["tract_length_sd"][0] == np.sqrt(16.0 - 2 * 20 * 3.0 + 400 * 1.0) / 2.0
    ref = pkg.moment_sd(s)
    for k in ref:
        assert np.array_equal(out[k], ref[k], equal_nan=True)
    out = pkg.long_moment_sd(s, total=np.array([100.0, 0.0, 10.0]))
    assert out["share"][0] == 0.4 and out["share_sd"][0] == 0.04 and out["share"][2] == 0.5
    assert np.isnan(out["share"][1]) and np.isnan(out["share_sd"][1])
    assert pkg.long_moment_sd(s.reshape(3, 1), total=50.0)["share"].shape == (3, 1)


def test_binding_mirrors_the_header(pkg):
    """The enum, the record and the argument order in include/nghmm.h, the binding and the kernels'
    header; no chain twin."""
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    assert int(re.search(r"NGHMM_LONG_MOMENTS_MB = (\d+)", header).group(1)) == pkg.LONG_MOMENTS_MB == 1
    decl = re.search(r"int nghmm_ibd_long_moments\((.*?)\);", header, re.S).group(1)
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
    assert args == ["nghmm_t* h", "int what", "uint32_t n_lengths", "const double* min_length", "uint64_t n_regions",
                    "const uint64_t* region_begin", "const uint64_t* region_end", "nghmm_long_moment_stat* stats"]
    rec = re.search(r"typedef struct nghmm_long_moment_stat \{(.*?)\} nghmm_long_moment_stat;", header, re.S).group(1)
    fields = re.findall(r"double (\w+);", rec)
    assert tuple(fields) == pkg.LONG_MOMENT_DTYPE.names == pkg.MOMENT_REGION_DTYPE.names == mu.FIELDS
    assert pkg.LONG_MOMENT_DTYPE.itemsize == C.sizeof(pkg.hmm.LongMomentStat) == 40
    assert "sizeof(nghmm_long_moment_stat) == 40" in header
    assert "nghmm_ibd_long_moments" in pkg.hmm.EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "ngsf-hmm_amd", "hmm.py")).read()
    sig = re.search(r'"nghmm_ibd_long_moments": \(i32, \[(.*?)\]\)', src, re.S).group(1)
    assert [a.strip() for a in re.sub(r"C\.POINTER\(u64\)", "u64p", sig).split(",")] == \
        ["vp", "i32", "u32", "dp", "u64", "u64p", "u64p", "vp"]
    kh = open(os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "kernels_long_moments.hpp")).read()
    assert int(re.search(r"kLongMomentEntry = (\d+)", kh).group(1)) == 9
    assert "nghmm_chain_ibd_long_moments" not in header and not hasattr(pkg.Chain, "ibd_long_moments")
    assert hasattr(pkg.NgsFHMM, "ibd_long_moments")


@pytest.fixture(scope="module")
def asan_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp with and without the entry of tests/stub/nghmm_long_moments_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_long_moments")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_long_moments_stub.cpp")), ("without", ("nghmm_stub.cpp",))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "%.10g" % v


def test_ibd_long_moments_writer_under_address_sanitizer(pkg, tmp_path, asan_host):
    """--ibd_long_moments writes PREFIX.ibd.long.moments: the header, one line per individual,
    chromosome (or window that restarts at every chromosome) and threshold in that order, the stub's
    formulas as %.10g, NA for the correlation where a variance is 0; Mb by default and sites with
    --long_moments_sites; default IDs and --ind_names; multi-start replicates (the winning one's
    only); more than one handle is refused before any work; without the flag the file does not
    appear and the other files are byte-identical; the two companion flags alone are a warning; bad
    threshold lists are refused; a library without the entry still links and stops the run with a
    message."""
    I, S = 5, 301
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "0", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k} extra\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    runs = [
        ("chrom", [], 0, None, "0,0.25,1.5", False),
        ("window", ["--long_moments_window", 40, "--ind_names", tmp_path / "names.txt"], 40, names, "1,2,30", True),
        ("win7", ["--long_moments_window", 7], 7, None, "0.5", False),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], 0, None, "1,2,3,4,5,6,7,8", True),
    ]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    n_na = 0
    for tag, extra, window, ids, lens, in_sites in runs:
        plain, ex = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"ex_{tag}")
        unit = ["--long_moments_sites"] if in_sites else []
        r = run(asan_host["full"], plain, extra + unit)
        assert ("are only used by --ibd_long_moments" in r.stderr) == bool(window or in_sites)
        assert ("--ind_names is only used by" in r.stderr and "and --ibd_long_moments" in r.stderr) == (tag == "window")
        run(asan_host["full"], ex, extra + unit + ["--ibd_long_moments", lens])
        ids = ids or [f"ind{i}" for i in range(I)]
        regions = summary_util.chrom_regions(chrom, window)
        L = [float(x) for x in lens.split(",")]
        want = ["\t".join(["ind", "chr", "first_pos", "last_pos", "n_sites", "min_len", "exp_len", "sd_len",
                           "exp_tracts", "sd_tracts", "corr"])]
        for i in range(I):
            for r_, (a, b) in enumerate(regions):
                a, b = int(a), int(b)
                for k, l in enumerate(L):
                    mean_a = (1.0 + i) * (b - a) / (3.0 + l) + (0.25 if in_sites else 0.5) * (k + 1)
                    mean_t = (1.0 + i) / (2.0 + i + a) + 1e-3 * k
                    var_a = 0.0 if r_ % 3 == 2 else 4.0 + k + 0.5 * i
                    cov = (-0.5 if k % 2 else 0.75) / (1.0 + i)
                    var_t = 0.0 if (i % 2 == 1 and k == 0) else 0.25 * (k + 1) + 1e-2 * (b - a)
                    corr = _g10(cov / (np.sqrt(var_a) * np.sqrt(var_t))) if var_a > 0 and var_t > 0 else "NA"
                    n_na += corr == "NA"
                    want.append("\t".join([ids[i], chrom[a], str(pos[a]), str(pos[b - 1]), str(b - a), _g10(l),
                                           _g10(mean_a), _g10(np.sqrt(var_a)), _g10(mean_t), _g10(np.sqrt(var_t)),
                                           corr]))
        got = open(ex + ".ibd.long.moments").read()
        assert got == "\n".join(want) + "\n", tag
        assert got.count("\n") == 1 + I * len(regions) * len(L)
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(ex + ext, "rb").read(), (tag, ext)
        made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                                  if f.startswith(os.path.basename(pre) + "."))
        new = [e for e in made(ex) if e not in made(plain)]
        assert all(e.endswith(".ibd.long.moments") for e in new), (tag, new)
        assert len(new) == (2 if tag == "starts" else 1)          # (the winning replicate's only)
    assert n_na > 10
    # more than one handle: refused at argument checking, before any work
    r = run(asan_host["full"], str(tmp_path / "shards"),
            ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--ibd_long_moments", "1"], ok=False)
    assert "--ibd_long_moments: site shards (--n_gpus > 1) are not supported yet!" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("shards.")]
    for lens, unit in (("", []), ("1,,2", []), ("1,x", []), ("2,1", []), ("1,1", []), ("-1,2", []),
                       ("0.5,2", ["--long_moments_sites"]), ("0,1", ["--long_moments_sites"]),
                       ("1,2,3,4,5,6,7,8,9", []), ("inf", []), ("nan", [])):
        r = run(asan_host["full"], str(tmp_path / "bad"), unit + ["--ibd_long_moments", lens], ok=False)
        assert "invalid --ibd_long_moments" in r.stderr, (lens, r.stderr[-500:])
    r = run(asan_host["full"], str(tmp_path / "bad"), ["--ibd_long_moments", "1", "--long_moments_window", 0], ok=False)
    assert "invalid --long_moments_window" in r.stderr
    r = run(asan_host["without"], str(tmp_path / "none"), ["--ibd_long_moments", "1"], ok=False)
    assert "--ibd_long_moments: the library has no nghmm_ibd_long_moments!" in r.stderr
    run(asan_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_chrom") + ext, "rb").read(), ext
