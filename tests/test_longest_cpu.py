"""The longest IBD tract without a GPU: the two numpy yardsticks of tests/longest_util.py against
brute-force enumeration, the identities of include/nghmm.h (nghmm_ibd_longest) on the yardsticks,
their spread on the cohort of tests/test_gpu_longest.py (the figure that test's tolerance is made
of), on the same cohort the condition under which that test compares p_any with sampled paths;
and the host's --ibd_longest writer, a program of its own under AddressSanitizer / UBSan, against
the CPU stand-in of the library (tests/stub/)."""
import os
import subprocess

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import expect_util as xu
import longest_util as lu
import sample_util as su
import summary_util
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The yardsticks against enumeration: probabilities, sums of at most 12 terms of order 1, each a
# product of at most 12 factors: a few hundred roundings of 1.1e-16 at the worst.  The same bound
# as test_bylength_cpu.py's and test_expect_cpu.py's.
ENUM_ATOL = 2e-13


def _small_sets(S):
    return {"whole": np.array([[0, S]]), "chrom": np.array([[0, 7], [7, S]]), "single": xu.single_site_regions(S),
            "inside": np.array([[1, 6], [8, 11]]), "across": np.array([[2, 10]]), "gaps": np.array([[0, 3], [5, 9], [11, 12]])}


def test_yardsticks_equal_enumeration():
    """A and B against all 2^12 paths, sites and Mb: the whole data (two chromosomes), the
    chromosomes, regions inside a chromosome, across the chromosome start and of one site; a
    missing cell, a called heterozygote whose IBD state is excluded (exact zeros at that cell)."""
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    ca, cb = lu.cells_a(e, pos, F, A), lu.cells_b(e, pos, F, A)
    worst = 0.0
    for unit, L in bu.SMALL_LEN.items():
        for tag, reg in _small_sets(S).items():
            want = lu.enumerate_longest(e, pos, F, A, L, unit, reg)
            np.testing.assert_allclose(want["p_any"] + want["p_none"], 1.0, rtol=0, atol=ENUM_ATOL)
            for name, rec in (("A", lu.records_a(ca, pos, L, unit, reg)), ("B", lu.records_b(cb, pos, L, unit, reg))):
                for f in lu.FIELDS:
                    assert np.isfinite(rec[f]).all(), (name, unit, tag, f)
                    worst = max(worst, np.abs(rec[f] - want[f]).max())
                    np.testing.assert_allclose(rec[f], want[f], rtol=0, atol=ENUM_ATOL, err_msg=f"{name} {unit} {tag} {f}")
                if tag == "single":   # no run on the excluded cell, exactly
                    assert (rec["p_any"][1, 4] == 0.0).all() and (rec["p_none"][1, 4] == 1.0).all(), (name, unit)
    print(f"\n  yardsticks against enumeration: largest difference {worst:.2e}")


def test_identities_on_the_yardsticks():
    """At L = 1 site and at 0 Mb a one-site region gives p_any = pi_s(1) and p_none = pi_s(0); p_any
    is non-increasing in k and at most ibd_by_length's expected number of tracts cut at the
    region's edges -- over whole chromosomes bylength_util's own; p_any + p_none = 1;
    longest_classes adds up to 1."""
    from importlib import import_module
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    post = xu.terms_b(e, pos, F, A)["ibd"]
    ca, cb = lu.cells_a(e, pos, F, A), lu.cells_b(e, pos, F, A)
    one = xu.single_site_regions(S)
    for unit, L in bu.SMALL_LEN.items():
        tr = bu.region_records(bu.terms_b(e, pos, F, A, L, unit), np.array([[0, 7], [7, S]]))["tracts"]
        for rec_fn, cells in ((lu.records_a, ca), (lu.records_b, cb)):
            r1 = rec_fn(cells, pos, L, unit, one)
            np.testing.assert_allclose(r1["p_any"][..., 0], post, rtol=0, atol=ENUM_ATOL)
            np.testing.assert_allclose(r1["p_none"][..., 0], 1 - post, rtol=0, atol=ENUM_ATOL)
            for tag, reg in _small_sets(S).items():
                rec = rec_fn(cells, pos, L, unit, reg)
                assert (np.diff(rec["p_any"], axis=-1) <= ENUM_ATOL).all(), (unit, tag)
                np.testing.assert_allclose(rec["p_any"] + rec["p_none"], 1.0, rtol=0, atol=ENUM_ATOL)
                assert (rec["p_any"] >= 0).all() and (rec["p_none"] >= 0).all()
                if tag == "chrom":
                    assert (rec["p_any"] <= tr + ENUM_ATOL).all(), unit
                cls = import_module("ngsf-hmm_amd").longest_classes(rec)
                assert cls.shape == rec.shape[:-1] + (len(L) + 1,)
                np.testing.assert_allclose(cls.sum(axis=-1), 1.0, rtol=0, atol=ENUM_ATOL)
                assert (cls >= -ENUM_ATOL).all()


def _cohort(pkg):
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    return d, su.emissions_np(gl, np.full(d.n_sites, freq)), F, A


def test_yardstick_spread_on_the_gpu_cohort(pkg):
    """|A - B| per unit and field on the cohort, thresholds and region sets of the GPU test
    (printed; longest_util.SPREAD holds the figures, and the GPU tolerance is 16 x them).  To
    re-measure: pytest -s tests/test_longest_cpu.py -k spread, and copy the printed maxima."""
    d, e, F, A = _cohort(pkg)
    pos = d.pos_dist_mb
    ca, cb = lu.cells_a(e, pos, F, A), lu.cells_b(e, pos, F, A)
    for unit, L in bu.COHORT_LEN.items():
        worst = {f: 0.0 for f in lu.FIELDS}
        for name, reg in xu.region_sets(d.n_sites, pos, xu.SPREAD_LANE_SITES).items():
            a, b = lu.records_a(ca, pos, L, unit, reg), lu.records_b(cb, pos, L, unit, reg)
            assert all(np.isfinite(x[f]).all() for x in (a, b) for f in lu.FIELDS), (unit, name)
            s = lu.spread(a, b)
            worst = {f: max(worst[f], s[f]) for f in worst}
            if unit == "sites":   # 2000 sites exceed every chromosome: exactly nothing
                assert (a["p_any"][..., -1] == 0).all() and (b["p_any"][..., -1] == 0).all()
        print(f"\n  spread |A - B| in {unit}: " + ", ".join(f"{f} {worst[f]:.3e}" for f in worst))
        # what the GPU test uses is what is measured here (within a factor of two: libm versions)
        for f in worst:
            assert 0 < lu.SPREAD[unit][f] and worst[f] <= 2 * lu.SPREAD[unit][f], (unit, f, worst[f])
    # far inside the project's own bound on posteriors (1e-9 per site)
    assert max(max(t.values()) for t in lu.TOL.values()) <= 1e-9


def test_sampler_condition_on_the_gpu_cohort(pkg):
    """The restatement of the sampler (sample_util) against yardstick B on the GPU test's cohort,
    draws and seed, at the thresholds SAMPLER_LEN: the condition that test relies on holds before
    the device is asked."""
    d, e, F, A = _cohort(pkg)
    pos = d.pos_dist_mb
    f = su.forward_filter(e, pos, F, A)
    thr = su.thresholds(f, pos, F, A)
    u = su.uniforms(xu.SAMPLER_SEED, range(xu.SAMPLER_DRAWS), d.n_ind, d.n_sites)
    paths = su.backward_draw(thr, u)
    cb = lu.cells_b(e, pos, F, A)
    for unit, L in bu.SAMPLER_LEN.items():
        exact = lu.records_b(cb, pos, L, unit, [[0, d.n_sites]])["p_any"][:, 0]
        worst = lu.sampler_check(lu.path_longest(paths, pos, unit), exact, L, unit)
        print(f"\n  sampler restatement against yardstick B in {unit}: largest |z| = {worst:.2f}")


def test_record_mirrors_the_header(pkg):
    import ctypes as C
    import re
    assert C.sizeof(pkg.hmm.LongestStat) == 16
    assert list(pkg.LONGEST_DTYPE.names) == list(lu.FIELDS)
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    body = re.search(r"typedef struct nghmm_longest_stat \{(.*?)\} nghmm_longest_stat;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == list(lu.FIELDS)
    assert int(re.search(r"NGHMM_LONGEST_MB = (\d+)", header).group(1)) == pkg.LONGEST_MB == 1
    rec = np.zeros((2, 3), dtype=pkg.LONGEST_DTYPE)
    rec["p_any"], rec["p_none"] = [[0.75, 0.5, 0.125]] * 2, [[0.25, 0.5, 0.875]] * 2
    assert np.array_equal(pkg.longest_classes(rec), [[0.25, 0.25, 0.375, 0.125]] * 2)


@pytest.fixture(scope="module")
def asan_longest_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp with and without the entries of tests/stub/nghmm_longest_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_longest")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_longest_stub.cpp")), ("without", ("nghmm_stub.cpp",))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "%.10g" % v


def test_ibd_longest_writer_under_address_sanitizer(pkg, tmp_path, asan_longest_host):
    """--ibd_longest writes PREFIX.ibd.longest: the header, one line per individual, chromosome (or
    window that restarts at every chromosome) and threshold in that order, the stub's formulas as
    %.10g; Mb by default and sites with --longest_sites; default IDs and --ind_names, one handle or
    a chain of three, multi-start replicates (the winning one's only); without the flag the file
    does not appear and the other files are byte-identical; the other two flags alone are a
    warning; bad threshold lists are refused; a library without the entry still links and stops
    the run with a message."""
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
        ("window", ["--longest_window", 40, "--ind_names", tmp_path / "names.txt"], 40, names, "1,2,30", True),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--longest_window", 7,
                   "--ind_names", tmp_path / "names.txt"], 7, names, "0.5", False),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], 0, None, "1,2,3,4,5,6,7,8", True),
    ]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    for tag, extra, window, ids, lens, in_sites in runs:
        plain, ex = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"ex_{tag}")
        unit = ["--longest_sites"] if in_sites else []
        r = run(asan_longest_host["full"], plain, extra + unit)
        assert ("are only used by --ibd_longest" in r.stderr) == (window > 0 or in_sites)
        run(asan_longest_host["full"], ex, extra + unit + ["--ibd_longest", lens])
        ids = ids or [f"ind{i}" for i in range(I)]
        regions = summary_util.chrom_regions(chrom, window)
        L = [float(x) for x in lens.split(",")]
        want = ["ind\tchr\tfirst_pos\tlast_pos\tn_sites\tmin_len\tp_any\tp_none"]
        for i in range(I):
            for a, b in regions:
                a, b = int(a), int(b)
                for k, l in enumerate(L):
                    want.append("\t".join([ids[i], chrom[a], str(pos[a]), str(pos[b - 1]), str(b - a), _g10(l),
                                           _g10((1.0 + i) / ((2.0 + i + a) * (1.0 + l))),
                                           _g10((0.25 if in_sites else 0.5) / (k + 1) + 1e-7 * (b - a) + 1e-9 * i)]))
        got = open(ex + ".ibd.longest").read()
        assert got == "\n".join(want) + "\n", tag
        assert got.count("\n") == 1 + I * len(regions) * len(L)
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(ex + ext, "rb").read(), (tag, ext)
        made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                                  if f.startswith(os.path.basename(pre) + "."))
        new = [e for e in made(ex) if e not in made(plain)]
        assert all(e.endswith(".ibd.longest") for e in new), (tag, new)
        assert len(new) == (2 if tag == "starts" else 1)          # (the winning replicate's only)
    for lens, unit in (("", []), ("1,,2", []), ("1,x", []), ("2,1", []), ("1,1", []), ("-1,2", []),
                       ("0.5,2", ["--longest_sites"]), ("0,1", ["--longest_sites"]),
                       ("1,2,3,4,5,6,7,8,9", []), ("inf", []), ("nan", [])):
        r = run(asan_longest_host["full"], str(tmp_path / "bad"), unit + ["--ibd_longest", lens], ok=False)
        assert "invalid --ibd_longest" in r.stderr, (lens, r.stderr[-500:])
    r = run(asan_longest_host["full"], str(tmp_path / "bad"), ["--ibd_longest", "1", "--longest_window", 0], ok=False)
    assert "invalid --longest_window" in r.stderr
    r = run(asan_longest_host["without"], str(tmp_path / "none"), ["--ibd_longest", "1"], ok=False)
    assert "--ibd_longest: the library has no nghmm_chain_ibd_longest!" in r.stderr
    run(asan_longest_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_chrom") + ext, "rb").read(), ext
