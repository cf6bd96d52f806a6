"""Expected IBD above a minimum tract length without a GPU: the two numpy yardsticks of
tests/bylength_util.py against brute-force enumeration, the identities of include/nghmm.h
(nghmm_ibd_by_length) against expect_util's yardstick, their spread on the cohort of
tests/test_gpu_bylength.py (the figure that test's tolerance is made of), on the same cohort the
condition under which that test compares the exact means with sampled paths; and the host's
--ibd_by_length writer, a program of its own under AddressSanitizer / UBSan, against the CPU
stand-in of the library (tests/stub/)."""
import os
import subprocess

import numpy as np
import pytest

import bylength_util as bu
import cli_util
import expect_util as xu
import summary_util
import sample_util as su
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The yardsticks against enumeration: sums of at most 12 terms of order 1 (lengths of order 10
# sites, 3 Mb), each a product of at most 12 factors: a few hundred roundings of 1.1e-16 at the
# worst.  The same bound as test_expect_cpu.py's.
ENUM_ATOL = 2e-13


def test_yardsticks_equal_enumeration():
    """A and B against all 2^12 paths for the whole data, sites and Mb: two chromosomes, a missing
    cell, a called heterozygote whose IBD state is excluded (exact zeros at that cell)."""
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    whole, one = np.array([[0, S]]), xu.single_site_regions(S)
    worst = 0.0
    for unit, L in bu.SMALL_LEN.items():
        want_tr, want_ln = bu.enumerate_by_length(e, pos, F, A, L, unit)
        for name, fn in (("A", bu.terms_a), ("B", bu.terms_b)):
            t = fn(e, pos, F, A, L, unit)
            assert np.isfinite(t[0]).all() and np.isfinite(t[1]).all(), (name, unit)
            assert (t[0][1, 4] == 0.0).all() and (t[1][1, 4] == 0.0).all(), "no tract begins in the excluded state"
            rec = bu.region_records(t, whole)
            worst = max(worst, np.abs(rec["tracts"][:, 0] - want_tr).max(), np.abs(rec["length"][:, 0] - want_ln).max())
            np.testing.assert_allclose(rec["tracts"][:, 0], want_tr, rtol=0, atol=ENUM_ATOL, err_msg=f"{name} {unit}")
            np.testing.assert_allclose(rec["length"][:, 0], want_ln, rtol=0, atol=ENUM_ATOL, err_msg=f"{name} {unit}")
            # regions that partition the data add up to the whole
            r1 = bu.region_records(t, one)
            for f in bu.FIELDS:
                np.testing.assert_allclose(r1[f].sum(axis=1), rec[f][:, 0], rtol=0, atol=ENUM_ATOL)
    print(f"\n  yardsticks against enumeration: largest difference {worst:.2e}")
    # a step into the excluded state is blocked in both
    _, rho = bu.cells_a(e, pos, F, A)
    _, lrho = bu.cells_b(e, pos, F, A)
    assert rho[1, 4] == 0.0 and np.isneginf(lrho[1, 4])
    assert np.array_equal(rho == 0.0, np.isneginf(lrho))


def test_identities_against_the_expectations():
    """With L = 1 site tracts is ibd_expect's starts per region and, over whole chromosomes, length
    its ibd; with L = 0 Mb length is its ibd_mb; both fields are non-increasing in k and
    length >= L_k tracts."""
    e, pos, F, A, _, _, _ = xu.small_case()
    S = e.shape[1]
    ex = xu.terms_b(e, pos, F, A)
    sets = {"whole": np.array([[0, S]]), "chrom": np.array([[0, 7], [7, S]]), "single": xu.single_site_regions(S)}
    for fn in (bu.terms_a, bu.terms_b):
        ts, tm = fn(e, pos, F, A, bu.SMALL_LEN["sites"], "sites"), fn(e, pos, F, A, bu.SMALL_LEN["mb"], "mb")
        for name, reg in sets.items():
            want = xu.region_records(ex, reg)
            rs, rm = bu.region_records(ts, reg), bu.region_records(tm, reg)
            np.testing.assert_allclose(rs["tracts"][..., 0], want["starts"], rtol=0, atol=ENUM_ATOL)
            np.testing.assert_allclose(rm["tracts"][..., 0], want["starts"], rtol=0, atol=ENUM_ATOL)
            if name != "single":
                np.testing.assert_allclose(rs["length"][..., 0], want["ibd"], rtol=0, atol=ENUM_ATOL)
                np.testing.assert_allclose(rm["length"][..., 0], want["ibd_mb"], rtol=0, atol=ENUM_ATOL)
            for rec, L in ((rs, bu.SMALL_LEN["sites"]), (rm, bu.SMALL_LEN["mb"])):
                for f in bu.FIELDS:
                    assert (np.diff(rec[f], axis=-1) <= ENUM_ATOL).all(), (name, f)
                assert (rec["length"] >= np.asarray(L) * rec["tracts"] - ENUM_ATOL).all(), name


def _cohort(pkg):
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    return d, su.emissions_np(gl, np.full(d.n_sites, freq)), F, A


def test_yardstick_spread_on_the_gpu_cohort(pkg):
    """|A - B| per unit and field on the cohort, thresholds and region sets of the GPU test
    (printed; bylength_util.SPREAD holds the figures, and the GPU tolerance is 16 x them).  To
    re-measure: pytest -s tests/test_bylength_cpu.py -k spread, and copy the printed maxima."""
    d, e, F, A = _cohort(pkg)
    pos = d.pos_dist_mb
    for unit, L in bu.COHORT_LEN.items():
        ta, tb = bu.terms_a(e, pos, F, A, L, unit), bu.terms_b(e, pos, F, A, L, unit)
        assert all(np.isfinite(x).all() for x in ta + tb), unit
        worst = {f: 0.0 for f in bu.FIELDS}
        for name, reg in xu.region_sets(d.n_sites, pos, xu.SPREAD_LANE_SITES).items():
            a, b = bu.region_records(ta, reg), bu.region_records(tb, reg)
            s = bu.spread(a, b)
            worst = {f: max(worst[f], s[f]) for f in worst}
            if unit == "sites":   # 2000 sites exceed every chromosome: exactly nothing
                assert (a["tracts"][..., -1] == 0).all() and (b["length"][..., -1] == 0).all()
        print(f"\n  spread |A - B| in {unit}: " + ", ".join(f"{f} {worst[f]:.3e}" for f in worst))
        # what the GPU test uses is what is measured here (within a factor of two: libm versions)
        for f in worst:
            assert 0 < bu.SPREAD[unit][f] and worst[f] <= 2 * bu.SPREAD[unit][f], (unit, f, worst[f])
    # far inside the project's own bound on posteriors (1e-9 per site) for a region of any length
    assert max(max(t.values()) for t in bu.TOL.values()) <= 1e-9 * 7


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
    for unit, L in bu.SAMPLER_LEN.items():
        exact = bu.region_records(bu.terms_b(e, pos, F, A, L, unit), [[0, d.n_sites]])[:, 0]
        tr, ln = bu.path_by_length(paths, pos, L, unit)
        worst = bu.sampler_check(tr, ln, exact, unit)
        print(f"\n  sampler restatement against yardstick B in {unit}: largest |z| = {worst:.2f}")


def test_record_mirrors_the_header(pkg):
    import ctypes as C
    import re
    hm = pkg.hmm
    assert C.sizeof(hm.ByLengthStat) == 16
    assert list(pkg.BYLENGTH_DTYPE.names) == list(bu.FIELDS)
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    body = re.search(r"typedef struct nghmm_bylength_stat \{(.*?)\} nghmm_bylength_stat;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == list(bu.FIELDS)
    assert int(re.search(r"NGHMM_BYLENGTH_MB = (\d+)", header).group(1)) == pkg.BYLENGTH_MB == 1
    rec = np.zeros((2, 3), dtype=pkg.BYLENGTH_DTYPE)
    rec["tracts"], rec["length"] = [[5, 2, 2]] * 2, [[30, 24, 24]] * 2
    cls = pkg.by_length_classes(rec)
    assert np.array_equal(cls["tracts"], [[3, 0, 2]] * 2) and np.array_equal(cls["length"], [[6, 0, 24]] * 2)
    assert np.array_equal(cls["mean_length"], [[2, np.nan, 12]] * 2, equal_nan=True)


@pytest.fixture(scope="module")
def asan_bylength_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp with and without the entries of tests/stub/nghmm_bylength_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_bylength")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_bylength_stub.cpp")), ("without", ("nghmm_stub.cpp",))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "%.10g" % v


def test_ibd_by_length_writer_under_address_sanitizer(pkg, tmp_path, asan_bylength_host):
    """--ibd_by_length writes PREFIX.ibd.bylength: the header, one line per individual, chromosome
    (or window that restarts at every chromosome) and threshold in that order, the stub's formulas
    as %.10g; Mb by default and sites with --by_length_sites; default IDs and --ind_names, one
    handle or a chain of three, multi-start replicates (the winning one's only); without the flag
    the file does not appear and the other files are byte-identical; the other two flags alone are
    a warning; bad threshold lists are refused; a library without the entry still links and stops
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
        ("window", ["--by_length_window", 40, "--ind_names", tmp_path / "names.txt"], 40, names, "1,2,30", True),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--by_length_window", 7,
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
        unit = ["--by_length_sites"] if in_sites else []
        r = run(asan_bylength_host["full"], plain, extra + unit)
        assert ("are only used by --ibd_by_length" in r.stderr) == (window > 0 or in_sites)
        run(asan_bylength_host["full"], ex, extra + unit + ["--ibd_by_length", lens])
        ids = ids or [f"ind{i}" for i in range(I)]
        regions = summary_util.chrom_regions(chrom, window)
        L = [float(x) for x in lens.split(",")]
        want = ["ind\tchr\tfirst_pos\tlast_pos\tn_sites\tmin_len\texp_tracts\texp_len"]
        for i in range(I):
            for a, b in regions:
                a, b = int(a), int(b)
                for k, l in enumerate(L):
                    want.append("\t".join([ids[i], chrom[a], str(pos[a]), str(pos[b - 1]), str(b - a), _g10(l),
                                           _g10((1.0 + i) / ((1.0 + a) * (1.0 + l))),
                                           _g10((0.25 if in_sites else 1e-3) * (b - a) / (k + 1) + 1e-7 * i)]))
        got = open(ex + ".ibd.bylength").read()
        assert got == "\n".join(want) + "\n", tag
        assert got.count("\n") == 1 + I * len(regions) * len(L)
        if window:       # the windows restart at every chromosome
            first = {c: chrom.index(c) for c in set(chrom)}
            assert {int(a) for a, _ in regions} >= set(first.values())
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(ex + ext, "rb").read(), (tag, ext)
        made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                                  if f.startswith(os.path.basename(pre) + "."))
        new = [e for e in made(ex) if e not in made(plain)]
        assert all(e.endswith(".ibd.bylength") for e in new), (tag, new)
        assert len(new) == (2 if tag == "starts" else 1)          # (the winning replicate's only)
    for lens, unit in (("", []), ("1,,2", []), ("1,x", []), ("2,1", []), ("1,1", []), ("-1,2", []),
                       ("0.5,2", ["--by_length_sites"]), ("0,1", ["--by_length_sites"]),
                       ("1,2,3,4,5,6,7,8,9", []), ("inf", []), ("nan", [])):
        r = run(asan_bylength_host["full"], str(tmp_path / "bad"), unit + ["--ibd_by_length", lens], ok=False)
        assert "invalid --ibd_by_length" in r.stderr, (lens, r.stderr[-500:])
    r = run(asan_bylength_host["full"], str(tmp_path / "bad"), ["--ibd_by_length", "1", "--by_length_window", 0],
            ok=False)
    assert "invalid --by_length_window" in r.stderr
    r = run(asan_bylength_host["without"], str(tmp_path / "none"), ["--ibd_by_length", "1"], ok=False)
    assert "--ibd_by_length: the library has no nghmm_chain_ibd_by_length!" in r.stderr
    run(asan_bylength_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_chrom") + ext, "rb").read(), ext
