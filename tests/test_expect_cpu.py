"""Path expectations without a GPU: the two numpy yardsticks of tests/expect_util.py against
brute-force enumeration, the identities of include/nghmm.h (nghmm_ibd_expect), and their spread on
the cohort of tests/test_gpu_expect.py (the figure that test's tolerance is made of), and on the
same cohort the condition under which that test compares the exact means with sampled paths; and
the host's --ibd_expect writers, a program of its own under AddressSanitizer / UBSan, against the
CPU stand-in of the library (tests/stub/)."""
import math
import os
import subprocess

import numpy as np
import pytest

import cli_util
import expect_util as xu
import summary_util
import sample_util as su
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, tag, atol=2e-13):
    assert not np.isnan(got).any(), tag
    known = ~np.isnan(want)            # (enumerate_expect: lp of a step out of an excluded state)
    got, want = got[known], want[known]
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), (tag, "-inf exactly where enumeration has it")
    np.testing.assert_allclose(got[~inf], want[~inf], rtol=0, atol=atol, err_msg=tag)


def test_yardsticks_equal_enumeration():
    """A and B against all 2^12 paths: per single-site region (every cell's terms) and for the whole
    data; two chromosomes, a missing cell, a called heterozygote whose IBD state is excluded -- its
    xi entries are exactly 0, and the path of individual 1, which goes through it, has -inf."""
    e, pos, F, A, path, _, _ = xu.small_case()
    S = e.shape[1]
    assert np.isneginf(e[1, 4, 1]), "the restatement carries the exact zero"
    tot, want = xu.enumerate_expect(e, pos, F, A, path)
    assert np.isneginf(tot["log_p_path"][1]) and np.isfinite(tot["log_p_path"][[0, 2]]).all()
    assert np.isnan(want["lp"]).sum() == 1 and np.isnan(want["lp"][1, 5]) and np.isneginf(want["lp"][1, 4])
    one, whole = xu.single_site_regions(S), np.array([[0, S]])
    for name, fn in (("A", xu.terms_a), ("B", xu.terms_b)):
        got = fn(e, pos, F, A, path)
        for t in xu.TERMS:
            _close(got[t], want[t], f"{name} {t}")
            assert not np.isnan(got[t]).any()
        assert got["ibd"][1, 4] == 0.0 and got["start"][1, 4] == 0.0 and got["on"][1, 4] == 0.0
        assert (got["h"] >= 0).all()
        rec1, recw = xu.region_records(got, one), xu.region_records(got, whole)
        w1 = xu.region_records(want, one)
        for f in xu.REGION_FIELDS:
            _close(rec1[f], w1[f], f"{name} single-site {f}")
        # the identities, against statistics of the enumerated paths themselves
        for f, k in (("starts", "n_tracts"), ("ibd", "ibd_sites"), ("ibd_mb", "ibd_mb"),
                     ("switches", "switches"), ("entropy", "entropy"), ("log_p_path", "log_p_path")):
            _close(recw[f][:, 0], tot[k], f"{name} whole {f}", atol=1e-12)
        # regions that partition the data add up to the whole
        for f in xu.REGION_FIELDS:
            fin = np.isfinite(recw[f][:, 0])
            np.testing.assert_allclose(rec1[f].sum(axis=1)[fin], recw[f][fin, 0], rtol=0, atol=1e-12)
        sites = xu.site_records(got)
        np.testing.assert_allclose(sites["ibd"], want["ibd"].sum(axis=0), rtol=0, atol=1e-12)
    # without a path the last field is 0
    assert (xu.region_records(xu.terms_b(e, pos, F, A), whole)["log_p_path"] == 0).all()


def test_pair_marginals_add_up_to_the_posterior():
    """xi(0, 1) + xi(1, 1) = pi(1): ibd_s against the per-site posterior of sample_util; on a
    start-free site start_s + xi(1, 1) = pi(1)."""
    e, pos, F, A, path, _, _ = xu.small_case()
    f = su.forward_filter(e, pos, F, A)
    post = su.posterior(f, e, pos, F, A)
    cs = xu.chrom_start(pos)
    for fn in (xu.terms_a, xu.terms_b):
        t = fn(e, pos, F, A, path)
        np.testing.assert_allclose(t["ibd"], post, rtol=0, atol=1e-14)
        d = np.where(np.isinf(pos), 1.0, pos)
        np.testing.assert_allclose((t["on"] + t["mb"] / d)[:, ~cs], post[:, ~cs], rtol=0, atol=1e-14)


def _cohort_terms(pkg):
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    tb = xu.terms_b(e, d.pos_dist_mb, F, A)
    path = (tb["ibd"] >= 0.5).astype(np.uint8)
    return d, e, F, A, path


def test_yardstick_spread_on_the_gpu_cohort(pkg):
    """|A - B| per field on the cohort and region sets of the GPU test (printed;
    expect_util.REGION_SPREAD / SITE_SPREAD hold the figures, and the GPU tolerance is 16 x them).
    To re-measure: pytest -s tests/test_expect_cpu.py -k spread, and copy the printed maxima."""
    d, e, F, A, path = _cohort_terms(pkg)
    pos = d.pos_dist_mb
    ta, tb = xu.terms_a(e, pos, F, A, path), xu.terms_b(e, pos, F, A, path)
    for t in xu.TERMS:
        assert not np.isnan(ta[t]).any() and not np.isnan(tb[t]).any(), t
    worst = {f: 0.0 for f in xu.REGION_FIELDS}
    for name, reg in xu.region_sets(d.n_sites, pos, xu.SPREAD_LANE_SITES).items():
        a, b = xu.region_records(ta, reg), xu.region_records(tb, reg)
        assert np.isfinite(b["log_p_path"]).all(), name
        s = xu.spread(a, b)
        worst = {f: max(worst[f], s[f]) for f in worst}
    ws = xu.spread(xu.site_records(ta), xu.site_records(tb))
    print("\n  region spread |A - B|: " + ", ".join(f"{f} {worst[f]:.3e}" for f in worst))
    print("  site spread   |A - B|: " + ", ".join(f"{f} {ws[f]:.3e}" for f in ws))
    # what the GPU test uses is what is measured here (within a factor of two: libm versions)
    for f in worst:
        assert 0 < xu.REGION_SPREAD[f] and worst[f] <= 2 * xu.REGION_SPREAD[f], (f, worst[f])
    for f in ws:
        assert 0 < xu.SITE_SPREAD[f] and ws[f] <= 2 * xu.SITE_SPREAD[f], (f, ws[f])
    # far inside the project's own bound on posteriors (1e-9 per site) for a region of any length
    assert max(xu.REGION_TOL.values()) <= 1e-9 * 7 and max(xu.SITE_TOL.values()) <= 1e-9 * d.n_ind


def test_sampler_condition_on_the_gpu_cohort(pkg):
    """The restatement of the sampler (sample_util) against yardstick B on the GPU test's cohort,
    draws and seed: the condition that test relies on holds before the device is asked."""
    d, e, F, A, _ = _cohort_terms(pkg)
    pos = d.pos_dist_mb
    f = su.forward_filter(e, pos, F, A)
    thr = su.thresholds(f, pos, F, A)
    u = su.uniforms(xu.SAMPLER_SEED, range(xu.SAMPLER_DRAWS), d.n_ind, d.n_sites)
    stats = su.path_stats(su.backward_draw(thr, u), pos)
    exact = xu.region_records(xu.terms_b(e, pos, F, A), [[0, d.n_sites]])[:, 0]
    worst = xu.sampler_check(stats, exact)
    print(f"\n  sampler restatement against yardstick B: largest |z| = {worst:.2f}")


def test_records_mirror_the_header(pkg):
    import ctypes as C
    import re
    hm = pkg.hmm
    assert C.sizeof(hm.ExpectRegion) == 48 and C.sizeof(hm.ExpectSite) == 32
    assert list(pkg.EXPECT_REGION_DTYPE.names) == list(xu.REGION_FIELDS)
    assert list(pkg.EXPECT_SITE_DTYPE.names) == list(xu.SITE_FIELDS)
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    for name, fields in (("nghmm_expect_region", xu.REGION_FIELDS), ("nghmm_expect_site", xu.SITE_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*[,;]", body) == list(fields)
    assert int(re.search(r"NGHMM_EXPECT_VITERBI = (\d+)", header).group(1)) == pkg.EXPECT_VITERBI == 1
    rec = np.zeros((2, 3), dtype=pkg.EXPECT_REGION_DTYPE)
    rec["ibd"], rec["ibd_mb"] = [[4, 0, 9]] * 2, [[1, 0, 3]] * 2
    rec["starts"] = [[2, 0, 3]] * 2
    sites, mb = pkg.expect_tract_length(rec)
    assert np.array_equal(sites, [[2, np.nan, 3]] * 2, equal_nan=True)
    assert np.array_equal(mb, [[0.5, np.nan, 1]] * 2, equal_nan=True)


@pytest.fixture(scope="module")
def asan_expect_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp with and without the entries of tests/stub/nghmm_expect_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_expect")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_expect_stub.cpp")), ("without", ("nghmm_stub.cpp",))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "-inf" if v == -math.inf else "%.10g" % v


def test_ibd_expect_writers_under_address_sanitizer(pkg, tmp_path, asan_expect_host):
    """--ibd_expect writes PREFIX.ibd.expect and PREFIX.ibd.breaks: the headers, one line per
    individual and chromosome (or window that restarts at every chromosome) and one per site, the
    stub's formulas as %.10g with -inf written as -inf; default IDs and --ind_names, one handle or
    a chain of three, multi-start replicates (the winning one's only); without the flag neither
    file appears and the other files are byte-identical; --expect_window alone is a warning; a
    library without the entry stops the run with a message."""
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
        ("chrom", [], 0, None),
        ("window", ["--expect_window", 40, "--ind_names", tmp_path / "names.txt"], 40, names),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--expect_window", 7,
                   "--ind_names", tmp_path / "names.txt"], 7, names),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], 0, None),
    ]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    n_inf = 0
    for tag, extra, window, ids in runs:
        plain, ex = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"ex_{tag}")
        r = run(asan_expect_host["full"], plain, extra)
        assert ("--expect_window is only used by --ibd_expect" in r.stderr) == (window > 0)
        run(asan_expect_host["full"], ex, extra + ["--ibd_expect"])
        ids = ids or [f"ind{i}" for i in range(I)]
        regions = summary_util.chrom_regions(chrom, window)
        want = ["ind\tchr\tfirst_pos\tlast_pos\tn_sites\texp_ibd_sites\texp_tracts\texp_switches\t"
                "exp_ibd_mb\tentropy\tlog10_p_path"]
        for i in range(I):
            for a, b in regions:
                a, b = int(a), int(b)
                n = b - a
                lp = -math.inf if a % 7 == 0 else (-n / 8.0 - i) / math.log(10.0)
                n_inf += a % 7 == 0
                want.append("\t".join([ids[i], chrom[a], str(pos[a]), str(pos[b - 1]), str(n),
                                       _g10(0.25 * n + i), _g10(1.0 / (1.0 + a)), _g10(2.0 / (1.0 + a)),
                                       _g10(0.001 * n), _g10(1e-12 * (i + 1) * n), _g10(lp)]))
        assert open(ex + ".ibd.expect").read() == "\n".join(want) + "\n", tag
        want = ["chr\tpos\ton\toff\tibd\tentropy"]
        for s in range(S):
            want.append("\t".join([chrom[s], str(pos[s]), _g10(1.0 / (s + 2)), _g10(1.0 / (s + 3)),
                                   _g10(0.5 * I), _g10(1e-3 * s)]))
        assert open(ex + ".ibd.breaks").read() == "\n".join(want) + "\n", tag
        if window:       # the windows restart at every chromosome
            first = {c: chrom.index(c) for c in set(chrom)}
            assert all(int(a) in first.values() or chrom[int(a)] == chrom[int(a) - 1] for a, _ in regions)
            assert {int(a) for a, _ in regions} >= set(first.values())
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(ex + ext, "rb").read(), (tag, ext)
        made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                                  if f.startswith(os.path.basename(pre) + "."))
        new = [e for e in made(ex) if e not in made(plain)]
        assert all(e.endswith((".ibd.expect", ".ibd.breaks")) for e in new), (tag, new)
        assert len(new) == (4 if tag == "starts" else 2)          # (the winning replicate's only)
    assert n_inf > 5
    r = run(asan_expect_host["full"], str(tmp_path / "bad"), ["--ibd_expect", "--expect_window", 0], ok=False)
    assert "invalid --expect_window" in r.stderr
    r = run(asan_expect_host["without"], str(tmp_path / "none"), ["--ibd_expect"], ok=False)
    assert "--ibd_expect: the library has no nghmm_chain_ibd_expect!" in r.stderr
    run(asan_expect_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_chrom") + ext, "rb").read(), ext
