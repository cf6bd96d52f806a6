"""Posterior moments of IBD share and tract count without a GPU: the two numpy yardsticks of
tests/moments_util.py against brute-force enumeration, their spread on the cohorts of
tests/test_gpu_moments.py (the figures that test's tolerances are made of), the condition under
which that test compares the exact variances with sampled paths, the records against the header;
and the host's --ibd_moments writer, a program of its own under AddressSanitizer / UBSan, against
the CPU stand-in of the library (tests/stub/)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cli_util
import expect_util as xu
import moments_util as mu
import sample_util as su
import summary_util
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yardsticks_equal_enumeration():
    """A and B against all 2^12 paths on the 3 x 12 case (two chromosomes, a missing cell, an
    excluded state): the whole data, each chromosome, [3, 9) across the chromosome start, every
    single site; both lengths.  The float64 enumeration's own sums of 4096 terms are good to about
    1e-14 (variances of the order of 1)."""
    e, pos, F, A, _, _, _ = xu.small_case()
    sets = mu.small_regions()
    assert np.isinf(pos[7]) and sets["mid"][0, 0] < 7 < sets["mid"][0, 1]
    for L in mu.LENGTHS:
        a = mu.moments_a(e, pos, F, A, list(sets.values()), L)
        b = mu.moments_b(e, pos, F, A, list(sets.values()), L)
        for k, (name, reg) in enumerate(sets.items()):
            want = mu.enumerate_moments(e, pos, F, A, reg, L)
            for tag, got in (("A", a[k]), ("B", b[k])):
                for f in mu.FIELDS:
                    assert np.isfinite(got[f]).all(), (L, name, tag, f)
                    np.testing.assert_allclose(got[f], want[f], rtol=0, atol=2e-14, err_msg=f"{L} {name} {tag} {f}")
        cells = b[list(sets).index("cells")]
        # the excluded state: a one-site region with variance exactly 0
        assert cells["var_a"][1, 4] == 0.0 and cells["var_t"][1, 4] == 0.0 and cells["mean_a"][1, 4] == 0.0
        if L == "sites":       # a one-site region: mean pi, variance pi (1 - pi)
            pi = cells["mean_a"]
            np.testing.assert_allclose(cells["var_a"], pi * (1 - pi), rtol=0, atol=1e-15)
        # chromosomes are independent: their covariance matrices add up to the whole data's
        chrom, whole = b[list(sets).index("chrom")], b[list(sets).index("whole")]
        for f in mu.FIELDS:
            np.testing.assert_allclose(chrom[f].sum(axis=1), whole[f][:, 0], rtol=0, atol=1e-14)


def _cohort(pkg):
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    return d, su.emissions_np(gl, np.full(d.n_sites, freq)), F, A


def _worst(a, b):
    worst = {f: 0.0 for f in mu.FIELDS}
    for x, y in zip(a, b):
        s = mu.spread(x, y)
        worst = {f: max(worst[f], s[f]) for f in worst}
    return worst


@pytest.fixture(scope="module")
def cohort_b(pkg):
    """Yardstick B on the cohort over all region sets, both lengths (shared: one pass each)."""
    d, e, F, A = _cohort(pkg)
    sets = xu.region_sets(d.n_sites, d.pos_dist_mb, mu.SPREAD_LANE_SITES)
    return sets, {L: mu.moments_b(e, d.pos_dist_mb, F, A, list(sets.values()), L) for L in mu.LENGTHS}


def test_yardstick_spread_on_the_gpu_cohorts(pkg, cohort_b):
    """|A - B| per length and field on the 20 x 5003 cohort over all the region sets of the GPU
    test, and on the confident chain over its two regions (printed; moments_util.COHORT_SPREAD /
    CONFIDENT_SPREAD hold the figures, and the GPU tolerances are 16 x them).
    To re-measure: pytest -s tests/test_moments_cpu.py -k spread, and copy the printed maxima."""
    d, e, F, A = _cohort(pkg)
    sets, b = cohort_b
    print()
    for L in mu.LENGTHS:
        a = mu.moments_a(e, d.pos_dist_mb, F, A, list(sets.values()), L)
        worst = _worst(a, b[L])
        print(f"  cohort    {L:5s} spread |A - B|: " + ", ".join(f"{f} {worst[f]:.3e}" for f in worst))
        for f in worst:     # what the GPU test uses is what is measured here (a factor of two: libm versions)
            assert 0 < mu.COHORT_SPREAD[L][f] and worst[f] <= 2 * mu.COHORT_SPREAD[L][f], (L, f, worst[f])
    gl, pos, F, A, freq, regs = mu.confident_case(pkg)
    e = su.emissions_np(gl, np.full(gl.shape[0], freq))
    lr = e[..., 1] - e[..., 0]
    assert 1.3 < np.abs(lr).mean() < 1.8 and np.isinf(pos).sum() == 2
    for L in mu.LENGTHS:
        a = mu.moments_a(e, pos, F, A, list(regs.values()), L)
        bb = mu.moments_b(e, pos, F, A, list(regs.values()), L)
        worst = _worst(a, bb)
        print(f"  confident {L:5s} spread |A - B|: " + ", ".join(f"{f} {worst[f]:.3e}" for f in worst))
        for f in worst:
            assert 0 < mu.CONFIDENT_SPREAD[L][f] and worst[f] <= 2 * mu.CONFIDENT_SPREAD[L][f], (L, f, worst[f])
        if L == "sites":
            # the chain is confident: thousands of IBD sites known to a few (sd / mean < 1e-3), so
            # an uncentred float64 jet (eps E[A]^2 / Var per operation) cannot hold the tolerance
            w = bb[0][:, 0]
            assert (w["mean_a"] > 5000).all() and (w["var_a"] < 100).all()
            assert (2.2e-16 * w["mean_a"] ** 2 > 16 * mu.CONFIDENT_SPREAD[L]["var_a"]).all()


def test_sampler_condition_on_the_gpu_cohort(pkg, cohort_b):
    """The restatement of the sampler (sample_util) against yardstick B's variances and covariance
    on the GPU test's cohort, draws and seed: the condition that test relies on holds before the
    device is asked."""
    d, e, F, A = _cohort(pkg)
    pos = d.pos_dist_mb
    sets, b = cohort_b
    k = list(sets).index("whole")
    f = su.forward_filter(e, pos, F, A)
    thr = su.thresholds(f, pos, F, A)
    u = su.uniforms(mu.SAMPLER_SEED, range(mu.SAMPLER_DRAWS), d.n_ind, d.n_sites)
    stats = su.path_stats(su.backward_draw(thr, u), pos)
    worst = mu.sampler_check(stats, b["sites"][k][:, 0], b["mb"][k][:, 0])
    print(f"\n  sampler restatement against yardstick B's variances: largest |z| = {worst:.2f}")
    # and the means are those of the expectation yardstick
    want = xu.region_records(xu.terms_b(e, pos, F, A), [[0, d.n_sites]])[:, 0]
    np.testing.assert_allclose(b["sites"][k]["mean_a"][:, 0], want["ibd"], rtol=0, atol=xu.REGION_TOL["ibd"])
    np.testing.assert_allclose(b["sites"][k]["mean_t"][:, 0], want["starts"], rtol=0, atol=xu.REGION_TOL["starts"])
    np.testing.assert_allclose(b["mb"][k]["mean_a"][:, 0], want["ibd_mb"], rtol=0, atol=xu.REGION_TOL["ibd_mb"])


def test_records_mirror_the_header(pkg):
    hm = pkg.hmm
    assert C.sizeof(hm.MomentRegion) == 40
    assert list(pkg.MOMENT_REGION_DTYPE.names) == list(mu.FIELDS)
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    body = re.search(r"typedef struct nghmm_moment_region \{(.*?)\} nghmm_moment_region;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == list(mu.FIELDS)
    assert int(re.search(r"NGHMM_MOMENTS_MB = (\d+)", header).group(1)) == pkg.MOMENTS_MB == 1


def test_moment_sd_on_hand_made_records(pkg):
    rec = np.zeros((1, 4), dtype=pkg.MOMENT_REGION_DTYPE)
    rec["mean_a"], rec["mean_t"] = [[12.0, 3.0, 0.0, 5.0]], [[3.0, 0.0, 0.0, 2.0]]
    rec["var_a"], rec["var_t"] = [[4.0, 1.0, 0.0, 9.0]], [[0.25, 0.0, 0.0, 1.0]]
    rec["cov_at"] = [[0.5, 0.0, 0.0, -1.5]]
    sd = pkg.moment_sd(rec)
    assert np.array_equal(sd["sd_a"], [[2.0, 1.0, 0.0, 3.0]]) and np.array_equal(sd["sd_t"], [[0.5, 0.0, 0.0, 1.0]])
    assert np.array_equal(sd["corr"], [[0.5, np.nan, np.nan, -0.5]], equal_nan=True)
    assert np.array_equal(sd["tract_length"], [[4.0, np.nan, np.nan, 2.5]], equal_nan=True)
    # sqrt(var_a - 2 R cov + R^2 var_t) / mean_t
    want = [[np.sqrt(4.0 - 2 * 4.0 * 0.5 + 16.0 * 0.25) / 3.0, np.nan, np.nan,
             np.sqrt(9.0 + 2 * 2.5 * 1.5 + 6.25) / 2.0]]
    np.testing.assert_allclose(sd["tract_length_sd"], want, rtol=1e-15, equal_nan=True)
    assert all(v.shape == rec.shape for v in sd.values())


@pytest.fixture(scope="module")
def asan_moments_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp with and without the entries of tests/stub/nghmm_moments_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_moments")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_moments_stub.cpp")), ("without", ("nghmm_stub.cpp",))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "%.10g" % v


def test_ibd_moments_writer_under_address_sanitizer(pkg, tmp_path, asan_moments_host):
    """--ibd_moments writes PREFIX.ibd.moments: the header, one line per individual and chromosome
    (or window that restarts at every chromosome), the stub's formulas as %.10g with NA for a
    correlation whose variance is 0; default IDs and --ind_names, one handle or a chain of three,
    multi-start replicates (the winning one's only); without the flag the file does not appear and
    the other files are byte-identical; --moments_window alone is a warning; a library without the
    entry still links and stops the run with a message."""
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
        ("window", ["--moments_window", 40, "--ind_names", tmp_path / "names.txt"], 40, names),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--moments_window", 7,
                   "--ind_names", tmp_path / "names.txt"], 7, names),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], 0, None),
    ]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    def corr(cov, va, vt):
        return _g10(cov / (np.sqrt(va) * np.sqrt(vt))) if va > 0 and vt > 0 else "NA"

    n_na = 0
    for tag, extra, window, ids in runs:
        plain, ex = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"ex_{tag}")
        r = run(asan_moments_host["full"], plain, extra)
        assert ("--moments_window is only used by --ibd_moments" in r.stderr) == (window > 0)
        run(asan_moments_host["full"], ex, extra + ["--ibd_moments"])
        ids = ids or [f"ind{i}" for i in range(I)]
        regions = summary_util.chrom_regions(chrom, window)
        want = ["ind\tchr\tfirst_pos\tlast_pos\tn_sites\texp_ibd_sites\tsd_ibd_sites\texp_tracts\tsd_tracts\t"
                "corr_sites_tracts\texp_ibd_mb\tsd_ibd_mb\tcorr_mb_tracts"]
        for i in range(I):
            for a, b in regions:
                a, b = int(a), int(b)
                n = float(b - a)
                mt, vt = 1.0 / (1.0 + a) + i, (0.0 if a % 5 == 0 else 0.125 * (i + 1))
                va, vm = 0.5 * n + i, 1e-6 * n * i
                cs, cm = 0.01 * np.sqrt(n), -1e-4 * np.sqrt(n)
                n_na += (vt == 0) + (vm == 0 or vt == 0)
                want.append("\t".join([ids[i], chrom[a], str(pos[a]), str(pos[b - 1]), str(b - a),
                                       _g10(0.25 * n + i), _g10(np.sqrt(va)), _g10(mt), _g10(np.sqrt(vt)),
                                       corr(cs, va, vt), _g10(0.001 * n + 1e-4 * i), _g10(np.sqrt(vm)),
                                       corr(cm, vm, vt)]))
        assert open(ex + ".ibd.moments").read() == "\n".join(want) + "\n", tag
        if window:       # the windows restart at every chromosome
            first = {c: chrom.index(c) for c in set(chrom)}
            assert {int(a) for a, _ in regions} >= set(first.values())
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(ex + ext, "rb").read(), (tag, ext)
        made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                                  if f.startswith(os.path.basename(pre) + "."))
        new = [e for e in made(ex) if e not in made(plain)]
        assert all(e.endswith(".ibd.moments") for e in new), (tag, new)
        assert len(new) == (2 if tag == "starts" else 1)          # (the winning replicate's only)
    assert n_na > 10
    r = run(asan_moments_host["full"], str(tmp_path / "bad"), ["--ibd_moments", "--moments_window", 0], ok=False)
    assert "invalid --moments_window" in r.stderr
    r = run(asan_moments_host["without"], str(tmp_path / "none"), ["--ibd_moments"], ok=False)
    assert "--ibd_moments: the library has no nghmm_chain_ibd_moments!" in r.stderr
    run(asan_moments_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_chrom") + ext, "rb").read(), ext
