"""Tract support without a GPU: the two numpy yardsticks of tests/support_util.py against brute-force
enumeration, their spread on the cohort of tests/test_gpu_support.py (the figure that test's
tolerance is made of), and the host's --ibd_support writer under AddressSanitizer / UBSan against
the CPU stand-in of the library (tests/stub/)."""
import math
import os
import subprocess

import numpy as np
import pytest

import cli_util
import sample_util as su
import support_util as sup
import tracts_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_case(with_zero):
    """3 x 12: two chromosomes (a start at site 7), random likelihoods, one frequency per site;
    with_zero: individual 1 has a cell with likelihoods (0, 1, 0) at site 4."""
    rng = np.random.default_rng(11)
    I, S = 3, 12
    gl = np.log(rng.dirichlet(np.ones(3), size=(S, I)))
    if with_zero:
        with np.errstate(divide="ignore"):
            gl[4, 1] = np.log(np.array([0.0, 1.0, 0.0]))
    pos = rng.uniform(0.01, 0.6, S)
    pos[0] = pos[7] = np.inf
    e = su.emissions_np(gl, rng.uniform(0.1, 0.5, S))
    F, A = np.array([0.3, 0.6, 0.85]), np.array([0.4, 1.5, 0.05])
    ranges = [(0, 0, S - 1), (1, 0, 2), (1, 3, 3), (1, 4, 4), (1, 5, 9), (1, 10, 11),
              (2, 0, 0), (2, 2, 6), (2, 7, 7), (2, 8, 11)]
    return e, pos, F, A, sup.to_records(ranges)


@pytest.mark.parametrize("with_zero", [False, True])
def test_yardsticks_equal_enumeration(with_zero):
    """A and B against all 2^12 paths: a chromosome start inside a range ((1, 5, 9)), one-site
    ranges, the whole data; with a (0, 1, 0) cell the all-IBD probability of every range over it
    is exactly 0 and both yardsticks say -inf."""
    e, pos, F, A, rec = _small_case(with_zero)
    want, post = sup.enumerate_support(e, pos, F, A, rec)
    ind, lo, hi = sup.as_ranges(rec)
    if with_zero:
        assert np.isneginf(e[1, 4, 1]), "the restatement carries the exact zero"
        over = (ind == 1) & (lo <= 4) & (hi >= 4)
        assert over.sum() == 1 and np.isneginf(want[over, 0]).all()
    for name, fn in (("A", sup.support_a), ("B", sup.support_b)):
        got = fn(e, pos, F, A, rec)
        for col, field in enumerate(("log_p_ibd", "log_p_non")):
            fin = np.isfinite(want[:, col])
            assert np.array_equal(np.isneginf(got[field]), ~fin), (name, field)
            np.testing.assert_allclose(got[field][fin], want[fin, col], rtol=0, atol=2e-13,
                                       err_msg=f"{name} {field}")
        for k, (i, a, b) in enumerate(zip(ind, lo, hi)):
            seg = post[i, a:b + 1]
            assert abs(got["post_min"][k] - seg.min()) < 1e-13 and got["post_min_site"][k] == a + seg.argmin()
    # the whole data in one state: ln of that path's posterior, and the two cannot exceed 1
    k = 0
    assert lo[k] == 0 and hi[k] == e.shape[1] - 1
    assert math.exp(got["log_p_ibd"][k]) + math.exp(got["log_p_non"][k]) <= 1.0
    # a one-site range: the per-site posterior
    one = lo == hi
    np.testing.assert_allclose(np.exp(got["log_p_ibd"][one]), got["post_min"][one], rtol=1e-12)
    # posterior2 is sample_util.posterior with the other state next to it
    f = su.forward_filter(e, pos, F, A)
    p2 = sup.posterior2(f, e, pos, F, A)
    assert np.array_equal(p2[..., 1], su.posterior(f, e, pos, F, A))


def test_yardstick_spread_on_the_gpu_cohort(pkg):
    """|A - B| on the cohort of the GPU test, per field: the measured spread of two correct
    restatements (printed; the header of tests/test_gpu_support.py quotes it).  Also: every range
    is finite in B, and the yardstick alone leaves fewer than 2 % of the ranges without a
    post_min_site that the tolerance can tell from its runner-up."""
    POST_TOL, SPREAD = sup.POST_TOL, sup.SPREAD
    d, gl, F, A, freq = sup.gpu_cohort(pkg)
    e = su.emissions_np(gl, np.full(d.n_sites, freq))
    f = su.forward_filter(e, d.pos_dist_mb, F, A)
    post = su.posterior(f, e, d.pos_dist_mb, F, A)
    worst = {"log_p_ibd": 0.0, "log_p_non": 0.0, "post_min": 0.0}
    n_all = n_close = n_site_diff = 0
    for rec in sup.cohort_ranges(post, d.pos_dist_mb, 80):
        assert len(rec) > 20
        a = sup.support_a(e, d.pos_dist_mb, F, A, rec)
        b = sup.support_b(e, d.pos_dist_mb, F, A, rec)
        for fld in ("log_p_ibd", "log_p_non"):
            assert np.isfinite(b[fld]).all() and np.isfinite(a[fld]).all()
        s = sup.spread(a, b)
        worst = {k: max(worst[k], s[k]) for k in worst}
        close = b["runner_up"] - b["post_min"] <= POST_TOL
        n_all += len(rec)
        n_close += int(close.sum())
        n_site_diff += int((a["post_min_site"][~close] != b["post_min_site"][~close]).sum())
    print(f"\n  spread |A - B|: log_p_ibd {worst['log_p_ibd']:.3e}, log_p_non "
          f"{worst['log_p_non']:.3e}, post_min {worst['post_min']:.3e}; "
          f"{n_close} of {n_all} ranges have a runner-up within {POST_TOL:g}")
    assert n_site_diff == 0
    assert n_close < 0.02 * n_all
    # what the GPU test quotes is what is measured here (within a factor of two: libm versions)
    for k in worst:
        assert worst[k] <= 2 * SPREAD[k], (k, worst[k], SPREAD[k])
    assert sup.LOG_TOL <= 1e-9 and POST_TOL <= 1e-9      # (a range has at least one site)


@pytest.fixture(scope="module")
def asan_support_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp plus the tract and support entries of the stubs next to it."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stub = lambda f: os.path.join(ROOT, "tests", "stub", f)
    tmp = tmp_path_factory.mktemp("asan_support")
    exes = {}
    for tag, files in (("full", ("nghmm_stub.cpp", "nghmm_tracts_stub.cpp", "nghmm_support_stub.cpp")),
                       ("without", ("nghmm_stub.cpp", "nghmm_tracts_stub.cpp"))):
        exes[tag] = str(tmp / f"ngsF-HMM_asan_{tag}")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", host, *[stub(f) for f in files], "-o", exes[tag],
                        "-lz", "-lpthread"], check=True)
    return exes


def _g10(v):
    return "%.10g" % v


def test_ibd_support_writer_under_address_sanitizer(pkg, tmp_path, asan_support_host):
    """--ibd_support writes PREFIX.ibd.support: the header, then one line per line of
    PREFIX.ibd.bed in its order, with its chr / start / end / IDs / skips and the stub's formula
    in the other columns (-inf written as -inf); one handle or a chain of three, multi-start
    replicates (the winning one's only); without the flag the set of output files and their bytes
    do not change; against a library without the entry the run stops with the message."""
    I, S = 5, 301            # odd: the stand-in's filler path changes phase from line to line
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "0", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k} extra\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0, "--ibd_bed"]
    runs = [
        ("one", [], None),
        ("names", ["--ind_names", tmp_path / "names.txt"], names),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--ind_names",
                   tmp_path / "names.txt"], names),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], None),
    ]

    def run(exe, out, extra, ok=True):
        r = subprocess.run([exe] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    site_of = {(f"chr{int(c)}", int(x)): s for s, (c, x) in enumerate(zip(d.chrom, d.pos))}
    ln10 = math.log(10.0)
    for tag, extra, ids in runs:
        plain, sup_ = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"sup_{tag}")
        run(asan_support_host["full"], plain, extra)
        run(asan_support_host["full"], sup_, extra + ["--ibd_support"])
        ids = ids or [f"ind{i}" for i in range(I)]
        bed = open(sup_ + ".ibd.bed").read().split("\n")[:-1]
        got = open(sup_ + ".ibd.support").read().split("\n")
        assert got[-1] == "" and len(got) == len(bed) + 2 and len(bed) > 100
        assert got[0] == "chr\tstart\tend\tind\tn_sites\tpost_mean\tlog10_p_ibd\tlod\tpost_min\tpost_min_pos"
        n_inf = 0
        for b, g in zip(bed, got[1:]):
            chrom, start, end, name, length = b.split("\t")
            first, last = site_of[(chrom, int(start) + 1)], site_of[(chrom, int(end))]
            ind, n = ids.index(name), last - first + 1
            lp_ibd = -math.inf if first % 7 == 0 else -(first + 1) / 8.0 - ind
            lp_non = -3.0 * n - ind / 4.0
            n_inf += first % 7 == 0
            want = [chrom, start, end, name, str(n), _g10(0.5), _g10(lp_ibd / ln10),
                    _g10((lp_ibd - lp_non) / ln10), _g10(1.0 / (2.0 + first)), str(int(d.pos[last]))]
            if first % 7 == 0:
                assert want[6] == want[7] == "-inf"
            assert g.split("\t") == want, (tag, b, g)
        assert n_inf > 5
        assert "0" not in [ln.split("\t")[3] for ln in got[1:-1]]     # the BED file's skips
        exts = [".indF", ".ibd", ".geno", ".ibd.bed"]
        for ext in exts:
            assert open(plain + ext, "rb").read() == open(sup_ + ext, "rb").read(), (tag, ext)
        made = lambda pre: sorted(f[len(os.path.basename(pre)):] for f in os.listdir(tmp_path)
                                  if f.startswith(os.path.basename(pre) + "."))
        new = [e for e in made(sup_) if e not in made(plain)]
        assert ".ibd.support" in new and all(e.endswith(".ibd.support") for e in new), (tag, new)
        assert len(new) == (2 if tag == "starts" else 1)          # (the winning replicate's only)
    r = run(asan_support_host["without"], str(tmp_path / "none"), ["--ibd_support"], ok=False)
    assert "--ibd_support: the library has no nghmm_chain_tract_support!" in r.stderr
    run(asan_support_host["without"], str(tmp_path / "none_plain"), [])
    for ext in (".indF", ".ibd", ".geno", ".ibd.bed"):
        assert open(str(tmp_path / "none_plain") + ext, "rb").read() == \
            open(str(tmp_path / "plain_one") + ext, "rb").read(), ext
