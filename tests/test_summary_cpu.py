"""Region and site summaries without a GPU: the numpy restatement of the definitions
(tests/summary_util.py) against a literal loop, the region helpers of the package, and the host's
--ibd_summary writers under AddressSanitizer / UBSan against the CPU stand-in of the library
(tests/stub/)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cli_util
import summary_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_literal_loop():
    """5 x 40, two chromosomes: regions of one site, across the chromosome start, with gaps; IBD
    runs across region edges and across the chromosome start."""
    rng = np.random.default_rng(5)
    I, S = 5, 40
    d = rng.uniform(0.001, 0.2, S)
    d[0] = d[23] = np.inf
    path = (rng.random((I, S)) < 0.6).astype(np.uint8)
    path[0, :] = 1
    path[1, 20:27] = 1
    marg = rng.random((I, S))
    marg[2, 7] = 0.5            # on the threshold: counted
    regions = np.array([(0, 1), (1, 9), (9, 10), (12, 30), (30, 40)])
    reg, sites, n_mb = summary_util.summarize(path, marg, d, regions, 0.5)
    want_reg, want_sites = summary_util.triple_loop(path, marg, d, regions, 0.5)
    for f in ("vit_sites", "post_sites"):
        assert np.array_equal(reg[f], want_reg[f])
    for f in ("vit_count", "post_count"):
        assert np.array_equal(sites[f], want_sites[f])
    np.testing.assert_allclose(reg["post_sum"], want_reg["post_sum"], rtol=40 * 2.0 ** -52, atol=0)
    np.testing.assert_allclose(reg["vit_mb"], want_reg["vit_mb"], rtol=40 * 2.0 ** -52, atol=0)
    np.testing.assert_allclose(sites["post_sum"], want_sites["post_sum"], rtol=10 * 2.0 ** -52, atol=0)
    # what the rules are there for: individual 0 is IBD everywhere
    assert reg["vit_sites"][0].tolist() == [1, 8, 1, 18, 10]
    assert reg["vit_mb"][0, 0] == 0.0 and n_mb[0].tolist() == [0, 7, 0, 16, 9]   # 23 is skipped in [12, 30)
    assert reg["post_sites"][2, 1] >= 1
    # a source switched off leaves zeros
    r2, s2, _ = summary_util.summarize(path, marg, d, regions, 0.5, posterior=False)
    assert not r2["post_sites"].any() and not r2["post_sum"].any() and not s2["post_sum"].any()
    assert np.array_equal(r2["vit_sites"], reg["vit_sites"])
    r3, s3, _ = summary_util.summarize(path, marg, d, regions, 0.5, viterbi=False)
    assert not r3["vit_sites"].any() and not r3["vit_mb"].any() and not s3["vit_count"].any()


def test_region_helpers(pkg):
    inf = np.inf
    #             0    1  2  3  4  5    6  7    8  9  10 11 12
    d = np.array([0.1, 1, 1, 1, 1, 1, inf, 1, inf, 1, 1, 1, 1])     # site 0 starts one without inf
    assert pkg.chromosome_regions(d).tolist() == [[0, 6], [6, 8], [8, 13]]
    # a window that ends exactly at a chromosome start (3 + 3 = 6), a chromosome shorter than
    # the window (6..8), a shorter last window (11..13)
    assert pkg.window_regions(d, 3).tolist() == [[0, 3], [3, 6], [6, 8], [8, 11], [11, 13]]
    assert pkg.window_regions(d, 1).tolist() == [[s, s + 1] for s in range(13)]
    assert pkg.window_regions(d, 100).tolist() == pkg.chromosome_regions(d).tolist()
    assert pkg.window_regions(d, 6).tolist() == [[0, 6], [6, 8], [8, 13]]
    assert pkg.chromosome_regions(d).dtype.kind == "i"
    with pytest.raises(pkg.NgsFHMMError):
        pkg.window_regions(d, 0)
    with pytest.raises(pkg.NgsFHMMError):
        pkg.chromosome_regions(np.zeros(0))
    # the same regions as the command line makes from the --pos file's names
    names = ["a"] * 6 + ["b"] * 2 + ["c"] * 5
    assert summary_util.chrom_regions(names, 3).tolist() == pkg.window_regions(d, 3).tolist()
    assert summary_util.chrom_regions(names).tolist() == pkg.chromosome_regions(d).tolist()


def test_records_and_segment_constant_mirror_the_sources(pkg):
    import ctypes as C
    hm = pkg.hmm
    assert C.sizeof(hm.RegionStat) == 32 and C.sizeof(hm.SiteStat) == 16
    assert [f[0] for f in hm.RegionStat._fields_] == list(hm.REGION_STAT_DTYPE.names) == \
        list(summary_util.REGION_DTYPE.names)
    assert [f[0] for f in hm.SiteStat._fields_] == list(hm.SITE_STAT_DTYPE.names) == \
        list(summary_util.SITE_DTYPE.names)
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    body = re.search(r"typedef struct nghmm_region_stat \{(.*?)\} nghmm_region_stat;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == list(hm.REGION_STAT_DTYPE.names)
    body = re.search(r"typedef struct nghmm_site_stat \{(.*?)\} nghmm_site_stat;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == list(hm.SITE_STAT_DTYPE.names)
    hpp = open(os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "kernels_summary.hpp")).read()
    assert int(re.search(r"kSummarySeg = (\d+);", hpp).group(1)) == pkg.SUMMARY_SEGMENT_SITES
    assert pkg.SUMMARY_SEGMENT_SITES % 16 == 0


@pytest.fixture(scope="module")
def asan_summary_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp plus the summary entries of tests/stub/nghmm_summary_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stubs = [os.path.join(ROOT, "tests", "stub", f) for f in ("nghmm_stub.cpp", "nghmm_summary_stub.cpp")]
    exe = str(tmp_path_factory.mktemp("asan_summary") / "ngsF-HMM_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", host, *stubs, "-o", exe, "-lz", "-lpthread"],
                   check=True)
    return exe


def test_ibd_summary_writers_under_address_sanitizer(pkg, tmp_path, asan_summary_host):
    """--ibd_summary writes PREFIX.ibd.regions and PREFIX.ibd.sites = the definitions applied to
    the run's own .ibd file and .pos file, byte for byte: per chromosome and per window (one that
    leaves a shorter last window, one longer than a chromosome), default IDs and --ind_names, one
    handle or a chain of three, multi-start replicates (the winning one's only); without the flag
    neither file appears and the other files are byte-identical."""
    I, S = 5, 301            # odd: the stand-in's filler path changes phase from line to line
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "0", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k} extra\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]
    chrom, pos, dist = summary_util.read_pos(p["pos_gz"])
    assert len(set(chrom)) == 3
    runs = [
        ("chrom", [], 0, 0.5, None),
        ("window", ["--summary_window", 40, "--ind_names", tmp_path / "names.txt"], 40, 0.5, names),
        ("wide", ["--summary_window", 100000, "--summary_thresh", 0.75], 100000, 0.75, None),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--summary_window", 7,
                   "--ind_names", tmp_path / "names.txt"], 7, 0.5, names),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], 0, 0.5, None),
    ]

    def run(out, extra):
        r = subprocess.run([asan_summary_host] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    for tag, extra, window, thr, ids in runs:
        plain, summ = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"summ_{tag}")
        run(plain, extra)       # (--summary_window / --summary_thresh alone: a warning)
        run(summ, extra + ["--ibd_summary"])
        ids = ids or [f"ind{i}" for i in range(I)]
        path, marg = summary_util.read_ibd(summ + ".ibd", I)
        regions = summary_util.chrom_regions(chrom, window)
        reg, sites, _ = summary_util.summarize(path, marg, dist, regions, thr)
        assert reg["vit_sites"].sum() > 100 and len(regions) >= 3
        assert open(summ + ".ibd.regions").read() == summary_util.regions_text(reg, regions, chrom, pos, ids), tag
        assert open(summ + ".ibd.sites").read() == summary_util.sites_text(sites, chrom, pos, I), tag
        if thr > 0.5:
            assert not reg["post_sites"].any()
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(summ + ext, "rb").read(), (tag, ext)
        for ext in (".ibd.regions", ".ibd.sites"):
            assert not os.path.exists(plain + ext)
        if tag == "starts":     # the winning replicate's only, like .indF.se
            have = [os.path.exists(f"{summ}.REP_{k:02d}.ibd.regions") for k in (1, 2)]
            assert sorted(have) == [False, True]

    # the argument checks of the command line
    for bad, msg in ((["--ibd_summary", "--summary_thresh", 0], "invalid --summary_thresh"),
                     (["--ibd_summary", "--summary_thresh", 1.5], "invalid --summary_thresh"),
                     (["--ibd_summary", "--summary_window", 0], "invalid --summary_window")):
        r = subprocess.run([asan_summary_host] + [str(a) for a in base + bad + ["--out", str(tmp_path / "bad")]],
                           env=env, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (bad, r.stderr[-500:])
    r = run(str(tmp_path / "warn"), ["--ind_names", tmp_path / "names.txt"])
    assert "--ind_names is only used by" in r.stderr and "--ibd_summary" in r.stderr
