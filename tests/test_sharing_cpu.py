"""Pairwise IBD sharing without a GPU: the numpy restatement of the definitions
(tests/sharing_util.py) against a literal loop, sharing_jaccard, the bindings against the header,
and the host's --ibd_sharing writer under AddressSanitizer / UBSan against the CPU stand-in of the
library (tests/stub/)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cli_util
import sharing_util
import summary_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_literal_loop():
    """5 x 40, a posterior exactly on the threshold (counted), ranges of one site, inside and
    all."""
    rng = np.random.default_rng(5)
    I, S = 5, 40
    path = (rng.random((I, S)) < 0.6).astype(np.uint8)
    path[0, :] = 1
    marg = rng.random((I, S))
    marg[2, 7] = 0.5            # on the threshold: counted
    marg[3, 7] = 0.75
    for begin, end in ((0, S), (7, 8), (3, 29), (39, 40)):
        vit, both, prod = sharing_util.sharing(path, marg, 0.5, begin, end)
        wv, wb, wp = sharing_util.triple_loop(path, marg, 0.5, begin, end)
        assert vit.dtype == both.dtype == np.uint64 and prod.dtype == np.float64
        assert np.array_equal(vit, wv) and np.array_equal(both, wb)
        np.testing.assert_allclose(prod, wp, rtol=2 * (end - begin + 1) * 2.0 ** -53, atol=0)
        assert np.array_equal(vit, vit.T) and np.array_equal(both, both.T)
    vit, both, prod = sharing_util.sharing(path, marg, 0.5, 7, 8)
    assert both[2, 2] == 1 and both[2, 3] == 1               # 0.5 >= 0.5
    assert sharing_util.sharing(path, marg, np.nextafter(0.5, 1.0), 7, 8)[1][2, 2] == 0
    vit, both, prod = sharing_util.sharing(path, marg)
    assert vit[0, 0] == S and np.array_equal(vit[0], np.diag(vit))   # individual 0 is IBD everywhere
    assert np.array_equal(np.diag(vit), path.sum(axis=1))
    np.testing.assert_allclose(np.diag(prod), (marg * marg).sum(axis=1), rtol=1e-13)
    # the writer and the parser are inverse to each other (to the 10 digits printed)
    ids = [f"ind{i}" for i in range(I)]
    got = sharing_util.parse_sharing(sharing_util.sharing_text(vit, both, prod, ids), I)
    assert got[0] == ids and np.array_equal(got[1], vit) and np.array_equal(got[2], both)
    np.testing.assert_allclose(got[3], prod, rtol=5e-10)


def test_sharing_jaccard(pkg):
    both = np.array([[4, 2, 0, 0], [2, 6, 3, 0], [0, 3, 3, 0], [0, 0, 0, 0]], dtype=np.uint64)
    j = pkg.sharing_jaccard(both)
    want = np.array([[1, 2 / 8, 0, 0], [2 / 8, 1, 3 / 6, 0], [0, 3 / 6, 1, 0], [0, 0, 0, 0]])
    assert j.dtype == np.float64 and np.array_equal(j, want)      # (3, 3): 0 / 0 -> 0
    assert np.array_equal(j, j.T)
    with pytest.raises(pkg.NgsFHMMError):
        pkg.sharing_jaccard(np.zeros((2, 3)))


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_bindings_and_split_constant_mirror_the_sources(pkg):
    hm = pkg.hmm
    L = pkg.load_library()
    vp, u64p, dp = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    ctype = {"nghmm_t* h": vp, "nghmm_t** hs": C.POINTER(vp), "int n": C.c_int, "int what": C.c_int,
             "double threshold": C.c_double, "uint64_t site_begin": C.c_uint64,
             "uint64_t site_end": C.c_uint64, "uint64_t* vit_both": u64p, "uint64_t* post_both": u64p,
             "double* post_prod": dp}
    one = _header_args("nghmm_ibd_sharing")
    assert one == ["nghmm_t* h", "int what", "double threshold", "uint64_t site_begin",
                   "uint64_t site_end", "uint64_t* vit_both", "uint64_t* post_both", "double* post_prod"]
    chain = _header_args("nghmm_chain_ibd_sharing")
    assert chain == ["nghmm_t** hs", "int n"] + one[1:]
    for name, args in (("nghmm_ibd_sharing", one), ("nghmm_chain_ibd_sharing", chain)):
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [ctype[a] for a in args], name
        assert name in hm.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    m = re.search(r"enum \{ NGHMM_SHARING_VITERBI = (\d+), NGHMM_SHARING_POSTERIOR = (\d+) \};", header)
    assert (int(m.group(1)), int(m.group(2))) == (pkg.SHARING_VITERBI, pkg.SHARING_POSTERIOR) == (1, 2)
    hpp = open(os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "kernels_sharing.hpp")).read()
    assert int(re.search(r"kSharingSplit = (\d+);", hpp).group(1)) == pkg.SHARING_SPLIT_SITES
    assert int(re.search(r"kSharingMaxSplits = (\d+);", hpp).group(1)) == 1024
    assert re.search(r"kSharingScratchBytes = 256ull << 20;", hpp)
    assert pkg.SHARING_SPLIT_SITES % 64 == 0
    # the plan: a function of (I, begin, end); edges at multiples of 64; the caps
    L_ = pkg.SHARING_SPLIT_SITES
    assert pkg.sharing_splits(40, 0, 2 * L_ + 5) == (0, 704, 3)
    assert pkg.sharing_splits(40, 17, 18) == (0, 64, 1)
    assert pkg.sharing_splits(40, 130, 131) == (128, 64, 1)
    first, length, n = pkg.sharing_splits(1000, 0, 1_000_000)
    assert n == 33 and n * 1000 * 1000 * 8 <= 1 << 28 and length % 64 == 0 and n * length >= 1_000_000
    assert pkg.sharing_splits(100, 0, 100_000_000)[2] == 1024
    assert pkg.sharing_splits(10_000, 0, 100_000) == (0, 100_032, 1)


@pytest.fixture(scope="module")
def asan_sharing_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined, a program of its own, against
    tests/stub/nghmm_stub.cpp plus the sharing entries of tests/stub/nghmm_sharing_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stubs = [os.path.join(ROOT, "tests", "stub", f) for f in ("nghmm_stub.cpp", "nghmm_sharing_stub.cpp")]
    exe = str(tmp_path_factory.mktemp("asan_sharing") / "ngsF-HMM_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", host, *stubs, "-o", exe, "-lz", "-lpthread"],
                   check=True)
    return exe


def test_ibd_sharing_writer_under_address_sanitizer(pkg, tmp_path, asan_sharing_host):
    """--ibd_sharing writes PREFIX.ibd.sharing = the definitions applied to the run's own .ibd
    file, byte for byte: default IDs and --ind_names, one handle or a chain of three, multi-start
    replicates (the winning one's only); without the flag the file does not appear and the other
    files are byte-identical."""
    I, S = 5, 301            # odd: the stand-in's filler path changes phase from line to line
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "0", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k} extra\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]
    runs = [
        ("plain", [], 0.5, None),
        ("names", ["--ind_names", tmp_path / "names.txt"], 0.5, names),
        ("thresh", ["--sharing_thresh", 0.75], 0.75, None),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--ind_names",
                   tmp_path / "names.txt"], 0.5, names),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], 0.5, None),
    ]

    def run(out, extra):
        r = subprocess.run([asan_sharing_host] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r

    for tag, extra, thr, ids in runs:
        plain, shar = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"shar_{tag}")
        r = run(plain, extra)
        if tag == "thresh":     # --sharing_thresh alone: a warning
            assert "--sharing_thresh is only used by --ibd_sharing" in r.stderr
        run(shar, extra + ["--ibd_sharing"])
        ids = ids or [f"ind{i}" for i in range(I)]
        path, marg = summary_util.read_ibd(shar + ".ibd", I)
        vit, both, prod = sharing_util.sharing(path, marg, thr)
        assert vit.sum() > 100 and vit[0, 1] != vit[0, 2]
        text = open(shar + ".ibd.sharing").read()
        assert text == sharing_util.sharing_text(vit, both, prod, ids), tag
        got = sharing_util.parse_sharing(text, I)
        assert got[0] == ids and np.array_equal(got[1], vit) and np.array_equal(got[2], both)
        assert both.any() == (thr <= 0.5)          # the stand-in's posteriors are 0.5 everywhere
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(shar + ext, "rb").read(), (tag, ext)
        assert not os.path.exists(plain + ".ibd.sharing")
        assert sorted(os.listdir(tmp_path)).count(f"plain_{tag}.ibd.sharing") == 0
        new = {f[len(f"shar_{tag}"):] for f in os.listdir(tmp_path) if f.startswith(f"shar_{tag}")} - \
            {f[len(f"plain_{tag}"):] for f in os.listdir(tmp_path) if f.startswith(f"plain_{tag}")}
        if tag == "starts":     # the winning replicate's only, like .indF.se
            have = [os.path.exists(f"{shar}.REP_{k:02d}.ibd.sharing") for k in (1, 2)]
            assert sorted(have) == [False, True]
            assert len(new) == 2 and ".ibd.sharing" in new
        else:
            assert new == {".ibd.sharing"}, (tag, new)

    # the argument checks of the command line
    for bad in (["--ibd_sharing", "--sharing_thresh", 0], ["--ibd_sharing", "--sharing_thresh", 1.5],
                ["--sharing_thresh", -1]):
        r = subprocess.run([asan_sharing_host] + [str(a) for a in base + bad + ["--out", str(tmp_path / "bad")]],
                           env=env, capture_output=True, text=True)
        assert r.returncode != 0 and "invalid --sharing_thresh" in r.stderr, (bad, r.stderr[-500:])
    r = run(str(tmp_path / "warn"), ["--ind_names", tmp_path / "names.txt"])
    assert "--ind_names is only used by" in r.stderr and "--ibd_sharing" in r.stderr
    r = run(str(tmp_path / "nowarn"), ["--ind_names", tmp_path / "names.txt", "--ibd_sharing"])
    assert "--ind_names is only used by" not in r.stderr
