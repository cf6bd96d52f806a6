"""The yardstick of the observed-information tests checked before it is used (tests/info_util.py),
the standard-error rule, the C ABI surface of nghmm_obs_info and the host's --indF_se; no GPU.

Worst relative error of the binary64 restatement of the jet recursion against the 50-digit
reference over the cases of test_restatement_agrees_with_the_50_digit_reference (measured):
lkl 1.2e-15, g_F 1.1e-14, g_A 1.0e-14, h_FF 5.8e-13, h_FA 1.9e-13, h_AA 4.1e-14 -- the Hessian's
largest at 3000 sites; as a share of the device tests' bounds at most 1.2e-3 (lkl), 5.8e-4 (h_FF)
and 6.7e-6 (the gradient).  DESIGN.md section 4 has the same figures per number of sites; the
test prints them (run with -s)."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np

import info_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_agrees_with_the_50_digit_reference():
    """Three chromosomes, random emissions, the points (0.1, 0.5), (0.02, 3.0), (0.6, 0.01) and the
    corner (1e-15, 10): gradient and Hessian of the binary64 restatement stay three decades inside
    the device tests' bounds, lkl inside 1e-14 relative (a hundredth of its bound; it carries the
    rounding of a sum of S logarithms)."""
    scale = {f: 1e-3 for f in iu.FIELDS}
    scale["lkl"] = 1e-2
    for seed, n_ind, n_sites in ((1, 3, 500), (2, 1, 3000)):
        le, pos = iu.random_case(seed, n_ind, n_sites)
        assert np.isinf(pos).sum() == 3
        for F, A in iu.POINTS + ((1e-15, 10.0),):
            ref = iu.ref_records(le, pos, F, A)
            got = iu.jet_info_np(le, pos, F, A)
            iu.check_records(got, ref, F, A, scale=scale, label=f"{n_sites} sites ({F}, {A})")
            rel = {f: float(np.max(np.abs(got[f] - ref[f]) / np.abs(ref[f]))) for f in iu.FIELDS}
            print("   relative: " + ", ".join(f"{f} {rel[f]:.2g}" for f in iu.FIELDS))


def test_reference_on_two_sites_by_hand():
    """l(F, a) of two sites in closed form, differentiated by hand in F: the reference's value and
    its F derivatives."""
    le = np.log(np.array([[0.5, 0.25], [0.125, 0.5]]))
    pos = np.array([np.inf, 0.5])
    F, A = 0.25, 2.0
    c = math.exp(-A * 0.5)
    # v1 = (q0 e00, q1 e01); Z = sum_l e1l (c v1_l + (1 - c) (v1_0 + v1_1) q_l)
    def Z(f):
        q0, q1 = 1 - f, f
        v0, v1 = q0 * 0.5, q1 * 0.25
        s = v0 + v1
        return 0.125 * (c * v0 + (1 - c) * s * q0) + 0.5 * (c * v1 + (1 - c) * s * q1)
    r = iu.ref_info(le, pos, F, A)
    assert abs(r[0] - math.log(Z(F))) < 1e-15
    # Z is a quadratic in F: exact central differences
    h = 0.125
    Z1 = (Z(F + h) - Z(F - h)) / (2 * h)
    Z2 = (Z(F + h) - 2 * Z(F) + Z(F - h)) / (h * h)
    assert abs(r[1] - Z1 / Z(F)) < 1e-13
    assert abs(r[3] - (Z2 / Z(F) - (Z1 / Z(F)) ** 2)) < 1e-12
    got = iu.jet_info_np(le[None], pos, F, A)[0]
    for k, f in enumerate(iu.FIELDS):
        assert abs(got[f] - r[k]) <= 1e-13 * max(1.0, abs(r[k])), f


def _records(rows):
    out = np.zeros(len(rows), dtype=iu.INFO_DTYPE)
    for k, (hFF, hFA, hAA) in enumerate(rows):
        out[k] = (-100.0, 0.0, 0.0, hFF, hFA, hAA)
    return out


def test_std_errors_on_hand_made_records():
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    assert hm.INFO_DTYPE == iu.INFO_DTYPE and hm.INFO_DTYPE.itemsize == 48
    nan = math.nan
    # -h = [[4, 1], [1, 1]]: det 3, inverse [[1, -1], [-1, 4]] / 3
    cases = [
        ((-4.0, -1.0, -1.0), 0.3, 0.5, (math.sqrt(1 / 3), math.sqrt(4 / 3), -0.5)),      # interior
        ((-4.0, -1.0, -1.0), 0.5e-5, 0.5, (nan, nan, nan)),                               # F at its lower bound
        ((-4.0, -1.0, -1.0), 1 - 0.5e-5, 0.5, (nan, nan, nan)),                           # ... upper
        ((-4.0, -1.0, -1.0), 0.3, 1e-15, (0.5, nan, nan)),                                # alpha at its lower bound
        ((-4.0, -1.0, -1.0), 0.3, 10.0, (0.5, nan, nan)),                                 # ... upper
        ((4.0, -1.0, -1.0), 0.3, 0.5, (nan, nan, nan)),                                   # not definite: h_FF > 0
        ((-1.0, -2.0, -1.0), 0.3, 0.5, (nan, nan, nan)),                                  # ... det < 0
        ((4.0, -1.0, -1.0), 0.3, 10.0, (nan, nan, nan)),                                  # alpha fixed, h_FF > 0
        ((-4.0, 1.0, -1.0), 1e-5, 1e-14, (math.sqrt(1 / 3), math.sqrt(4 / 3), 0.5)),      # just inside
    ]
    info = _records([c[0] for c in cases])
    F = np.array([c[1] for c in cases])
    A = np.array([c[2] for c in cases])
    got = np.stack(hm.std_errors(info, F, A), axis=1)
    want = np.array([c[3] for c in cases])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-15)


def test_header_binding_and_library_have_the_entries():
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    text = open(os.path.join(ROOT, "include", "nghmm.h")).read()
    assert "conditional on the frequencies" in re.sub(r"\s+", " ", text.lower().replace("*", ""))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(hm.library_path())
    for name in ("nghmm_obs_info", "nghmm_chain_obs_info"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in hm.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "typedef struct nghmm_info" in text


def _asan_build(tmp, stubs):
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    exe = str(tmp / "ngsF-HMM_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", host,
                    *[os.path.join(ROOT, "tests", "stub", f) for f in stubs], "-o", exe, "-lz", "-lpthread"],
                   check=True)
    return exe


def _g(v):
    return "NA" if math.isnan(v) else "%.10g" % v


def test_cli_indF_se_under_address_sanitizer(tmp_path_factory, tmp_path):
    """--indF_se against the stand-in library writes PREFIX.indF.se with exactly the bytes that
    Python's std_errors and "%.10g" make of the stand-in's records (one of them not definite, one
    with a negative determinant), --ind_names is honoured, a chain and the multi-start path work;
    without the flag the output files are those of a build against the stand-ins without the
    entry, byte for byte; against those the flag stops with a message.  A run against the
    stand-in whose EM ends on the bounds (tests/stub/nghmm_bounds_stub.cpp: individual 2's alpha
    is 10, individual 4's indF 1e-6) writes NA for se_alpha and corr next to a number for se_indF
    in the one row and NA for all three in the other.  The host's rule equals Python's on a list
    of records (--se_kat)."""
    import cli_util
    pkg = importlib.import_module("ngsf-hmm_amd")
    new = _asan_build(tmp_path_factory.mktemp("asan_info"),
                      ("nghmm_stub.cpp", "nghmm_tracts_stub.cpp", "nghmm_sample_stub.cpp", "nghmm_info_stub.cpp"))
    old = _asan_build(tmp_path_factory.mktemp("asan_old"),
                      ("nghmm_stub.cpp", "nghmm_tracts_stub.cpp", "nghmm_sample_stub.cpp"))
    bnd = _asan_build(tmp_path_factory.mktemp("asan_bounds"),
                      ("nghmm_bounds_stub.cpp", "nghmm_tracts_stub.cpp", "nghmm_sample_stub.cpp",
                       "nghmm_info_stub.cpp"))
    I, S = 5, 301
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "x", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k}\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]

    def run(exe, out, extra, ok=True, stdin=None):
        r = subprocess.run([exe] + [str(a) for a in base + extra + (["--out", out] if out else [])], env=env,
                           capture_output=True, text=True, input=stdin)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert (r.returncode == 0) == ok, (extra, r.stderr[-3000:])
        return r

    def stub_records(F):
        out = np.zeros(I, dtype=iu.INFO_DTYPE)
        for i in range(I):
            out[i] = (-1000.0 - 3.0 * i - F[i], 0.001 * (i + 1), -0.002 * (i + 1),
                      7.0 if i == 1 else -(40.0 + 10.0 * i), 50.0 if i == 3 else 1.5 + 0.5 * i, -(2.0 + i))
        return out

    def expected(ids, F, A):
        rec = stub_records(F)
        se_F, se_A, corr = pkg.std_errors(rec, F, A)
        text = "ind\tindF\tse_indF\talpha\tse_alpha\tcorr\tlkl\tgrad_indF\tgrad_alpha\n"
        for i in range(I):
            text += "\t".join([ids[i]] + [_g(v) for v in (F[i], se_F[i], A[i], se_A[i], corr[i], rec["lkl"][i],
                                                         rec["g_F"][i], rec["g_A"][i])]) + "\n"
        return text, (se_F, se_A, corr)

    def final_F(f0, iters):                 # the stand-in's iteration: F <- 0.25 + 0.5 F
        for _ in range(iters):
            f0 = 0.25 + 0.5 * f0
        return f0

    runs = [("one", ["--indF", "0.3,0.5"], None, 0.5),
            ("bounds", ["--indF", "0.3,0.5"], None, 0.5),
            ("chain", ["--indF", "0.3,0.5", "--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--ind_names",
                       tmp_path / "names.txt"], names, 0.5),
            ("starts", ["--indF", "0.3,0.5", "--n_starts", 2, "--keep_starts", "--seed", 3], None, 0.5)]
    for tag, extra, ids, alpha in runs:
        plain, se, ref = (str(tmp_path / f"{k}_{tag}") for k in ("plain", "se", "ref"))
        exe = bnd if tag == "bounds" else new
        run(exe, plain, extra)
        run(old, ref, extra)
        run(exe, se, extra + ["--indF_se"])
        ids = ids or [f"ind{i}" for i in range(I)]
        rows = open(se + ".indF.se").read().split("\n")[1:-1]
        F = np.array([float(r.split("\t")[1]) for r in rows])
        A = np.array([float(r.split("\t")[3]) for r in rows])
        # the stand-in's parameters: alpha as given, F after two or three of its iterations; the
        # bounds stand-in's individuals 2 and 4 on their bounds
        free = np.ones(I, dtype=bool)
        if tag == "bounds":
            assert A[2] == 10.0 and F[4] == 1e-6
            free[[2, 4]] = False
            assert [c == "NA" for c in rows[2].split("\t")] == [0, 0, 0, 0, 1, 1, 0, 0, 0]
            assert [c == "NA" for c in rows[4].split("\t")] == [0, 0, 1, 0, 1, 1, 0, 0, 0]
        assert any(np.allclose(F[free], final_F(0.3, n), rtol=1e-9, atol=0) for n in (2, 3)), F
        assert np.all(np.delete(A, 2) == alpha) and A[2] == (alpha if free[2] else 10.0)
        text, (se_F, se_A, corr) = expected(ids, F, A)
        assert open(se + ".indF.se").read() == text, tag
        assert np.isnan(se_F[1]) and np.isnan(corr[3]) and np.isfinite(se_F[0]) and np.isfinite(corr[0])
        assert np.isfinite(se_F[2]) and np.isnan(se_A[2]) == np.isnan(corr[2]) == (not free[2])
        assert np.isnan(se_F[4]) == (not free[4])
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(se + ext, "rb").read(), (tag, ext)
            if tag != "bounds":         # (the bounds stand-in's parameters are its own)
                assert open(plain + ext, "rb").read() == open(ref + ext, "rb").read(), (tag, ext)
        assert not os.path.exists(plain + ".indF.se")
        produced = lambda pre: sorted(f for f in os.listdir(tmp_path) if f.startswith(os.path.basename(pre) + "."))
        assert [f.split(".", 1)[1] for f in produced(plain)] == [f.split(".", 1)[1] for f in produced(ref)]
        if tag == "starts":                 # the winning replicate's only (and its copy)
            reps = [k for k in (1, 2) if os.path.exists(f"{se}.REP_{k:02d}.indF.se")]
            assert len(reps) == 1
            assert open(f"{se}.REP_{reps[0]:02d}.indF.se").read() == text
    r = run(old, str(tmp_path / "old_flag"), ["--indF_se"], ok=False)
    assert "--indF_se: the library has no nghmm_chain_obs_info" in r.stderr
    # the host's rule against Python's, bounds on either side included
    rng = np.random.default_rng(4)
    n = 200
    F = np.concatenate([rng.uniform(0, 1, n - 6), [0.5e-5, 1e-5, 1 - 0.5e-5, 1 - 1e-5, 0.3, 0.3]])
    A = np.concatenate([rng.uniform(0, 10, n - 6), [0.5, 0.5, 0.5, 0.5, 1e-15, 10.0]])
    rec = np.zeros(n, dtype=iu.INFO_DTYPE)
    rec["h_FF"], rec["h_FA"], rec["h_AA"] = rng.normal(-2, 2, n), rng.normal(0, 2, n), rng.normal(-2, 2, n)
    text = "".join("%r %r %r %r %r\n" % (float(F[i]), float(A[i]), float(rec["h_FF"][i]), float(rec["h_FA"][i]),
                                           float(rec["h_AA"][i])) for i in range(n))
    r = run(new, None, ["--se_kat"], stdin=text)
    se_F, se_A, corr = pkg.std_errors(rec, F, A)
    want = "".join("\t".join(_g(v) for v in (se_F[i], se_A[i], corr[i])) + "\n" for i in range(n))
    assert r.stdout.endswith(want) and 20 < int(np.isnan(se_A).sum()) < n - 20
