"""IBD tracts without a GPU: the --ind_names checks of the command line, bed_lines against a
restatement of scripts/convert_ibd.pl (convert_ibd.pl:99-130), and the host's --ibd_bed writer
under AddressSanitizer / UBSan against the CPU stand-in of the library (tests/stub/)."""
import os
import subprocess

import numpy as np
import pytest

import cli_util
import tracts_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binary(pkg):
    if not os.path.exists(cli_util.BINARY):
        pkg.build_library()
    return cli_util.BINARY


BASE = ["--geno", "x.gz", "--pos", "p", "--n_ind", 3, "--n_sites", 4, "--out", "o", "--ibd_bed",
        "--verbose", 0]


@pytest.mark.parametrize("content,msg", [
    (None, "cannot open individual names file (--ind_names)!"),
    ("a\nb\n", "number of lines in --ind_names file is not --n_ind!"),
    ("a\nb\nc\nd\n", "number of lines in --ind_names file is not --n_ind!"),
    ("a\n\tb\nc\n", "empty individual name in --ind_names file!"),
    ("a\n\nc\n", "empty individual name in --ind_names file!"),
])
def test_ind_names_errors(binary, tmp_path, content, msg):
    names = tmp_path / "names.txt"
    if content is not None:
        names.write_text(content)
    r = cli_util.run_cli(BASE + ["--ind_names", names], check=False)
    assert r.returncode != 0
    assert f"ERROR: [parse_cmd_args] {msg}" in r.stderr


def _write_ibd(path, paths):
    with open(path, "w") as fh:
        fh.write("//\t" + "\t".join("-1.0000000000" for _ in paths) + "\n")
        for row in paths:
            fh.write("".join(str(int(v)) for v in row) + "\n")
        for row in paths:
            fh.write("\t".join("0.500000" for _ in row) + "\n")


def test_bed_lines_equal_convert_ibd(pkg, tmp_path):
    """Hand-made paths: tracts at the first and last site, across a chromosome change, of one
    site, whole chromosomes; an individual whose ID Perl reads as false is skipped by both."""
    chroms = ["chr1"] * 7 + ["chr2"] * 5 + ["chrX"] * 4
    pos = [10, 20, 35, 36, 50, 51, 90, 5, 6, 7, 100, 2000, 1, 2, 3, 4]
    S = len(pos)
    paths = np.array([
        [1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 1],
        [0] * S,
        [1] * S,
        [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1],
        [1] * S,
    ], dtype=np.uint8)
    names = ["s1", "s2", "s3", "s4", "0"]
    cs = np.array([c != p for c, p in zip(chroms, [None] + chroms[:-1])])
    rle = tracts_util.rle_tracts(paths, cs)
    recs = np.array([(i, a, n, 0.0, 0.0) for i, a, n, _ in rle
                     if names[i] not in ("", "0")], dtype=pkg.hmm.TRACT_DTYPE)
    ibd, posf = tmp_path / "t.ibd", tmp_path / "t.pos"
    _write_ibd(ibd, paths)
    posf.write_text("".join(f"{c}\t{p}\n" for c, p in zip(chroms, pos)))
    want = tracts_util.convert_ibd(str(ibd), str(posf), names)
    assert want.count("\n") > 10
    assert pkg.bed_lines(recs, chroms, pos, names) == want


@pytest.fixture(scope="module")
def asan_tracts_host(tmp_path_factory):
    """The C++ host under -fsanitize=address,undefined against tests/stub/nghmm_stub.cpp plus
    the tract entries of tests/stub/nghmm_tracts_stub.cpp."""
    host = os.path.join(ROOT, "ngsf-hmm_amd", "csrc", "host", "ngsF-HMM.cpp")
    stubs = [os.path.join(ROOT, "tests", "stub", f) for f in ("nghmm_stub.cpp", "nghmm_tracts_stub.cpp")]
    exe = str(tmp_path_factory.mktemp("asan_tracts") / "ngsF-HMM_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", host, *stubs, "-o", exe, "-lz", "-lpthread"],
                   check=True)
    return exe


def test_ibd_bed_writer_under_address_sanitizer(pkg, tmp_path, asan_tracts_host):
    """--ibd_bed writes PREFIX.ibd.bed = convert_ibd.pl on the run's own .ibd path lines and
    .pos file, with default IDs and with --ind_names, one handle or a chain of three, multi-start
    replicates; the other files are byte-identical to a run without the flag."""
    I, S = 5, 301            # odd: the stand-in's filler path changes phase from line to line
    d = pkg.simulate.simulate(I, S, seed=9, n_chrom=3)
    p = cli_util.write_inputs(str(tmp_path), d, d.gl)
    names = ["NA0001", "NA0002", "0", "pop1_x", "last"]
    (tmp_path / "names.txt").write_text("".join(f"{n}\tgroup{k} extra\n" for k, n in enumerate(names)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    base = ["--geno", p["geno_gz"], "--pos", p["pos_gz"], "--n_ind", I, "--n_sites", S, "--freq", 0.1,
            "--min_iters", 2, "--max_iters", 3, "--verbose", 0]
    runs = [
        ("one", [], None),
        ("names", ["--ind_names", tmp_path / "names.txt"], names),
        ("chain", ["--n_gpus", 3, "--devices", "0,0,0", "--mode", "fast", "--ind_names",
                   tmp_path / "names.txt"], names),
        ("starts", ["--n_starts", 2, "--keep_starts", "--seed", 3, "--log", 1], None),
    ]

    def run(out, extra):
        r = subprocess.run([asan_tracts_host] + [str(a) for a in base + extra + ["--out", out]], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]

    for tag, extra, ids in runs:
        plain, bed = str(tmp_path / f"plain_{tag}"), str(tmp_path / f"bed_{tag}")
        run(plain, extra)
        run(bed, extra + ["--ibd_bed"])
        ids = ids or [f"ind{i}" for i in range(I)]
        prefixes = [bed]
        if tag == "starts":
            prefixes += [bed + ".REP_01", bed + ".REP_02"]
        for pre in prefixes:
            want = tracts_util.convert_ibd(pre + ".ibd", p["pos_gz"], ids)
            assert want.count("\n") > 100
            assert open(pre + ".ibd.bed").read() == want, (tag, pre)
        for ext in (".indF", ".ibd", ".geno"):
            assert open(plain + ext, "rb").read() == open(bed + ext, "rb").read(), (tag, ext)
        assert not os.path.exists(plain + ".ibd.bed")
