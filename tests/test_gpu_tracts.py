"""IBD tracts called on the device (nghmm_ibd_tracts / nghmm_chain_ibd_tracts, include/nghmm.h)
against a numpy run-length encoding of the handle's own path and posteriors, the oracle's
Viterbi path, one handle against chains of site shards, and the command line's .ibd.bed against
a restatement of scripts/convert_ibd.pl on the run's own .ibd file."""
import os

import numpy as np
import pytest

import cli_util
import orclib
import tracts_util
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

I, S = 40, 20000
SEG = 2048          # sites per lane of the kernels' count and emit passes


def _params(n):
    F = np.linspace(0.05, 0.95, n)
    A = np.full(n, 0.05)
    A[:min(5, n)] = 1e-3        # long tracts: whole chromosomes, several segments each
    return F, A


def _coords(t):
    return [(int(r["ind"]), int(r["first_site"]), int(r["n_sites"])) for r in t]


def _check(t, want, rtol=1e-12):
    assert _coords(t) == [w[:3] for w in want]
    np.testing.assert_allclose(t["post_sum"], [w[3] for w in want], rtol=rtol, atol=1e-300)
    np.testing.assert_array_equal(t["post_mean"], t["post_sum"] / t["n_sites"])


@pytest.fixture(scope="module")
def cohort(pkg):
    d = pkg.simulate.simulate(I, S, seed=7, n_chrom=3, indF="r", alpha="r", missing_rate=0.02)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    cs = np.isinf(d.pos_dist_mb)
    cs[0] = True
    return d, gl, cs


def test_exact_mode_viterbi_and_posterior(pkg, cohort, orc_det):
    d, gl, cs = cohort
    F, A = _params(I)
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_EXACT) as h:
        h.load(gl, d.pos_dist_mb)
        h.set_params(F, A, 0.2)
        h.init_emission()
        # before any decode: VITERBI is refused, POSTERIOR sees the zeros of no E-step
        with pytest.raises(pkg.NgsFHMMError) as ei:
            h.ibd_tracts("viterbi")
        assert ei.value.code == -10 and "Viterbi" in ei.value.message
        assert len(h.ibd_tracts("posterior", 1e-300)) == 0
        for _ in range(2):
            h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
        path = h.viterbi()
        marg = h.marg_prob
        t = h.ibd_tracts("viterbi")
        _check(t, tracts_util.rle_tracts(path, cs, marg))
        # the long tracts this cohort is built for: over three segments, at both chromosome ends
        spans = (t["first_site"] + t["n_sites"] - 1) // SEG - t["first_site"] // SEG
        assert spans.max() >= 3
        assert np.isin(t["first_site"], np.flatnonzero(cs)).any()
        ends = t["first_site"] + t["n_sites"]
        assert np.isin(ends, np.r_[np.flatnonzero(cs)[1:], S]).any()
        # the oracle's decode with the same parameters (det build: the same bits)
        em = orclib.OracleEM(orc_det, gl, d.pos_dist_mb)
        em.set_params(h.indF, h.alpha, h.freq)
        assert em.init_emission() == 0
        assert _coords(t) == [w[:3] for w in tracts_util.rle_tracts(em.viterbi(), cs)]
        # POSTERIOR: thresholds and minimum lengths against numpy
        for thr in (0.5, 0.9, 1.0):
            for m in (1, 50):
                tp = h.ibd_tracts("posterior", thr, m)
                _check(tp, tracts_util.rle_tracts(marg >= thr, cs, marg, m))
        tp = h.ibd_tracts("posterior", 0.5)
        assert ((tp["first_site"] + tp["n_sites"] - 1) // SEG - tp["first_site"] // SEG).max() >= 3
        # determinism, and the count / fetch contract of the C ABI
        for src, thr, m in (("viterbi", 0.5, 1), ("posterior", 0.5, 50)):
            a, b = h.ibd_tracts(src, thr, m), h.ibd_tracts(src, thr, m)
            assert a.tobytes() == b.tobytes()
        import ctypes as C
        n = C.c_uint64(0)
        buf = (pkg.hmm.Tract * 4)()
        assert h.lib.nghmm_ibd_tracts(h.handle, 0, 0.5, 1, C.cast(buf, C.c_void_p), 3, C.byref(n)) == 0
        assert n.value == len(t) > 3
        assert [(buf[k].ind, buf[k].first_site, buf[k].n_sites, buf[k].post_sum) for k in range(3)] == \
            [(int(r["ind"]), int(r["first_site"]), int(r["n_sites"]), float(r["post_sum"])) for r in t[:3]]
        assert buf[3].n_sites == 0 and all(buf[k].reserved == 0 for k in range(3))
        for thr in (0.0, -0.5, 1.5, float("nan")):
            with pytest.raises(pkg.NgsFHMMError) as ei:
                h.ibd_tracts("posterior", thr)
            assert ei.value.code == -10
        assert h.lib.nghmm_ibd_tracts(h.handle, 7, 0.5, 1, None, 0, C.byref(n)) == -10
        # a reload forgets the decode
        h.load(gl, d.pos_dist_mb)
        with pytest.raises(pkg.NgsFHMMError):
            h.ibd_tracts("viterbi")


@pytest.mark.parametrize("n_ind,n_sites,mode", [
    (70, 5003, "fast"), (1, 900, "fast"), (5, 10, "fast"), (64, 16, "fast"), (3, 7, "exact"),
    (130, 4099, "exact"),
])
def test_ragged_shapes(pkg, n_ind, n_sites, mode):
    d = pkg.simulate.simulate(n_ind, n_sites, seed=n_ind + n_sites, n_chrom=2 if n_sites > 20 else 1,
                              indF=0.7, alpha=0.05)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    cs = np.isinf(d.pos_dist_mb)
    cs[0] = True
    F, A = _params(n_ind)
    with pkg.NgsFHMM(n_ind, n_sites, mode=pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT) as h:
        h.load(gl, d.pos_dist_mb)
        h.set_params(F, A, 0.2)
        h.init_emission()
        h.iter_EM(1, indF_fixed=True, alpha_fixed=True)
        path, marg = h.viterbi(), h.marg_prob
        t = h.ibd_tracts("viterbi")
        _check(t, tracts_util.rle_tracts(path, cs, marg))
        assert len(t) > 0 or n_ind * n_sites < 1000
        for thr, m in ((0.5, 1), (0.9, 3)):
            _check(h.ibd_tracts("posterior", thr, m), tracts_util.rle_tracts(marg >= thr, cs, marg, m))


@pytest.mark.parametrize("n_shards", [2, 4])
def test_chain_merges_across_shards(pkg, cohort, n_shards):
    d, gl, cs = cohort
    F, A = _params(I)

    def make(lo, hi):
        h = pkg.NgsFHMM(I, hi - lo, mode=pkg.MODE_FAST)
        h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
        h.set_params(F, A, 0.2)
        h.init_emission()
        return h

    whole = make(0, S)
    whole.iter_EM(1, True, True)
    whole.viterbi()
    ref = whole.ibd_tracts("viterbi")
    long = ref[np.argmax(ref["n_sites"])]
    inside = int(long["first_site"] + long["n_sites"] // 2)            # inside a tract
    chrom = int(np.flatnonzero(cs)[1])                                   # at a chromosome start
    short = ref[(ref["n_sites"] >= 3) & (ref["first_site"] > chrom + 100)][0]
    after_end = int(short["first_site"] + short["n_sites"])             # a tract ends at a handle's last site
    cuts = [0, inside, S] if n_shards == 2 else [0] + sorted({inside, chrom, after_end}) + [S]
    assert len(cuts) == n_shards + 1
    hs = [make(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    ch = pkg.Chain(hs)
    ch.iter_EM(1, True, True)
    whole.set_params(hs[0].indF, hs[0].alpha, ch.freq)
    wp = whole.viterbi()
    cp = ch.viterbi()
    assert np.array_equal(cp, wp)
    marg = ch.marg_prob
    for m in (1, 50):
        t = ch.ibd_tracts("viterbi", min_sites=m)
        w = whole.ibd_tracts("viterbi", min_sites=m)
        assert _coords(t) == _coords(w)
        _check(t, tracts_util.rle_tracts(cp, cs, marg, m))
        np.testing.assert_allclose(t["post_sum"], w["post_sum"], rtol=1e-8)
    # min_sites after the merge: the tract the first cut halves survives whole
    w = whole.ibd_tracts("viterbi")
    cut = w[(w["ind"] == long["ind"]) & (w["first_site"] < inside) &
            (w["first_site"] + w["n_sites"] > inside)]
    assert len(cut) == 1
    t = ch.ibd_tracts("viterbi", min_sites=int(cut[0]["n_sites"]))
    assert (int(cut[0]["ind"]), int(cut[0]["first_site"]), int(cut[0]["n_sites"])) in _coords(t)
    tp = ch.ibd_tracts("posterior", 0.5, 2)
    _check(tp, tracts_util.rle_tracts(marg >= 0.5, cs, marg, 2))
    assert ch.ibd_tracts("viterbi").tobytes() == ch.ibd_tracts("viterbi").tobytes()
    for h in hs:
        h.close()
    whole.close()


CLI_I, CLI_S = 12, 3001


@pytest.fixture(scope="module")
def cli_data(pkg, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tracts_cli"))
    d = pkg.simulate.simulate(CLI_I, CLI_S, seed=31, n_chrom=3, indF=0.6, alpha=0.05)
    paths = cli_util.write_inputs(tmp, d, d.gl)
    names = os.path.join(tmp, "names.txt")
    with open(names, "w") as fh:
        fh.write("".join(f"IND_{i:03d} pop{i % 2}\n" for i in range(CLI_I)))
    return paths, names, tmp


@pytest.mark.parametrize("tag,extra,named", [
    ("exact", ["--mode", "exact"], False),
    ("exact_named", ["--mode", "exact"], True),
    ("fast_named", ["--mode", "fast"], True),
    ("chain", ["--mode", "fast", "--n_gpus", 2, "--devices", "0,0"], False),
])
def test_cli_ibd_bed(cli_data, tag, extra, named):
    paths, names, tmp = cli_data
    base = ["--geno", paths["glf_gz"], "--loglkl", "--pos", paths["pos_gz"], "--n_ind", CLI_I,
            "--n_sites", CLI_S, "--freq", 0.1, "--indF", "0.6,0.05", "--min_iters", 2, "--max_iters", 3,
            "--verbose", 0] + extra
    plain, bed = os.path.join(tmp, f"plain_{tag}"), os.path.join(tmp, f"bed_{tag}")
    cli_util.run_cli(base + ["--out", plain])
    cli_util.run_cli(base + ["--out", bed, "--ibd_bed"] + (["--ind_names", names] if named else []))
    ids = [f"IND_{i:03d}" for i in range(CLI_I)] if named else [f"ind{i}" for i in range(CLI_I)]
    want = tracts_util.convert_ibd(bed + ".ibd", paths["pos_gz"], ids)
    assert want.count("\n") >= CLI_I
    assert open(bed + ".ibd.bed").read() == want
    for ext in (".indF", ".ibd", ".geno"):
        assert open(plain + ext, "rb").read() == open(bed + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".ibd.bed")
