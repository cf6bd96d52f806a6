"""The Viterbi decode (k_trans_log_exact, k_viterbi_fwd_pc / k_viterbi_fwd_exact, k_viterbi_back)
against the oracle's path, cell for cell, on the decode problems of tests/viterbi_cases.py: across
the chunks of the forward sweep (switch viterbi_chunk, include/nghmm_debug.h), across every
remainder of sites that the groups of 8, blocks of 16, six loader waves and prefetch groups of 256
treat differently, in both modes, over chains of site shards, and once across a chunk boundary
that the production formula sets by itself.  tests/test_viterbi_cases_cpu.py shows on the oracle
alone that these cases would show a broken carry.  No tolerances: np.array_equal."""
import time

import numpy as np
import pytest

import orclib
import tracts_util
import viterbi_cases as vc
from conftest import has_gpu
from siteshard_util import Chain

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def _oracle(orc_det, case, n_threads=16):
    gl, pos, F, A, freq = case
    em = orclib.OracleEM(orc_det, gl, pos)
    em.set_params(F, A, freq)
    assert em.init_emission() == 0
    return em, em.viterbi(n_threads)


def _handle(pkg, mode, case):
    gl, pos, F, A, freq = case
    h = pkg.NgsFHMM(gl.shape[1], gl.shape[0], mode=mode)
    try:
        h.load(gl, pos)
        h.set_params(F, A, freq)
        h.init_emission()
    except BaseException:
        h.close()
        raise
    return h


def _same(got, want, what, chunk=0):
    """np.array_equal, and where the first difference sits relative to the kernels' edges."""
    if np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    i, s = (int(x[0]) for x in np.nonzero(got != want))
    ss = np.flatnonzero((got != want).any(axis=0))
    where = "individual %d (lane %d), site %d of %d: block %d + %d, group of 8 + %d, 256-group + %d" % (
        i, i % 64, s, want.shape[1], s // 16, s % 16, s % 8, s % 256)
    if chunk:
        where += ", chunk %d + %d" % (s // chunk, s % chunk)
    raise AssertionError("%s: %d cells of %d individuals differ from the oracle, at sites %d..%d; first: %s"
                         % (what, int((got != want).sum()), int((got != want).any(axis=1).sum()),
                            ss[0], ss[-1], where))


@pytest.mark.parametrize("I,chunk", [(I, c) for I in vc.COHORTS for c in vc.CHUNKS + (0,)])
def test_chunk_sweep_exact(pkg, orc_det, I, chunk):
    """(a) S = k * chunk + r sites in chunks of `chunk` (0: the default, one chunk), with the
    producer-consumer kernel and with its one-lane-per-individual twin."""
    for S in vc.sweep_sites(I, chunk):
        case = vc.case(I, S)
        em, want = _oracle(orc_det, case)
        em.close()
        with _handle(pkg, pkg.MODE_EXACT, case) as h:
            h.set_switch("viterbi_chunk", chunk)
            for serial in (0, 1):
                h.set_switch("exact_serial", serial)
                _same(h.viterbi(), want, "%d x %d, chunk %d, exact_serial %d" % (I, S, chunk, serial),
                      vc.chunk_sites(S, I, chunk))


def test_one_handle_many_chunk_lengths(pkg, orc_det):
    """(b) The switch may change between two decodes of one handle (the scratch is sized once):
    every chunk length gives the first path, and what reads the blocked path that the trace-back
    wrote -- the tracts, the genotype posteriors -- gives the oracle's too."""
    I, S, chunks = vc.MANY
    case = vc.case(I, S)
    em, want = _oracle(orc_det, case)
    cs = np.isinf(case[1])
    want_tracts = [w[:3] for w in tracts_util.rle_tracts(want, cs)]
    want_geno = em.geno_post(want)
    em.close()
    with _handle(pkg, pkg.MODE_EXACT, case) as h:
        h.estep()                                # (the tracts sum posteriors)
        first = None
        for serial in (0, 1):
            h.set_switch("exact_serial", serial)
            for c in chunks:
                h.set_switch("viterbi_chunk", c)
                got = h.viterbi()
                what = "%d x %d, chunk %d after others, exact_serial %d" % (I, S, c, serial)
                _same(got, want, what, vc.chunk_sites(S, I, c))
                first = got if first is None else first
                assert np.array_equal(got, first), what
                t = h.ibd_tracts("viterbi")
                assert [(int(r["ind"]), int(r["first_site"]), int(r["n_sites"])) for r in t] == want_tracts, what
                assert np.array_equal(h.geno_posteriors(), want_geno), what
        with pytest.raises(pkg.NgsFHMMError):
            h.set_switch("viterbi_chunks", 64)


@pytest.mark.parametrize("I", (1, 65))
def test_trace_back_edges(pkg, orc_det, I):
    """(c) The chunk at its default; S on both sides of the trace-back's block of 16 sites and
    prefetch group of 256, and many groups."""
    for S in vc.BACK_SITES:
        case = vc.case(I, S)
        em, want = _oracle(orc_det, case)
        em.close()
        with _handle(pkg, pkg.MODE_EXACT, case) as h:
            for serial in (0, 1):
                h.set_switch("exact_serial", serial)
                _same(h.viterbi(), want, "%d x %d, exact_serial %d" % (I, S, serial))


@pytest.mark.parametrize("I,S,chunk,chains", vc.FAST)
def test_fast_mode_and_site_shards(pkg, orc_det, I, S, chunk, chains):
    """(d) Fast mode decodes with the same kernels on recomputed log emissions.  One handle in
    short chunks; then chains of handles over unequal site ranges, each with a chunk length of
    its own: a handle after the first takes the scores of the one before (chain_start false) AND
    carries them over its own chunks, through the state doubles behind the transition logs.
    Every path is held to the oracle's path of the whole problem."""
    case = vc.case(I, S)
    gl, pos, F, A, freq = case
    em, want = _oracle(orc_det, case)
    em.close()
    cs = np.isinf(pos)
    want_tracts = [w[:3] for w in tracts_util.rle_tracts(want, cs)]
    with _handle(pkg, pkg.MODE_FAST, case) as h:
        h.estep()                                # (the tracts sum posteriors)
        for c in (chunk, 0, 16):
            h.set_switch("viterbi_chunk", c)
            _same(h.viterbi(), want, "fast %d x %d, chunk %d" % (I, S, c), vc.chunk_sites(S, I, c))
            t = h.ibd_tracts("viterbi")
            assert [(int(r["ind"]), int(r["first_site"]), int(r["n_sites"])) for r in t] == want_tracts
    for cuts, chunks in chains:
        ranges = list(zip(cuts[:-1], cuts[1:]))
        what = "fast %d x %d, shards %s with chunks %s" % (I, S, cuts, chunks)
        # the two halves called one by one (tests/siteshard_util.py)
        ch = Chain(pkg, gl, pos, len(ranges), ranges=ranges)
        try:
            ch.set_params(F, A, freq)
            for h, c in zip(ch.h, chunks):
                h.set_switch("viterbi_chunk", c)
            _same(ch.viterbi(), want, what + " (shard_forward / shard_back)")
            for h in ch.h:                       # ... and again with every handle in one chunk
                h.set_switch("viterbi_chunk", 0)
            _same(ch.viterbi(), want, what + " (default chunks)")
        finally:
            ch.close()
        # the library's own chain (nghmm_chain_viterbi)
        hs = []
        try:
            for (lo, hi), c in zip(ranges, chunks):
                hs.append(_handle(pkg, pkg.MODE_FAST, (np.ascontiguousarray(gl[lo:hi]),
                                                      np.ascontiguousarray(pos[lo:hi]), F, A, freq[lo:hi])))
                hs[-1].set_switch("viterbi_chunk", c)
            chain = pkg.Chain(hs)
            _same(chain.viterbi(), want, what + " (Chain.viterbi)")
        finally:
            for h in hs:
                h.close()


def test_a_chunk_boundary_of_the_production_formula(pkg, orc_det):
    """(e) No switch: 20 000 individuals make the formula's chunk 3344 sites, and 3353 sites cross
    it with a last group of one site after a whole one.  The likelihoods are those of 500
    simulated individuals 40 times over (the simulator at 20 000 x 3353 costs more than the test),
    every individual with parameters of its own; one allele frequency for all sites.  On the
    CPU alone the data take 3 s and the oracle 28 s (16 threads); the test prints its parts."""
    I0, S, reps = 500, 3344 + 9, 40
    I = I0 * reps
    assert vc.chunk_sites(S, I) == 3344 and vc.boundaries(S, I, 0) == [3344]
    t0 = time.time()
    gl0, pos, F0, A0, _ = vc.case(I0, S)
    gl = np.tile(gl0, (1, reps, 1))
    rng = np.random.default_rng([I, S])
    F = np.concatenate([F0, rng.uniform(0.02, 0.9, I - I0)])
    A = np.concatenate([A0, 10.0 ** rng.uniform(-3, 1, I - I0)])
    case = (gl, pos, F, A, 0.25)
    t1 = time.time()
    em = orclib.OracleEM(orc_det, gl, pos)
    em.set_params(F, A, 0.25)
    assert em.init_emission() == 0
    want, back = em.viterbi_back(16)
    em.close()
    vc.check_back_pointers(back)
    del back
    vc.check_boundaries(want, [3344])
    t2 = time.time()
    with _handle(pkg, pkg.MODE_EXACT, case) as h:
        for serial in (0, 1):
            h.set_switch("exact_serial", serial)
            _same(h.viterbi(), want, "%d x %d, exact_serial %d" % (I, S, serial), 3344)
    with _handle(pkg, pkg.MODE_FAST, case) as h:
        _same(h.viterbi(), want, "fast %d x %d" % (I, S), 3344)
    print("production chunk: data %.1f s, oracle %.1f s, GPU handles and decodes %.1f s"
          % (t1 - t0, t2 - t1, time.time() - t2))
