"""tests/viterbi_cases.py without a GPU: the generator is deterministic and builds what it says,
its restatement of the chunk length is the C code's, and on every shape and chunk length that
tests/test_gpu_viterbi.py decodes the ORACLE's path meets the conditions under which a broken
carry between two chunks would show: both states occupied at every chunk boundary, a switch of
state within eight sites of it, and all four predecessor choices somewhere in the case."""
import os
import re

import numpy as np
import pytest

import orclib
import viterbi_cases as vc

THREADS = min(16, os.cpu_count() or 1)


def _oracle(orc, I, S):
    gl, pos, F, A, freq = vc.case(I, S)
    em = orclib.OracleEM(orc, gl, pos)
    em.set_params(F, A, freq)
    assert em.init_emission() == 0
    path, back = em.viterbi_back(THREADS)
    assert np.array_equal(path, em.viterbi(THREADS))
    em.close()
    return path, back


def test_generator_is_deterministic_and_well_formed(pkg):
    for I, S in ((1, 17), (3, 70), (65, 1030), (129, 300)):
        a, b = vc.case(I, S), vc.case(I, S)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        gl, pos, F, A, freq = a
        assert gl.shape == (S, I, 3) and pos.shape == (S,) and F.shape == A.shape == (I,)
        assert freq.shape == (S,) and np.all((freq >= 0) & (freq <= 1))
        assert np.all(np.isfinite(gl)) and np.allclose(np.exp(gl).sum(axis=-1), 1.0, rtol=1e-9)
        assert np.all((F >= 1e-15) & (F <= 1 - 1e-15)) and np.all((A >= 1e-15) & (A <= 10))
        if I >= 8:
            assert list(zip(F[:4], A[:4])) == list(vc.CORNERS)
        starts = [s for s in np.flatnonzero(np.isinf(pos)) if s > 0]
        assert starts == vc.chrom_starts(S)
        assert np.all(pos[np.isfinite(pos)] > 0)
        if S > 66:
            assert {63, 64, 65} <= set(starts)
        for c in vc.CHUNKS:          # on a multiple of every chunk length, and on both neighbours
            if S > c + 1:
                assert any(s % c == 0 and {s - 1, s + 1} <= set(starts) for s in starts), c
        nd = vc.no_data_individuals(I)
        assert len(nd) == (3 if I >= 8 else 0)
        for i, f in zip(nd, vc.NO_DATA_F):
            assert np.all(gl[:, i, :] == np.log(1.0 / 3.0)) and F[i] == f
        assert sorted(vc.NO_DATA_F)[0] < 0.5 < sorted(vc.NO_DATA_F)[2] and 0.5 in vc.NO_DATA_F
        informative = np.ptp(gl, axis=-1).max(axis=0) > 0
        assert informative.sum() == I - len(nd)
    assert not np.array_equal(vc.case(65, 300, seed=1)[0], vc.case(65, 300, seed=2)[0])
    assert all((I, S) in {(i, s) for i, _, s in vc.sweep()} for I, S in vc.SEEDS)


def test_chunk_length_is_the_c_code(pkg):
    """chunk_sites() restates viterbi_chunk_sites, switch included; the formula is read back from
    the kernel source, and the kernels' group, slot, block and prefetch sizes that REMAINDERS and
    BACK_SITES straddle are the source's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "ngsf-hmm_amd", "csrc", "kernels_exact.hip")).read()
    body = src[src.index("uint64_t viterbi_chunk_sites(uint64_t S, uint64_t I, int64_t forced) {"):]
    body = re.sub(r"\s*//[^\n]*", "", body[:body.index("\n}\n")])
    assert [ln.strip() for ln in body.split("\n")[1:]] == [
        "uint64_t ch = (2ull << 30) / (I * 32);",
        "ch &= ~15ull;",
        "if (ch < 64) ch = 64;",
        "const uint64_t Sp = (S + 15) & ~15ull;",
        "if (ch > Sp) ch = Sp;",
        "if (forced <= 0) return ch;",
        "uint64_t n = (uint64_t)forced & ~15ull;",
        "if (n < 16) n = 16;",
        "return n < ch ? n : ch;",
    ]
    for name, value in (("VG", 8), ("VNL", 6), ("UV", 16), ("PFB", 16)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert '{"viterbi_chunk", &Switches::viterbi_chunk}' in open(
        os.path.join(root, "ngsf-hmm_amd", "csrc", "kernels_fast.hip")).read()
    # the rule: down to a multiple of 16, at least 16, never more than the default; 0 = the default
    assert vc.chunk_sites(10 ** 6, 1000) == 67104 and vc.chunk_sites(10 ** 6, 100) == 671088
    assert vc.chunk_sites(10 ** 5, 100) == 100000 and vc.chunk_sites(600, 129) == 608
    assert vc.chunk_sites(3353, 20000) == 3344 and vc.chunk_sites(10 ** 4, 10 ** 7) == 64
    for forced, want in ((0, 2064), (-5, 2064), (1, 16), (15, 16), (16, 16), (17, 16), (31, 16),
                         (32, 32), (100, 96), (256, 256), (2063, 2048), (2064, 2064), (10 ** 6, 2064)):
        assert vc.chunk_sites(2049, 129, forced) == want, forced
    assert vc.chunk_sites(7, 5, 64) == 16 and vc.chunk_sites(17, 5, 64) == 32
    # the remainders sit on both sides of a group (VG), a block (UV) and VNL groups
    assert {7, 8, 9, 15, 16, 17, 47, 48, 49} <= set(vc.REMAINDERS) and 6 * 8 == 48
    assert {255, 256, 257} <= set(vc.BACK_SITES) and 16 * 16 == 256
    # every switched sweep case crosses at least one boundary unless it is exactly one chunk
    for I, c, S in vc.sweep():
        if c:
            assert len(vc.boundaries(S, I, c)) == (S - 1) // c and (S > c or S == c)
        else:
            assert vc.boundaries(S, I, 0) == []
    assert {c for _, c, _ in vc.sweep()} == set(vc.CHUNKS) | {0}
    for I in vc.FULL_COHORTS:
        for c in vc.CHUNKS:
            assert all(any(k * c + r in vc.sweep_sites(I, c) for k in vc.MULTIPLES) for r in vc.REMAINDERS)


@pytest.mark.parametrize("I", vc.COHORTS)
def test_sweep_cases_can_expose_a_broken_carry(orc_det, pkg, I):
    """A single individual cannot be in both states at once, so at I = 1 the conditions cannot hold
    boundary by boundary: there, for every chunk length, some case switches state within eight
    sites of a boundary."""
    sites = {}
    for _, c, S in (x for x in vc.sweep() if x[0] == I):
        sites.setdefault(S, []).append(c)
    worst = [10 ** 9] * 3
    lone = {c: 0 for c in vc.CHUNKS}
    for S, chunks in sorted(sites.items()):
        path, back = _oracle(orc_det, I, S)
        if I == 1:
            sw = vc.switch_sites(path)
            for c in (c for c in chunks if c):
                lone[c] += any(sw[:, max(b - 8, 1):min(b + 8, S)].any() for b in vc.boundaries(S, I, c))
            continue
        vc.check_back_pointers(back)
        for c in chunks:
            for row in vc.check_boundaries(path, vc.boundaries(S, I, c)):
                worst = [min(w, r) for w, r in zip(worst, row[1:])]
    if I == 1:
        assert min(lone.values()) >= 1, lone
        return
    print("I = %d: over all boundaries, at least %d in state 0, %d in state 1, %d switching within 8 "
          "sites" % ((I,) + tuple(worst)))


def test_other_gpu_cases_can_expose_a_broken_carry(orc_det, pkg):
    I, S, chunks = vc.MANY
    path, back = _oracle(orc_det, I, S)
    vc.check_back_pointers(back)
    for c in chunks:
        vc.check_boundaries(path, vc.boundaries(S, I, c))
    assert vc.boundaries(S, I, 0) == [] and len(vc.boundaries(S, I, 16)) == 128
    for I, S, c, chains in vc.FAST:
        path, back = _oracle(orc_det, I, S)
        vc.check_back_pointers(back)
        assert vc.check_boundaries(path, vc.boundaries(S, I, c))
        for cuts, cs in chains:
            assert cuts[0] == 0 and cuts[-1] == S and len(cs) == len(cuts) - 1
            assert all(x % 16 for x in cuts[1:-1])
            assert len({b - a for a, b in zip(cuts[:-1], cuts[1:])}) == len(cs)     # unequal
            # every handle after the first takes scores over AND crosses a chunk of its own
            assert all(len(vc.boundaries(b - a, I, c_)) >= 1 for a, b, c_ in zip(cuts[:-1], cuts[1:], cs))
            vc.check_boundaries(path, vc.chain_boundaries(I, cuts, cs))


def test_what_the_oracle_decides_for_the_pinned_individuals(orc_det, pkg):
    """Not asserted as a truth about the model, only recorded so that a change of the generator is
    seen: the paths of the corner and no-data individuals at 65 x 1030."""
    path, _ = _oracle(orc_det, 65, 1030)
    assert not path[0].any() and path[1].all()           # F at its bounds
    assert 0 < path[3].sum() < 1030                      # F = 0.5, alpha = 10: the data decide
    nd = vc.no_data_individuals(65)
    assert not path[nd[0]].any() and path[nd[2]].all()   # F = 0.3 / F = 0.7 without data
    assert not path[nd[1]].any()                         # F = 0.5 without data: ties go to state 0
