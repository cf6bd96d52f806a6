"""Decode problems for the Viterbi kernels chosen by the test, not by an EM run.

case(I, S, seed) returns (gl [S][I][3] normalised natural-log likelihoods, pos_dist [S] in Mb,
indF [I], alpha [I], freq [S]): simulated sequencing data (simulate.simulate with 5 % missing
cells, random true F and allele frequencies) whose parameters are SET, so that the edges that
shape a path are met on purpose:

  * indF ~ U(0.02, 0.9) and alpha = 10^U(-3, 1) per individual: tracts of a few sites next to
    tracts of whole chromosomes in one launch;
  * individuals 0-3 sit in the corners of the parameter box, CORNERS;
  * individuals 4, 5 and I - 1 have no data at all (every cell log(1/3)) and F = 0.3, 0.5 (exactly)
    and 0.7: the transition terms and the tie rule alone decide their paths; the last of them is
    the last lane of a ragged last workgroup;
  * chromosome starts (pos_dist = +inf) at sites 63, 64, 65 and, for every chunk length c of
    CHUNKS, at the last multiple of c inside the case and at its two neighbours: a chain that
    restarts one site before, on and one site after a block, group and chunk edge.

Cohorts of fewer than 8 individuals have neither (a lone individual in a corner would be a
constant path).  sweep() lists the (I, chunk, S) the GPU test decodes; the CPU test holds
every one of them to the conditions that make a broken carry visible.  Numpy and the package's
simulator only; fixed seeds; no GPU.
"""
import importlib

import numpy as np

# (F, alpha): the bounds of the reference's optimizer
CORNERS = ((1e-15, 1e-15), (1 - 1e-15, 10.0), (0.5, 1e-15), (0.5, 10.0))
NO_DATA_F = (0.3, 0.5, 0.7)
CHUNKS = (16, 64, 80, 256)       # values of the switch viterbi_chunk that the GPU test sets
COHORTS = (1, 63, 64, 65, 129, 1100)
FULL_COHORTS = (65, 1100)        # every remainder at these
MULTIPLES = (1, 2, 5)
# sites past k chunks: the last group of 8 not whole, one group, one group and a site, a block of
# 16 and its neighbours, fewer groups than the six loader waves, exactly six, and one more site
REMAINDERS = (0, 1, 7, 8, 9, 15, 16, 17, 47, 48, 49)
FEW_REMAINDERS = (0, 7, 17, 49)
BACK_SITES = (1, 15, 16, 17, 255, 256, 257, 271, 272, 273, 4095, 4096, 4097)

# seeds other than the default (= I), for cases whose default draw misses a condition of
# tests/test_viterbi_cases_cpu.py: {(I, S): seed}
SEEDS = {(65, 209): 1065, (65, 415): 1065, (65, 561): 1065}


def chunk_sites(S, I, forced=0):
    """viterbi_chunk_sites (csrc/kernels_exact.hip) restated: the sites per chunk of the forward
    sweep, `forced` being the switch viterbi_chunk."""
    ch = (2 << 30) // (I * 32) & ~15
    ch = max(ch, 64)
    ch = min(ch, (S + 15) & ~15)
    if forced <= 0:
        return ch
    return min(max(forced & ~15, 16), ch)


def boundaries(S, I, forced):
    """First sites of the chunks after the first."""
    c = chunk_sites(S, I, forced)
    return list(range(c, S, c))


def chrom_starts(S):
    at = {63, 64, 65}
    for c in CHUNKS:
        m = (S - 1) // c * c
        if m >= c:
            at |= {m - 1, m, m + 1}
    return sorted(s for s in at if 1 <= s < S)


def case(I, S, seed=None):
    if seed is None:
        seed = SEEDS.get((I, S), I)
    sim = importlib.import_module("ngsf-hmm_amd.simulate")
    d = sim.simulate(I, S, seed=seed, missing_rate=0.05, indF="r", alpha=0.5, freq="r")
    gl = sim.normalise_log_gl(d.gl)
    pos = d.pos_dist_mb.copy()
    rng = np.random.default_rng([seed, I, S])
    F = rng.uniform(0.02, 0.9, I)
    A = 10.0 ** rng.uniform(-3, 1, I)
    if I >= 8:
        for i, (f, a) in enumerate(CORNERS):
            F[i], A[i] = f, a
        for i, f in zip((4, 5, I - 1), NO_DATA_F):
            gl[:, i, :] = np.log(1.0 / 3.0)
            F[i] = f
    pos[chrom_starts(S)] = np.inf
    return gl, pos, F, A, d.freq.copy()


def no_data_individuals(I):
    return (4, 5, I - 1) if I >= 8 else ()


def sweep_sites(I, chunk):
    """The site counts decoded at cohort I with viterbi_chunk = chunk (0: the default length,
    which none of these sizes reaches: the same counts as for 64, in one chunk)."""
    c = chunk if chunk else 64
    if I == 65:
        ks, rs = MULTIPLES, REMAINDERS
    elif I == 1100:      # (the largest: every remainder, every multiple at the short chunks only)
        ks, rs = (MULTIPLES if 0 < chunk <= 64 else (2,)), REMAINDERS
    else:
        ks, rs = (2,), FEW_REMAINDERS
    return sorted({k * c + r for k in ks for r in rs})


def sweep():
    """(I, chunk, S) of the GPU test's chunk sweep."""
    return [(I, c, S) for I in COHORTS for c in CHUNKS + (0,) for S in sweep_sites(I, c)]


# one handle decoded under one chunk length after another (rounded: 100 -> 96, 7 -> 16, 10^6 -> the
# default), 0 last
MANY = (200, 2049, (64, 16, 80, 256, 100, 7, 10 ** 6, 0))

# fast mode: (I, S, chunk of the single handle, chains); a chain = (cuts, one chunk per handle) with
# unequal ranges whose cuts are no multiples of 16
FAST = (
    (65, 1030, 80, (((0, 391, 1030), (64, 80)), ((0, 201, 643, 1030), (16, 80, 64)))),
    (1100, 700, 64, (((0, 333, 700), (80, 64)), ((0, 250, 457, 700), (64, 16, 80)))),
)


def chain_boundaries(I, cuts, chunks):
    """Global first sites of every chunk but the first of a chain of handles: the cuts and, inside
    handle r (sites cuts[r] .. cuts[r+1]), its own chunk boundaries."""
    out = []
    for lo, hi, c in zip(cuts[:-1], cuts[1:], chunks):
        if lo:
            out.append(lo)
        out += [lo + b for b in boundaries(hi - lo, I, c)]
    return out


def check_boundaries(path, bounds):
    """The conditions under which a broken carry at one of `bounds` shows in the path [I][S]: at
    every boundary b somebody is in state 0, somebody in state 1, and somebody switches state
    within [b - 8, b + 8).  Returns per boundary (b, in state 0, in state 1, switching)."""
    S = path.shape[1]
    sw = switch_sites(path)
    out = []
    for b in bounds:
        row = (b, int((path[:, b] == 0).sum()), int((path[:, b] == 1).sum()),
               int(sw[:, max(b - 8, 1):min(b + 8, S)].any(axis=1).sum()))
        assert min(row[1:]) >= 1, row
        out.append(row)
    return out


def check_back_pointers(back):
    """Both back-pointer bits take both values: all four predecessor choices occur."""
    assert len(np.unique(back & 1)) == 2 and len(np.unique(back >> 1)) == 2


def switch_sites(path):
    """[I][S] bool: the state at site s differs from the state at s - 1 (False at s = 0)."""
    sw = np.zeros(path.shape, dtype=bool)
    sw[:, 1:] = path[:, 1:] != path[:, :-1]
    return sw
