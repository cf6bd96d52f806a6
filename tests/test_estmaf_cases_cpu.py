"""tests/estmaf_cases.py without a GPU: the generator is deterministic, every family is present
at every cohort size the GPU test uses, and the conditions under which the GPU test may leave a
site out of its value comparison hold for the reference alone on the committed seeds."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import estmaf_cases as ec

THREADS = min(16, os.cpu_count() or 1)


def test_generator_is_deterministic_and_well_formed():
    for I in (1, 3, 65, 257):
        a = ec.cases(I)
        b = ec.cases(I)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        gl, post, labels = a
        assert gl.shape == (ec.N_SITES, I, 3) and post.shape == (ec.N_SITES, I)
        assert np.all(np.isfinite(gl)) and np.all(gl <= 0)
        # normalised as simulate.normalise_log_gl leaves them: the three likelihoods sum to one
        assert np.allclose(np.exp(gl).sum(axis=-1), 1.0, rtol=1e-12)
        assert np.all((post >= 0) & (post <= 1))
    other = ec.cases(65, seed=ec.SEED + 1)
    assert not np.array_equal(other[1], ec.cases(65)[1])
    assert ec.N_SITES >= 300 and ec.N_SITES % len(ec.RECIPES) == 0


def test_size_classes_are_the_dispatch_of_the_kernel_source():
    """size_class() restates fast_estmaf's table and estmaf_full_slots(); both are read back from
    the kernel source so that the edge individuals stay on the edge when the dispatch moves."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "ngsf-hmm_amd", "csrc", "kernels_fast_estmaf.hip")).read()
    table = re.findall(r"I_tot <= (\d+)\) LAUNCH_NI\((\d+), (\d+)\)", src)
    assert len(table) == 13 and "else LAUNCH_NI(16, 512);" in src
    for top, ni, block in table:
        assert ec.size_class(int(top))[:2] == (int(ni), int(block))
        assert ec.size_class(int(top) + 1)[:2] != (int(ni), int(block))
        assert int(top) in ec.SIZES and int(top) + 1 in ec.SIZES
    assert ec.size_class(8192)[:2] == (16, 512) and ec.size_class(8193) is None
    assert "BLOCK == 64 ? (NI == 16 ? 12 : NI == 12 ? 8 : NI == 8 ? 4 : NI == 4 ? 2 : NI == 2 ? 1 : 0)" in src
    assert ": (NI == 16 ? 8 : 0);" in src
    for I in ec.SIZES:
        sc = ec.size_class(I)
        if sc and sc[2]:
            # a class with unmasked slots only ever holds cohorts that fill them
            assert I > sc[2] * sc[1] - 1 and ec.edge_index(I) == sc[2] * sc[1] - 1


@pytest.mark.parametrize("I", ec.SIZES)
def test_every_family_at_every_size(I):
    gl, post, labels = ec.cases(I)
    for f in ec.FAMILIES:
        assert np.sum(labels == f) >= ec.N_SITES // len(ec.RECIPES), f
    sub = ec.anchor_sites(labels)
    assert set(labels[sub]) == set(ec.FAMILIES) and set(range(len(ec.RECIPES))) <= set(sub.tolist())
    assert np.all(np.isin(np.flatnonzero(np.isin(labels, ec.ANCHOR_EVERY_SITE)), sub))
    # the posterior families are what they say
    for s in np.flatnonzero(np.isin(labels, ec.ONE_MINUS_EPS)):
        assert np.all(post[s] < 1.0) and np.all(1.0 - post[s] <= 1.0000001e-9)
    for s in np.flatnonzero(np.isin(labels, ("post_snapped", "called_snapped"))):
        assert np.all((post[s] == 0) | (post[s] == 1))
    for s in np.flatnonzero(labels == "post_tiny"):
        assert np.all((post[s] == 1e-300) | (post[s] == 1e-17))
    # called heterozygotes at posterior exactly 1: the log-space route, on every het1 site
    logsp = ec.log_space_sites(gl, post)
    assert np.all(logsp[labels == "called_het1"])
    assert set(labels[logsp]) <= {"called_het1", "called_snapped"}
    # one informative individual where the family says
    e = ec.edge_index(I)
    for f, at in (("one_first", 0), ("one_edge_m1", e), ("one_edge", min(e + 1, I - 1)),
                  ("one_last", I - 1)):
        for s in np.flatnonzero(labels == f):
            informative = np.flatnonzero(np.ptp(gl[s], axis=-1) > 0)
            assert list(informative) == [at], (f, informative)


@pytest.mark.parametrize("I", ec.SIZES)
def test_reference_stopping_decisions_are_rarely_marginal(orc_libm, I):
    """The GPU test may leave a site out of its value comparison when some pass of the reference
    has |delta| within 1e-6 (relative) of the threshold 1e-5: at most 0.5 % of a size's sites."""
    gl, post, labels = ec.cases(I)

    def one(s):
        f, n, d = orc_libm.est_maf_trace(gl[s], post[s])
        f0, n0 = orc_libm.est_maf(gl[s], post[s]) if s % 16 == 0 else (f, n)
        assert f == f0 and n == n0 and len(d) == n and 1 <= n <= 101
        assert np.isfinite(f) and 0 <= f <= 1
        return ec.marginal(d)

    with ThreadPoolExecutor(THREADS) as pool:
        marginal = np.array(list(pool.map(one, range(len(labels)))))
    assert marginal.sum() <= 0.005 * len(labels), np.flatnonzero(marginal)


@pytest.mark.parametrize("I", (65, 1025))
def test_oracle_and_anchor_agree_on_the_pass_count(orc_libm, I):
    """... or when the double oracle and the binary128 anchor stop after different numbers of
    passes (on the subsample the anchor is computed on at large cohorts)."""
    import orclib
    anchor = orclib.HpAnchor()
    gl, post, labels = ec.cases(I)
    sub = ec.anchor_sites(labels)
    sub = sub[~ec.log_space_sites(gl, post)[sub]]

    def one(s):
        return orc_libm.est_maf(gl[s], post[s])[1] != anchor.est_maf(gl[s], post[s])[1]

    with ThreadPoolExecutor(THREADS) as pool:
        differ = np.array(list(pool.map(one, sub)))
    assert differ.sum() <= 0.005 * len(labels), sub[differ]


def test_marginal_is_a_band_around_the_threshold():
    assert ec.marginal([1e-2, 1e-5 * (1 + 5e-7)]) and ec.marginal([1e-5 * (1 - 9e-7), 0.0])
    assert not ec.marginal([1e-2, 1e-5 * (1 + 2e-6), 1e-5 * (1 - 2e-6)])
