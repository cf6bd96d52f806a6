"""What the nine chain entry points that walk the shards themselves (nghmm_chain_sample_paths,
_obs_info, _tract_support, _tract_bounds, _freq_info, _geno_smooth, _ibd_expect, _ibd_moments,
_ibd_by_length; include/nghmm.h) answer before they touch the device: handles that are no chain,
and a chain whose handles hold no data.  Every call returns an error and launches nothing."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

I, CUTS = 3, (0, 300, 640)     # two fast-mode site shards (test_gpu_siteshard.py's 3 x 640)
ONE = [[0, 0, 1]]              # one tract record: individual 0, site 0

# (the C name's tail, the call through hmm.Chain's own wrapper)
ENTRY_POINTS = [
    ("sample_paths", lambda ch: ch.sample_paths(1)),
    ("obs_info", lambda ch: ch.obs_info()),
    ("tract_support", lambda ch: ch.tract_support(ONE)),
    ("tract_bounds", lambda ch: ch.tract_bounds(ONE)),
    ("freq_info", lambda ch: ch.freq_info()),
    ("geno_smooth", lambda ch: ch.geno_smooth()),
    ("ibd_expect", lambda ch: ch.ibd_expect()),
    ("ibd_moments", lambda ch: ch.ibd_moments()),
    ("ibd_by_length", lambda ch: ch.ibd_by_length(1)),
]


def _handles(pkg, load):
    hs = [pkg.NgsFHMM(I, hi - lo, mode=pkg.MODE_FAST) for lo, hi in zip(CUTS[:-1], CUTS[1:])]
    if load:
        d = pkg.simulate.simulate(I, CUTS[-1], seed=I + CUTS[-1], n_chrom=2, missing_rate=0.1, indF="r")
        gl = pkg.simulate.normalise_log_gl(d.gl)
        for h, lo, hi in zip(hs, CUTS[:-1], CUTS[1:]):
            h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(d.pos_dist_mb[lo:hi]))
            h.set_params(0.2, 0.3, 0.15)
            h.init_emission()
    return hs


@pytest.fixture(scope="module")
def not_a_chain(pkg):
    """hmm.Chain's view of two loaded handles that nghmm_chain_setup has never seen."""
    import ctypes as C
    hs = _handles(pkg, load=True)
    ch = pkg.Chain.__new__(pkg.Chain)
    ch.handles, ch.lib = hs, hs[0].lib
    ch._arr = (C.c_void_p * len(hs))(*[h._h for h in hs])
    ch.n_ind, ch.n_sites = I, CUTS[-1]
    yield ch
    for h in hs:
        h.close()


@pytest.fixture(scope="module")
def empty_chain(pkg):
    """A chain of two handles into which nothing has been loaded."""
    hs = _handles(pkg, load=False)
    yield pkg.Chain(hs)
    for h in hs:
        h.close()


@pytest.mark.parametrize("name,call", ENTRY_POINTS, ids=[n for n, _ in ENTRY_POINTS])
def test_handles_that_are_no_chain(pkg, not_a_chain, name, call):
    with pytest.raises(pkg.NgsFHMMError) as ei:
        call(not_a_chain)
    print(f"\n  {ei.value.code}: {ei.value.message}")
    assert ei.value.code != 0
    assert f"nghmm_chain_{name}" in ei.value.message
    assert "call nghmm_chain_setup on these handles first" in ei.value.message


@pytest.mark.parametrize("name,call", ENTRY_POINTS, ids=[n for n, _ in ENTRY_POINTS])
def test_chain_that_holds_no_data(pkg, empty_chain, name, call):
    with pytest.raises(pkg.NgsFHMMError) as ei:
        call(empty_chain)
    print(f"\n  {ei.value.code}: {ei.value.message}")
    assert ei.value.code != 0
    assert f"nghmm_chain_{name}" in ei.value.message
    assert "holds no data" in ei.value.message
