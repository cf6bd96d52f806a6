"""What a handle takes from the device comes back when it is destroyed: the same cycle of
create / load / EM / decode / every output / replica / destroy, repeated in one process, leaves the
free device memory where it was.  (nghmm_destroy releases buffers that exist only after the
calls that need them -- tracts, sampled paths, observed information, the lanes, the scratch of
every output entry point -- so the cycle makes every one of them, on the parent and on its
replica.)"""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

I, S = 16, 2000
CYCLES = 20


def _outputs(pkg, h, d):
    """One small call per output entry point, on a handle that has iterated: every buffer a handle
    allocates on first use (one region, one threshold; the site records and the per-cell outputs
    are asked for, since they have owners of their own)."""
    I, S = d.n_ind, d.n_sites
    whole = np.array([[0, S]], dtype=np.int64)
    tracts = h.ibd_tracts("viterbi")
    h.ibd_tracts("posterior", 0.5, min_sites=3)
    assert len(h.format_posteriors()) == I * 9 * S
    assert h.geno_posteriors().shape == (S, I, 3)
    stats, paths = h.sample_paths(3, seed=5, keep=2)
    assert stats.shape == (3, I) and paths.shape == (2, I, S)
    assert len(h.obs_info()) == I
    assert len(h.tract_support(tracts)) == len(tracts)
    assert len(h.tract_bounds(tracts)[0]) == len(tracts)
    assert h.freq_info((0.5,), cavity=True)[2].shape == (I, S)
    assert set(h.geno_smooth(whole, sites=True, post=True, call=True)) == {"regions", "sites", "post", "call"}
    assert h.ibd_summary(whole)[1].shape == (S,)
    assert h.ibd_expect(whole, sites=True, viterbi=True)[1].shape == (S,)
    assert h.ibd_moments(whole).shape == (I, 1)
    assert h.ibd_by_length(8, regions=whole).shape == (I, 1, 1)
    assert h.ibd_longest(8, regions=whole).shape == (I, 1, 1)
    assert set(h.ibd_sharing()) == {"vit_both", "post_both", "post_prod"}


def _cycle(pkg, d, gl, mode):
    I, S = d.n_ind, d.n_sites
    h = pkg.NgsFHMM(I, S, mode=mode)
    if mode & pkg.GENO_PACKED:
        cuts = [0, 700, 701, S]
        h.load_chunks(d.pos_dist_mb, [(lo, d.gl[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])],
                      space=0, call_geno=True)
    else:
        h.load(gl, d.pos_dist_mb)
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    for _ in range(2):
        h.iter_EM()
    h.viterbi()
    _outputs(pkg, h, d)
    r = h.replica()
    r.set_params(0.2, 0.3, 0.1)
    r.init_emission()
    r.iter_EM()
    r.viterbi()
    _outputs(pkg, r, d)
    r.close()
    h.close()
    assert h.closed and r.closed


@pytest.mark.parametrize("mode_name", ["fast", "exact_packed"])
def test_destroy_gives_the_device_memory_back(pkg, mode_name):
    """With every output made on the replica too, this test found exact mode's sample_paths holding
    on to device memory: the kept paths left the device by a strided copy to pageable memory, and
    when a second handle of the process (a replica, or an independent one) had made that call too,
    the free memory after a cycle stepped down by 2 MiB in cycles 2, 4, 5, 6 and 7 and stayed there
    (30 cycles; with keep = 0, or with any other output, not at all).  One handle in exact mode now
    copies the rows in one piece (capi_sample.hip)."""
    mode = pkg.MODE_FAST if mode_name == "fast" else pkg.MODE_EXACT | pkg.GENO_PACKED
    d = pkg.simulate.simulate(I, S, seed=31, n_chrom=2, missing_rate=0.05)
    gl = pkg.simulate.normalise_log_gl(d.gl)
    free = {}
    for c in range(1, CYCLES + 1):
        _cycle(pkg, d, gl, mode)
        if c in (2, CYCLES):     # (cycle 1 is left out: the runtime sets up its own pools once)
            torch.cuda.synchronize()
            free[c] = torch.cuda.mem_get_info()[0]
    print(f"{mode_name}: free device memory after cycle 2 {free[2]} B, after cycle {CYCLES} {free[CYCLES]} B")
    assert free[CYCLES] == free[2]
