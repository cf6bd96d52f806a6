#!/usr/bin/env python3
"""The smoothed genotype posteriors at size (fast-mode handle after one EM iteration): wall time
of nghmm_geno_smooth -- the site records alone, with one region per chromosome, with the calls,
with the posteriors -- next to nghmm_freq_info with no levels on the same handle: the same two
walks plus a pass over the same cells.  The simulated data are ONE chromosome: the walks' worst
case.  Per cell the cell pass reads 16 B of weights and 24 B of dense likelihoods and writes up to
24 B of posteriors and 1 B of call; the posteriors and the calls are also copied to the host,
which the wall time includes.
   python tools/genosmooth_timing.py [n_ind n_sites]"""
import ctypes as C
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("ngsf-hmm_amd")
import numpy as np
import torch
I = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5)
torch.cuda.synchronize()

with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
    h.load_device(gl.data_ptr(), pos.data_ptr())
    del gl
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    h.iter_EM()
    print("%d x %d, layout (C, T) = %s" % (I, S, h.layout()), flush=True)

    def best(fn):
        ts = []
        for k in range(5):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return "best of 5 %.3f ms (median %.3f, first %.3f)" % (min(ts) * 1e3, sorted(ts)[2] * 1e3, ts[0] * 1e3)

    stats = np.zeros(S, dtype=pkg.FREQ_STAT_DTYPE)
    sp = C.c_void_p(stats.ctypes.data)
    print("nghmm_freq_info, 0 levels: " +
          best(lambda: h._check(h.lib.nghmm_freq_info(h.handle, 0, None, sp, None, None))), flush=True)
    sites = np.zeros(S, dtype=pkg.GENO_SITE_STAT_DTYPE)
    gp = C.c_void_p(sites.ctypes.data)
    u64p = C.POINTER(C.c_uint64)
    begin, end = np.array([0], dtype=np.uint64), np.array([S], dtype=np.uint64)
    regs = np.zeros((I, 1), dtype=pkg.GENO_REGION_STAT_DTYPE)
    rp = C.c_void_p(regs.ctypes.data)
    call = np.zeros((S, I), dtype=np.uint8)
    cp = call.ctypes.data_as(C.POINTER(C.c_uint8))
    L = h.lib
    print("nghmm_geno_smooth, sites: " +
          best(lambda: h._check(L.nghmm_geno_smooth(h.handle, 0, None, None, None, gp, None, None))), flush=True)
    first = sites.copy()
    print("nghmm_geno_smooth, sites and one region: " +
          best(lambda: h._check(L.nghmm_geno_smooth(h.handle, 1, begin.ctypes.data_as(u64p),
                                                    end.ctypes.data_as(u64p), rp, gp, None, None))), flush=True)
    print("nghmm_geno_smooth, sites and calls: " +
          best(lambda: h._check(L.nghmm_geno_smooth(h.handle, 0, None, None, None, gp, None, cp))), flush=True)
    if I * S * 24 <= 8 << 30:
        post = np.zeros((S, I, 3))
        pp = post.ctypes.data_as(C.POINTER(C.c_double))
        print("nghmm_geno_smooth, sites and posteriors: " +
              best(lambda: h._check(L.nghmm_geno_smooth(h.handle, 0, None, None, None, gp, pp, None))), flush=True)
    else:
        print("nghmm_geno_smooth, posteriors: skipped (%.1f GB on the host)" % (I * S * 24 / 1e9))
    cells = I * S
    print("walks 2 x 24 + 3 x 16 B per cell = %.2f GB, cell pass 16 + 24 B per cell = %.2f GB; the pass also "
          "makes 36 cross-lane exchanges of a double per wave and site.  What it costs is the difference "
          "between the two calls above, not a figure assumed here." % (cells * 96 / 1e9, cells * 40 / 1e9))
    print("the site records of the calls bitwise equal:", first.tobytes() == sites.tobytes(), flush=True)
    em = pkg.geno_em_freq(sites, I)
    print("em_freq - freq: median |.| %.3g; heterozygosity outside IBD: median %.3g"
          % (np.median(np.abs(em - h.freq)), np.median(pkg.het_outside_ibd(regs))), flush=True)
