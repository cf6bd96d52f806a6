#!/usr/bin/env python3
"""The per-site frequency likelihood at size (fast-mode handle after one EM iteration): wall time
of nghmm_freq_info with 0, 1 and 8 levels, next to nghmm_estep on the same handle and next to
est_maf's kernel time in the iteration before (timed by the handle's events with the switch
`spans`).  The call's two walks are plain recursions, one lane per individual and chromosome, so
that a chain of site shards gives the single handle's bits; the E-step's have 64 C lanes per
individual.  The simulated data are ONE chromosome: the call's worst case.  Per cell the walks
read the likelihoods twice (24 B dense) and write and read the two weights (16 B) twice; the site
pass reads 16 + 24 B and takes 3 + n_levels logarithms or divisions' worth of work.
   python tools/freqinfo_timing.py [n_ind n_sites]"""
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
    h.set_switch("spans", 1)
    h.iter_EM()
    estmaf_ms, estmaf_n = h.kernel_ms("est_maf")
    h.set_switch("spans", 0)
    print("%d x %d, layout (C, T) = %s" % (I, S, h.layout()), flush=True)
    ts = []
    for k in range(5):
        t0 = time.perf_counter()
        h.estep()
        ts.append(time.perf_counter() - t0)
    print("nghmm_estep (forward walk, boundary vectors, backward sweep): best of 5 %.3f ms (median %.3f)"
          % (min(ts) * 1e3, sorted(ts)[2] * 1e3), flush=True)
    print("est_maf in the fused iteration before: %.3f ms in %d launches" % (estmaf_ms, estmaf_n), flush=True)
    stats = np.zeros(S, dtype=pkg.FREQ_STAT_DTYPE)
    sp = C.c_void_p(stats.ctypes.data)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    first = None
    for lv in ((), (0.0,), (0.0, 0.01, 0.05, 0.2, 0.5, 0.8, 0.95, 1.0)):
        lv = np.array(lv, dtype=np.float64)
        curve = np.zeros((S, len(lv)))
        ts = []
        for k in range(5):
            t0 = time.perf_counter()
            h._check(h.lib.nghmm_freq_info(h.handle, len(lv), dp(lv) if len(lv) else None, sp,
                                           dp(curve) if len(lv) else None, None))
            ts.append(time.perf_counter() - t0)
        print("nghmm_freq_info, %d levels: best of 5 %.3f ms (median %.3f, first %.3f)"
              % (len(lv), min(ts) * 1e3, sorted(ts)[2] * 1e3, ts[0] * 1e3), flush=True)
        if first is None:
            first = stats.copy()
    cells = I * S
    print("walks 2 x 24 + 3 x 16 B per cell = %.2f GB, site pass 16 + 24 B per cell = %.2f GB: floor at "
          "6 TB/s %.3f ms" % (cells * 96 / 1e9, cells * 40 / 1e9, cells * 136 / 6e12 * 1e3))
    print("the records of the three calls bitwise equal:", first.tobytes() == stats.tobytes(), flush=True)
    se = pkg.freq_std_errors(stats)
    print("score: median |score| %.3g; se: median %.3g over %d sites with info > 0"
          % (np.median(np.abs(stats["score"])), np.nanmedian(se), int(np.isfinite(se).sum())), flush=True)
