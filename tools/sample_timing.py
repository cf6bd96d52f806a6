#!/usr/bin/env python3
"""Sampled IBD paths at size (fast-mode handle after EM iterations): wall time of
nghmm_sample_paths for (n_draws, keep) = (1, 1), (1, 0), (16, 0), (64, 0), next to the two
yardsticks taken in the same process: the stand-alone E-step (forward walk + bounds + backward
sweep, nghmm_estep) and nghmm_viterbi.
   python tools/sample_timing.py [n_ind n_sites [iterations]]"""
import ctypes as C
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("ngsf-hmm_amd")
import numpy as np
import torch
I = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5)
torch.cuda.synchronize()


def best(fn, n=3):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
    h.load_device(gl.data_ptr(), pos.data_ptr())
    del gl
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    for _ in range(ITERS):
        h.iter_EM()
    print("%d x %d after %d iterations" % (I, S, ITERS), flush=True)
    print("nghmm_estep (forward walk, bounds, backward sweep): %.2f ms; kernels %.2f ms" %
          (best(h.estep), h.kernel_ms("forward")[0]), flush=True)
    path = np.empty((I, S), dtype=np.uint8)
    pp = path.ctypes.data_as(C.POINTER(C.c_uint8))
    print("nghmm_viterbi: %.1f ms" % best(lambda: h._check(h.lib.nghmm_viterbi(h.handle, pp)), 2),
          flush=True)
    stats = np.zeros((64, I), dtype=pkg.PATH_STATS_DTYPE)
    sp = C.c_void_p(stats.ctypes.data)
    for n_draws, keep in ((1, 1), (1, 0), (16, 0), (64, 0)):
        ms = best(lambda: h._check(h.lib.nghmm_sample_paths(h.handle, 1, n_draws, sp, keep,
                                                           pp if keep else None)))
        print("nghmm_sample_paths(n_draws=%d, keep=%d): %.2f ms  (%.2f ms per draw)" %
              (n_draws, keep, ms, ms / n_draws), flush=True)
    q = pkg.path_stats_summary(stats)
    print("individual 0: tracts %s, IBD sites %s (2.5 %%, median, 97.5 %%)" %
          (q["n_tracts"][:, 0].tolist(), q["ibd_sites"][:, 0].tolist()), flush=True)
