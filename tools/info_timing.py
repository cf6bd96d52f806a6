#!/usr/bin/env python3
"""Observed information at size (fast-mode handle after EM iterations): wall time of
nghmm_obs_info at the current parameters, next to the yardsticks taken in the same process -- one
objective round of five finite-difference points per individual through nghmm_lkl_batch (what a
finite-difference gradient costs today) and the stand-alone E-step's forward walk -- and to the
one-read floor of 8 B per cell (emission ratio; the distances are shared by the individuals) at
the copy rate a device-to-device copy of the same number of bytes reaches here.
   python tools/info_timing.py [n_ind n_sites [iterations]]"""
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
dev = torch.device("cuda", 0)
gl, pos = pkg.simulate.simulate_torch(I, S, dev, seed=5)
torch.cuda.synchronize()


def best(fn, n=5):
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
    print("%d x %d after %d iterations, layout (C, T) = %s" % (I, S, ITERS, h.layout()), flush=True)
    out = np.zeros(I, dtype=pkg.INFO_DTYPE)
    po = C.c_void_p(out.ctypes.data)
    h.obs_info()
    ms_info = best(lambda: h._check(h.lib.nghmm_obs_info(h.handle, None, None, po)))
    print("nghmm_obs_info: %.2f ms" % ms_info, flush=True)
    F0, A0 = h.indF, h.alpha
    eh = 4e-6
    ind = np.repeat(np.arange(I), 5).astype(np.uint32)
    F = (np.repeat(F0, 5).reshape(I, 5) + np.array([0, eh, -eh, 0, 0])).reshape(-1)
    A = (np.repeat(A0, 5).reshape(I, 5) + np.array([0, 0, 0, eh, -eh])).reshape(-1)
    h.lkl(ind, F, A)
    ms_round = best(lambda: h.lkl(ind, F, A))
    print("one five-point objective round (nghmm_lkl_batch): %.2f ms; kernels %.2f ms" %
          (ms_round, h.kernel_ms("lkl_batch")[0]), flush=True)
    ms_estep = best(h.estep, 3)
    print("nghmm_estep: %.2f ms; forward-walk kernels %.2f ms" % (ms_estep, h.kernel_ms("forward")[0]),
          flush=True)
    n = I * S
    a = torch.empty(n, dtype=torch.float64, device=dev)
    b = torch.empty(n, dtype=torch.float64, device=dev)

    def copy():
        b.copy_(a)
        torch.cuda.synchronize()

    copy()
    ms_copy = best(copy)
    rate = 2 * 8 * n / (ms_copy * 1e-3) / 1e12   # bytes read + written
    floor = 8 * n / (rate * 1e12) * 1e3
    print("copy of %d doubles: %.2f ms = %.2f TB/s (read + write); one read of 8 B per cell at that "
          "rate: %.2f ms; nghmm_obs_info / floor = %.1f" % (n, ms_copy, rate, floor, ms_info / floor),
          flush=True)
    se = pkg.std_errors(out, F0, A0)
    print("individual 0: indF %.6f +- %.6f, alpha %.6f +- %.6f, corr %.3f, gradient (%.3g, %.3g)" %
          (F0[0], se[0][0], A0[0], se[1][0], se[2][0], out["g_F"][0], out["g_A"][0]), flush=True)
