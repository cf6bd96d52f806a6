#!/usr/bin/env python3
"""Tract support at size (fast-mode handle after one EM iteration and a Viterbi decode): wall
time of nghmm_tract_support on the Viterbi tracts of the decode, next to the E-step's backward
sweep of the same run (k_fast_bounds + k_fast_bwd_recompute8, timed by the handle's events in a
fused iteration with the switch `spans`).  Both read the same 12 B per cell -- the emission
ratio, a share of the distances and of the checkpoints -- and the sweep writes 8 B more; the
support walk skips the waves none of whose 64 lane-chunks holds a site of a range, and stops a wave
below its lowest range.  The call also includes what the sweep's time does not: the forward half
(k_fast_chunk_ops + k_sample_bounds), the upload of the records and the download of the scores.
   python tools/support_timing.py [n_ind n_sites]"""
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
    sweep_ms, sweep_n = h.kernel_ms("backward")
    h.set_switch("spans", 0)
    h.estep()
    estep_ms, _ = h.kernel_ms("forward")
    h.viterbi()
    tr = h.ibd_tracts("viterbi")
    n = len(tr)
    raw = np.zeros(n, dtype=pkg.hmm._TRACT_RAW_DTYPE)
    for f in ("ind", "first_site", "n_sites"):
        raw[f] = tr[f]
    out = np.zeros(n, dtype=np.dtype([("a", np.float64), ("b", np.float64), ("c", np.float64), ("d", np.uint64)]))
    ts = []
    for k in range(5):
        t0 = time.perf_counter()
        h._check(h.lib.nghmm_tract_support(h.handle, C.c_void_p(raw.ctypes.data), n, C.c_void_p(out.ctypes.data)))
        ts.append(time.perf_counter() - t0)
    first = out.copy()
    h._check(h.lib.nghmm_tract_support(h.handle, C.c_void_p(raw.ctypes.data), n, C.c_void_p(out.ctypes.data)))
    cells = I * S
    covered = int(tr["n_sites"].sum())
    print("%d x %d, layout (C, T) = %s: %d Viterbi tracts over %d cells (%.1f %% of all)" %
          (I, S, h.layout(), n, covered, 100.0 * covered / cells), flush=True)
    print("nghmm_tract_support: best of 5 %.3f ms (median %.3f, first %.3f)" %
          (min(ts) * 1e3, sorted(ts)[2] * 1e3, ts[0] * 1e3), flush=True)
    print("E-step backward sweep of the fused iteration (k_fast_bounds + k_fast_bwd_recompute8): "
          "%.3f ms in %d launches; stand-alone E-step (forward walk, bounds, sweep): %.3f ms" %
          (sweep_ms, sweep_n, estep_ms), flush=True)
    print("12 B per cell = %.2f GB: floor at 6 TB/s %.3f ms" % (cells * 12 / 1e9, cells * 12 / 6e12 * 1e3))
    print("two calls bitwise equal:", first.tobytes() == out.tobytes(), flush=True)
