#!/usr/bin/env python3
"""Pairwise IBD sharing at size (fast-mode handle after one EM iteration and a Viterbi decode):
nghmm_ibd_sharing per source and output, next to two floors:
  * one read of the posteriors, 8 B per cell, at 6 TB/s;
  * I^2 S multiply-adds at the FP64 vector rate tools/fp64_peak.hip measures.  Give the measured
    rate with --fma_rate (multiply-adds per second); the default is the peak that tool reports its
    percentage of, 256 CUs x 4 SIMDs x 2.4 GHz / 4 wave-instructions x 64 lanes = 3.93e13.
    (The kernel computes the blocks on and above the diagonal only, a little more than half.)

   python tools/sharing_timing.py [--fma_rate R] [n_ind n_sites]   default: 1000 x 1,000,000, then
                                                                   100 x 100,000"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
argv = sys.argv[1:]
fma_rate = 256 * 4 * 2.4e9 / 4 * 64
if "--fma_rate" in argv:
    k = argv.index("--fma_rate")
    fma_rate = float(argv[k + 1])
    del argv[k:k + 2]
sizes = [(int(argv[0]), int(argv[1]))] if len(argv) > 1 else [(1000, 1_000_000), (100, 100_000)]

pkg = importlib.import_module("ngsf-hmm_amd")
import torch


def timed(f, n=5):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, sorted(ts)[n // 2] * 1e3


for I, S in sizes:
    gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5)
    torch.cuda.synchronize()
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        h.load_device(gl.data_ptr(), pos.data_ptr())
        del gl
        h.set_params(0.1, 0.2, 0.1)
        h.init_emission()
        h.iter_EM()
        h.viterbi()
        t0 = time.perf_counter()
        h.ibd_sharing()          # (also makes the site-major copy of the posteriors and the scratch)
        print("first call (site-major posterior copy and scratch included): %.3f ms"
              % ((time.perf_counter() - t0) * 1e3))
        first, length, n = pkg.sharing_splits(I, 0, S)
        print("%d K-splits of %d sites, %.1f MB of partial matrices" % (n, length, n * I * I * 8 / 1e6))
        cases = [
            ("ibd_sharing, all three", lambda: h.ibd_sharing()),
            ("ibd_sharing, vit_both (int8 MFMA on the path)", lambda: h.ibd_sharing("vit_both")),
            ("ibd_sharing, post_both (threshold pass + int8 MFMA)", lambda: h.ibd_sharing("post_both")),
            ("ibd_sharing, post_prod (FP64 MFMA)", lambda: h.ibd_sharing("post_prod")),
        ]
        for name, f in cases:
            best, med = timed(f)
            print("%-52s %d x %d: best of 5 %.3f ms (median %.3f)" % (name, I, S, best, med), flush=True)
        print("floors: one read of the posteriors, 8 B per cell at 6 TB/s: %.3f ms; I^2 S = %.3g "
              "multiply-adds at %.3g per second: %.3f ms; the copy to the host: %.1f MB a matrix"
              % (I * S * 8 / 6e12 * 1e3, float(I) * I * S, fma_rate, float(I) * I * S / fma_rate * 1e3,
                 I * I * 8 / 1e6))
        a, b = h.ibd_sharing(), h.ibd_sharing()
        print("two calls bitwise equal:", all(a[k].tobytes() == b[k].tobytes() for k in a))
    del pos
    torch.cuda.empty_cache()
