#!/usr/bin/env python3
"""Mean and variance of IBD in long tracts at size (fast-mode handle after one EM iteration):
nghmm_ibd_long_moments with one threshold (1 Mb) and with five (1, 2, 4, 8, 16 Mb), one region over
all sites -- next to nghmm_ibd_count with n_counts = 8 and the same thresholds on the same handle
and session.  With 20 chromosomes and with one: the walks have individuals x chromosomes x
thresholds lanes.  The supposition to be checked: the call costs what ibd_count costs with
n_counts = 8 (18 state doubles and a ring entry of 9 against 24 and 9).

   python tools/long_moments_timing.py [n_ind n_sites]     wall times of the calls, best of 5 (each
        ends in a device synchronise: the records are copied to the host)

A call that the device has no memory for (the rings of a long threshold on one chromosome) is
reported as such and the run goes on."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000

pkg = importlib.import_module("ngsf-hmm_amd")
import torch

MB = (1, 2, 4, 8, 16)


def timed(f, n=5):
    f()                                   # (warm-up: scratch allocation, code objects)
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, sorted(ts)[n // 2] * 1e3


for n_chrom in (20, 1):
    gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5, n_chrom=n_chrom)
    torch.cuda.synchronize()
    with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
        h.load_device(gl.data_ptr(), pos.data_ptr())
        del gl
        torch.cuda.empty_cache()
        h.set_params(0.1, 0.2, 0.1)
        h.init_emission()
        h.iter_EM()
        cases = []
        for tag, L in (("1 x Mb", 1), ("5 x Mb", MB)):
            cases.append((f"ibd_count, {tag}, M = 8", lambda L=L: h.ibd_count(L, "mb", max_count=8)))
            cases.append((f"ibd_long_moments, {tag}", lambda L=L: h.ibd_long_moments(L, "mb")))
        for name, f in cases:
            try:
                best, med = timed(f)
                print("%d chromosome(s) %-28s %d x %d: best of 5 %.3f ms (median %.3f)" %
                      (n_chrom, name, I, S, best, med), flush=True)
            except pkg.NgsFHMMError as e:
                print("%d chromosome(s) %-28s %d x %d: %s" % (n_chrom, name, I, S, e), flush=True)
        try:
            a, b = h.ibd_long_moments(MB, "mb"), h.ibd_long_moments(MB, "mb")
            print("two calls bitwise equal:", a.tobytes() == b.tobytes())
            sd = pkg.long_moment_sd(a[:, 0], total=float(pos[torch.isfinite(pos)].sum()))
            print("share of the genome in runs >= 1, 2, 4, 8, 16 Mb (cohort mean):", sd["share"].mean(axis=0))
            print("its posterior sd (cohort mean):", sd["share_sd"].mean(axis=0))
            print("number of such runs (cohort mean):", a["mean_t"][:, 0].mean(axis=0), "sd", sd["sd_t"].mean(axis=0))
        except pkg.NgsFHMMError as e:
            print("ibd_long_moments:", e)
    del pos
    torch.cuda.empty_cache()
