#!/usr/bin/env python3
"""The distribution of the longest IBD tract at size (fast-mode handle after one EM iteration):
nghmm_ibd_longest with one threshold (1 Mb) and with five (1, 2, 4, 8, 16 Mb), one region over all
sites -- next to nghmm_freq_info without levels (the same kind of walk: one lane per individual and
chromosome) and nghmm_ibd_by_length with the same five thresholds on the same handle and session.
With 20 chromosomes and with one: the walks have individuals x chromosomes lanes.  The five
thresholds also with the K thresholds forced to be a loop inside a lane and forced to be lanes of
their own (NGHMM_LONGEST_SPLIT=0 / 1; the call chooses by longest_split_lanes, kernels_longest.hpp).

   python tools/longest_timing.py [n_ind n_sites]     wall times of the calls, best of 5 (each ends
        in a device synchronise: the records are copied to the host)

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
        def forced(split):
            def f():
                os.environ["NGHMM_LONGEST_SPLIT"] = split
                try:
                    return h.ibd_longest(MB, "mb")
                finally:
                    del os.environ["NGHMM_LONGEST_SPLIT"]
            return f

        cases = [
            ("ibd_longest, 1 x Mb", lambda: h.ibd_longest(1, "mb")),
            ("ibd_longest, 5 x Mb", lambda: h.ibd_longest(MB, "mb")),
            ("  ... thresholds as a loop", forced("0")),
            ("  ... thresholds as lanes", forced("1")),
            ("freq_info, no levels", lambda: h.freq_info()),
            ("ibd_by_length, 5 x Mb", lambda: h.ibd_by_length(MB, "mb")),
        ]
        for name, f in cases:
            try:
                best, med = timed(f)
                print("%d chromosome(s) %-28s %d x %d: best of 5 %.3f ms (median %.3f)" %
                      (n_chrom, name, I, S, best, med), flush=True)
            except pkg.NgsFHMMError as e:
                print("%d chromosome(s) %-28s %d x %d: %s" % (n_chrom, name, I, S, e), flush=True)
        try:
            a, b = h.ibd_longest(MB, "mb"), h.ibd_longest(MB, "mb")
            print("two calls bitwise equal:", a.tobytes() == b.tobytes())
            print("P(a run >= 1, 2, 4, 8, 16 Mb) (cohort mean):", a["p_any"][:, 0].mean(axis=0))
            print("largest |p_any + p_none - 1|: %.2e" % abs(a["p_any"] + a["p_none"] - 1).max())
        except pkg.NgsFHMMError as e:
            print("ibd_longest:", e)
    del pos
    torch.cuda.empty_cache()
