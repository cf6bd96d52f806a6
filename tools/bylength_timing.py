#!/usr/bin/env python3
"""Expected IBD above a minimum tract length at size (fast-mode handle after one EM iteration):
nghmm_ibd_by_length with the thresholds 1, 2, 4, 8, 16 Mb and 100 regions -- next to
nghmm_ibd_expect with site records on the same handle and session (the same walk, 32 B per cell
stored and a second pass over them) and to nghmm_estep.  Also in sites, with one region, and with
one threshold; and the largest |Q| the call met (include/nghmm.h: the accuracy of W).

   python tools/bylength_timing.py [n_ind n_sites]           wall times of the calls, best of 5
        (each ends in a device synchronise: the records are copied to the host)
   python tools/bylength_timing.py --trace [n_ind n_sites]   the same run as a child under
        rocprofv3 --kernel-trace, then the kernels' own times out of the trace: k_bylength_walk,
        k_bylength_scan, k_bylength_fill, k_bylength_terms, k_bylength_finish next to k_expect_walk
        and k_expect_sites"""
import csv
import glob
import importlib
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if a != "--trace"]
I = int(args[0]) if len(args) > 0 else 1000
S = int(args[1]) if len(args) > 1 else 1_000_000

KERNELS = ("k_bylength_walk", "k_bylength_scan", "k_bylength_fill", "k_bylength_terms", "k_bylength_finish",
           "k_expect_walk", "k_expect_sites", "k_expect_finish")


def from_trace(path):
    out = {}
    for r in csv.DictReader(open(path)):
        key = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if key:
            out.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


if "--trace" in sys.argv[1:]:
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--",
                        sys.executable, os.path.abspath(__file__), str(I), str(S)], check=True)
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            sys.exit("no kernel trace was written")
        t = from_trace(traces[0])
    for k in sorted(t):
        v = sorted(t[k])
        print("%-20s %3d launches, best %.1f us, median %.1f us" % (k, len(v), v[0], v[len(v) // 2]))
    sys.exit(0)

pkg = importlib.import_module("ngsf-hmm_amd")
import torch

gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5, n_chrom=20)
torch.cuda.synchronize()
with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
    h.load_device(gl.data_ptr(), pos.data_ptr())
    del gl
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    h.iter_EM()
    pos_h = pos.cpu().numpy()
    windows = pkg.window_regions(pos_h, max(S // 100, 1))
    MB = (1, 2, 4, 8, 16)

    def timed(f, n=5):
        f()                                   # (warm-up: scratch allocation, code objects)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, sorted(ts)[n // 2] * 1e3

    cases = [
        ("ibd_by_length, 5 x Mb, %d regions" % len(windows), lambda: h.ibd_by_length(MB, "mb", windows)),
        ("ibd_by_length, 5 x Mb, 1 region", lambda: h.ibd_by_length(MB, "mb")),
        ("ibd_by_length, 1 x Mb, %d regions" % len(windows), lambda: h.ibd_by_length(1, "mb", windows)),
        ("ibd_by_length, 5 x sites, %d regions" % len(windows),
         lambda: h.ibd_by_length((1, 10, 100, 1000, 10000), "sites", windows)),
        ("ibd_expect, %d regions, site records" % len(windows), lambda: h.ibd_expect(windows, sites=True)),
        ("ibd_expect, %d regions, no sites" % len(windows), lambda: h.ibd_expect(windows, sites=False)),
        ("estep", lambda: h.estep()),
    ]
    for name, f in cases:
        best, med = timed(f)
        print("%-44s %d x %d: best of 5 %.3f ms (median %.3f)" % (name, I, S, best, med), flush=True)
    C_, T_ = h.layout()[0], h.layout()[1]
    print("layout: C = %d waves, T = %d sites per lane" % (C_, T_))
    a, b = h.ibd_by_length(MB, "mb", windows), h.ibd_by_length(MB, "mb", windows)
    print("two calls bitwise equal:", a.tobytes() == b.tobytes())
    print("largest |Q| met: %.1f (absolute error of the exponent of W: %.1e)" %
          (h.by_length_qmax(), h.by_length_qmax() * 2.0 ** -53))
    print("tracts per individual >= 1, 2, 4, 8, 16 Mb (cohort mean):", a["tracts"].sum(axis=1).mean(axis=0))
