#!/usr/bin/env python3
"""Exact posterior moments at size (fast-mode handle after one EM iteration): nghmm_ibd_moments
with one region, with the chromosomes and with 1000 windows, both lengths -- next to
nghmm_obs_info on the same handle and session (the same read of 8 B per cell and the same jet
algebra), to nghmm_ibd_expect without site records (the means alone) and to nghmm_sample_paths with
100 draws, which is what the exact call replaces for the second moments.

   python tools/moments_timing.py [n_ind n_sites]            wall times of the calls (each ends in
        a device synchronise: the records are copied to the host)
   python tools/moments_timing.py --trace [n_ind n_sites]    the same run as a child under
        rocprofv3 --kernel-trace, then the kernels' own times out of the trace: k_moments_walk,
        k_moments_segments, k_moments_close next to k_info_walk, k_info_finish, k_expect_walk and
        the sampler's walks"""
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

KERNELS = ("k_moments_walk", "k_moments_segments", "k_moments_close", "k_info_walk", "k_info_finish",
           "k_expect_walk", "k_fast_chunk_ops", "k_sample_walk")


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
    chroms = pkg.chromosome_regions(pos_h)
    windows = pkg.window_regions(pos_h, max(S // 1000, 1))

    def timed(f, n=5):
        f()                                   # (warm-up: scratch allocation, code objects)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, sorted(ts)[n // 2] * 1e3

    cases = [
        ("ibd_moments, 1 region, sites", lambda: h.ibd_moments(None)),
        ("ibd_moments, 1 region, mb", lambda: h.ibd_moments(None, length="mb")),
        ("ibd_moments, %d chromosomes, sites" % len(chroms), lambda: h.ibd_moments(chroms)),
        ("ibd_moments, %d windows, sites" % len(windows), lambda: h.ibd_moments(windows)),
        ("ibd_moments, %d windows, mb" % len(windows), lambda: h.ibd_moments(windows, length="mb")),
        ("obs_info", lambda: h.obs_info()),
        ("ibd_expect, %d windows, no sites" % len(windows), lambda: h.ibd_expect(windows, sites=False)),
        ("sample_paths, 100 draws, statistics only", lambda: h.sample_paths(100, seed=1)),
    ]
    for name, f in cases:
        best, med = timed(f)
        print("%-44s %d x %d: best of 5 %.3f ms (median %.3f)" % (name, I, S, best, med), flush=True)
    C_, T_ = h.layout()[0], h.layout()[1]
    print("layout: C = %d waves, T = %d sites per lane" % (C_, T_))
    a, b = h.ibd_moments(windows), h.ibd_moments(windows)
    print("two calls bitwise equal:", a.tobytes() == b.tobytes())
