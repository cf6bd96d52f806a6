#!/usr/bin/env python3
"""Exact path expectations at size (fast-mode handle after one EM iteration and a Viterbi decode):
nghmm_ibd_expect with regions only (one per 10,000 sites), with the site records, and with the
Viterbi term -- next to nghmm_estep on the same handle and session (its backward sweep is the pass
of the same shape) and next to nghmm_sample_paths with 100 draws, which is what the exact call
replaces for the means.

   python tools/expect_timing.py [n_ind n_sites]            wall times of the calls (each ends in
        a device synchronise: the records are copied to the host)
   python tools/expect_timing.py --trace [n_ind n_sites]    the same run as a child under
        rocprofv3 --kernel-trace, then the kernels' own times out of the trace: k_expect_walk,
        k_expect_finish, k_expect_sites, the E-step's backward sweep, the sampler's walks"""
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

KERNELS = ("k_expect_walk", "k_expect_finish", "k_expect_sites", "k_support_bounds", "k_sample_bounds",
           "k_fast_chunk_ops", "k_fast_bwd", "k_sample_walk")


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

gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5)
torch.cuda.synchronize()
with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
    h.load_device(gl.data_ptr(), pos.data_ptr())
    del gl
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    h.iter_EM()
    h.viterbi()
    regions = pkg.window_regions(pos.cpu().numpy(), 10_000)

    def timed(f, n=5):
        f()                                   # (warm-up: scratch allocation, code objects)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, sorted(ts)[n // 2] * 1e3

    def estep():
        h.estep()
        h.synchronize()

    cases = [
        ("ibd_expect, %d regions, no sites" % len(regions), lambda: h.ibd_expect(regions, sites=False)),
        ("ibd_expect, regions, Viterbi term, no sites", lambda: h.ibd_expect(regions, sites=False, viterbi=True)),
        ("ibd_expect, regions + sites", lambda: h.ibd_expect(regions)),
        ("ibd_expect, regions + sites, Viterbi term", lambda: h.ibd_expect(regions, viterbi=True)),
        ("estep (forward walk, bounds, backward sweep)", estep),
        ("sample_paths, 100 draws, statistics only", lambda: h.sample_paths(100, seed=1)),
    ]
    for name, f in cases:
        best, med = timed(f)
        print("%-48s %d x %d: best of 5 %.3f ms (median %.3f)" % (name, I, S, best, med), flush=True)
    layout = h.layout()
    print("per-cell scratch of the site records: %.2f GB; the site records' copy to the host: %.1f MB"
          % (layout[0] * 64 * layout[1] * I * 32 / 1e9, S * 32 / 1e6))
    a, b = h.ibd_expect(regions, viterbi=True), h.ibd_expect(regions, viterbi=True)
    print("two calls bitwise equal:", a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes())
