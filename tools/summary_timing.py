#!/usr/bin/env python3
"""Region and site summaries at size (fast-mode handle after one EM iteration and a Viterbi
decode): nghmm_ibd_summary -- both sources, one region per 10,000 sites, site records -- next to
k_tract_count<POSTERIOR> of the same handle and session, the existing one-pass read of the same
posteriors.  The call should be near that kernel plus the read of the path (1 B per cell).

   python tools/summary_timing.py [n_ind n_sites]            wall times of the calls
   python tools/summary_timing.py --trace [n_ind n_sites]    the same run as a child under
        rocprofv3 --kernel-trace, then the kernels' own times out of the trace: k_summary_pass,
        the finish kernels, k_tract_count<POSTERIOR>, and the ratio of the first to the last"""
import csv
import glob
import importlib
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if a != "--trace"]
I = int(args[0]) if len(args) > 0 else 1000
S = int(args[1]) if len(args) > 1 else 1_000_000


def from_trace(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r["Kernel_Name"]
        m = re.search(r"k_tract_count<(\d)>", name)
        if m:   # (TRACTS_SRC_POSTERIOR = 1)
            key = "k_tract_count<POSTERIOR>" if m.group(1) == "1" else "k_tract_count<VITERBI>"
        else:
            key = next((k for k in ("k_summary_pass", "k_summary_finish_regions", "k_summary_finish_sites")
                        if k in name), None)
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
        print("%-28s %2d launches, best %.1f us, median %.1f us" % (k, len(v), v[0], v[len(v) // 2]))
    if "k_summary_pass" in t and "k_tract_count<POSTERIOR>" in t:
        a, b = min(t["k_summary_pass"]), min(t["k_tract_count<POSTERIOR>"])
        print("k_summary_pass / k_tract_count<POSTERIOR> = %.1f / %.1f = %.2f" % (a, b, a / b))
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
    t0 = time.perf_counter()
    h.ibd_tracts("posterior", 0.5)          # (also makes the site-major copy of the posteriors)
    print("first tract call (site-major posterior copy included): %.3f ms" % ((time.perf_counter() - t0) * 1e3))

    def timed(f, n=5):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, sorted(ts)[n // 2] * 1e3

    import ctypes as C
    n = C.c_uint64(0)
    cases = [
        ("ibd_summary, both sources, %d regions + sites" % len(regions), lambda: h.ibd_summary(regions)),
        ("ibd_summary, both sources, regions only", lambda: h.ibd_summary(regions, sites=False)),
        ("ibd_summary, both sources, sites only", lambda: h.ibd_summary(None)),
        ("ibd_summary, posterior alone, regions + sites", lambda: h.ibd_summary(regions, what="posterior")),
        ("ibd_summary, viterbi alone, regions + sites", lambda: h.ibd_summary(regions, what="viterbi")),
        ("ibd_tracts posterior, cap 0 (count, scan, emit, finish)",
         lambda: h.lib.nghmm_ibd_tracts(h.handle, pkg.TRACTS_POSTERIOR, 0.5, 1, None, 0, C.byref(n))),
    ]
    for name, f in cases:
        best, med = timed(f)
        print("%-58s %d x %d: best of 5 %.3f ms (median %.3f)" % (name, I, S, best, med), flush=True)
    cells = I * S
    print("one pass over 9 B per cell at 6 TB/s: %.3f ms; the site records' copy to the host: %.1f MB"
          % (cells * 9 / 6e12 * 1e3, S * 16 / 1e6))
    a, b = h.ibd_summary(regions), h.ibd_summary(regions)
    print("two calls bitwise equal:", a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes())
