#!/usr/bin/env python3
"""The per-site posterior of lying in a long IBD tract at size (fast-mode handle after one EM
iteration): nghmm_ibd_long with the thresholds 1 Mb alone and 1, 2, 4, 8, 16 Mb and 100 regions --
the region records alone, then with the site records, then with post -- next to
nghmm_ibd_by_length with the same thresholds on the same handle and session (the same walk and
cells; ibd_long adds per threshold the prefix of T_k, the gather at lo_k and the output passes).
post is K x I x S doubles on the host (8 GB per threshold at 1000 x 1 M): it is timed with one
threshold, and with five only with --post5.

   python tools/long_timing.py [--post5] [n_ind n_sites]     wall times of the calls, best of 5
        (each ends in a device synchronise: the records are copied to the host)"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if a != "--post5"]
I = int(args[0]) if len(args) > 0 else 1000
S = int(args[1]) if len(args) > 1 else 1_000_000

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

    R = len(windows)
    cases = []
    for L, tag in ((1, "1 x Mb"), (MB, "5 x Mb")):
        cases += [
            ("ibd_by_length, %s, %d regions" % (tag, R), lambda L=L: h.ibd_by_length(L, "mb", windows)),
            ("ibd_long, %s, %d regions" % (tag, R), lambda L=L: h.ibd_long(L, "mb", windows, sites=False)),
            ("ibd_long, %s, regions + sites" % tag, lambda L=L: h.ibd_long(L, "mb", windows, sites=True)),
        ]
        if L == 1 or "--post5" in sys.argv[1:]:
            cases.append(("ibd_long, %s, regions + sites + post" % tag,
                          lambda L=L: h.ibd_long(L, "mb", windows, sites=True, post=True)))
    cases.append(("ibd_long, 5 x sites, %d regions" % R,
                  lambda: h.ibd_long((1, 10, 100, 1000, 10000), "sites", windows, sites=False)))
    for name, f in cases:
        best, med = timed(f)
        print("%-44s %d x %d: best of 5 %.3f ms (median %.3f)" % (name, I, S, best, med), flush=True)
    C_, T_ = h.layout()[0], h.layout()[1]
    print("layout: C = %d waves, T = %d sites per lane" % (C_, T_))
    a, b = h.ibd_long(MB, "mb", windows), h.ibd_long(MB, "mb", windows)
    print("two calls bitwise equal:", all(a[k].tobytes() == b[k].tobytes() for k in a))
    by = h.ibd_by_length(MB, "mb", pkg.chromosome_regions(pos_h))
    lg = h.ibd_long(MB, "mb", pkg.chromosome_regions(pos_h), sites=False)["regions"]
    print("largest |mb - ibd_by_length's length| over the chromosomes: %.3e (lengths up to %.1f Mb)" %
          (abs(lg["mb"] - by["length"]).max(), by["length"].max()))
    print("sites per individual in tracts >= 1, 2, 4, 8, 16 Mb (cohort mean):",
          a["regions"]["sites"].sum(axis=1).mean(axis=0))
