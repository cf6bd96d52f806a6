#!/usr/bin/env python3
"""Tract bounds at size (fast-mode handle after one EM iteration and a Viterbi decode): wall time
of nghmm_tract_bounds on the Viterbi tracts of the decode with auto anchors and three levels, next
to nghmm_tract_support on the same tracts, which reads the same cells once.  The bounds call walks
three times -- the cores for the anchors, then twice the stretches between consecutive anchors,
which cover every site of a chromosome that holds a tract -- and moves its pieces through the host
between the walks; both calls include the forward half and the boundary vectors.
   python tools/bounds_timing.py [n_ind n_sites]"""
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
    h.iter_EM()
    h.viterbi()
    tr = h.ibd_tracts("viterbi")
    n = len(tr)
    raw = np.zeros(n, dtype=pkg.hmm._TRACT_RAW_DTYPE)
    for f in ("ind", "first_site", "n_sites"):
        raw[f] = tr[f]
    vp = lambda a: C.c_void_p(a.ctypes.data)
    score = np.zeros(n, dtype=np.dtype([("a", np.float64), ("b", np.float64), ("c", np.float64), ("d", np.uint64)]))
    bound = np.zeros(n, dtype=np.dtype([(f, pkg.TRACT_BOUND_DTYPE[f]) for f in pkg.TRACT_BOUND_DTYPE.names[:6]]))
    levels = np.array([0.975, 0.5, 0.025])
    start, end = np.zeros((n, 3), dtype=np.uint64), np.zeros((n, 3), dtype=np.uint64)
    support = lambda: h._check(h.lib.nghmm_tract_support(h.handle, vp(raw), n, vp(score)))
    bounds = lambda: h._check(h.lib.nghmm_tract_bounds(h.handle, vp(raw), n, None, pkg.hmm._dp(levels), 3, vp(bound),
                                                       vp(start), vp(end)))
    ts = {"nghmm_tract_support": [], "nghmm_tract_bounds": []}
    for name, call in (("nghmm_tract_support", support), ("nghmm_tract_bounds", bounds)):
        for k in range(5):
            t0 = time.perf_counter()
            call()
            ts[name].append(time.perf_counter() - t0)
    first = (bound.copy(), start.copy(), end.copy())
    bounds()
    covered = int(tr["n_sites"].sum())
    print("%d x %d, layout (C, T) = %s: %d Viterbi tracts over %d cells (%.1f %% of all)" %
          (I, S, h.layout(), n, covered, 100.0 * covered / (I * S)), flush=True)
    for name, t in ts.items():
        print("%s: best of 5 %.3f ms (median %.3f, first %.3f)" %
              (name, min(t) * 1e3, sorted(t)[2] * 1e3, t[0] * 1e3), flush=True)
    width = (end[:, 2] - end[:, 0]).astype(np.float64)
    print("95 %% interval of the end: median width %.0f sites, 90th percentile %.0f; reach_right >= 0.5 "
          "towards a neighbour: %d tracts" %
          (np.median(width), np.percentile(width, 90),
           int(((bound["log_reach_right"] >= np.log(0.5)) & (bound["right_limit"] < S - 1)).sum())), flush=True)
    print("two calls bitwise equal:", all(a.tobytes() == b.tobytes() for a, b in zip(first, (bound, start, end))),
          flush=True)
