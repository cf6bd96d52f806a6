#!/usr/bin/env python3
"""IBD tracts at size (fast-mode handle after one EM iteration and a Viterbi decode): wall time
of nghmm_ibd_tracts with cap = 0 (count, scan, emit, finish; the records stay on the device), for
both sources, next to the bytes each pass streams.  The first call of a source after the E-step
includes the site-major copy of the tile-major posteriors (ensure_marg), reported apart.
   python tools/tracts_timing.py [n_ind n_sites]"""
import ctypes as C
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("ngsf-hmm_amd")
import torch
I = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
gl, pos = pkg.simulate.simulate_torch(I, S, torch.device("cuda", 0), seed=5)
torch.cuda.synchronize()


def call(h, src, thr, m=1):
    n = C.c_uint64(0)
    t0 = time.perf_counter()
    h._check(h.lib.nghmm_ibd_tracts(h.handle, src, thr, m, None, 0, C.byref(n)))
    return time.perf_counter() - t0, n.value


with pkg.NgsFHMM(I, S, mode=pkg.MODE_FAST) as h:
    h.load_device(gl.data_ptr(), pos.data_ptr())
    del gl
    h.set_params(0.1, 0.2, 0.1)
    h.init_emission()
    h.iter_EM()
    h.viterbi()
    cells = I * S
    floors = {"viterbi": cells * 1, "posterior": cells * 8}   # bytes of the in-state source
    first, n = call(h, pkg.TRACTS_VITERBI, 0.5)
    print("first call (site-major posterior copy included): %.3f ms, %d tracts" % (first * 1e3, n),
          flush=True)
    for name, src, thr in (("viterbi", pkg.TRACTS_VITERBI, 0.5),
                           ("posterior", pkg.TRACTS_POSTERIOR, 0.5)):
        ts = []
        for k in range(5):
            dt, n = call(h, src, thr)
            ts.append(dt)
        best = min(ts)
        print("%s: %d x %d, %d tracts, best of 5 %.3f ms (median %.3f); source %.2f GB, "
              "floor at 6 TB/s %.3f ms (one pass)" %
              (name, I, S, n, best * 1e3, sorted(ts)[2] * 1e3, floors[name] / 1e9,
               floors[name] / 6e12 * 1e3), flush=True)
    dt, n = call(h, pkg.TRACTS_POSTERIOR, 0.5, 50)
    print("posterior, min_sites 50 (compaction): %.3f ms, %d tracts" % (dt * 1e3, n), flush=True)
    a = h.ibd_tracts("viterbi")
    b = h.ibd_tracts("viterbi")
    print("two fetches bitwise equal:", a.tobytes() == b.tobytes(), "records", len(a), flush=True)
