"""V site-shard handles of one process on ONE GPU for the site-shard tests: each holds all
individuals for a contiguous site range and runs in a thread of its own; the all-gather the
library asks for is done here (barrier + device copies)."""
import importlib
import threading

import numpy as np


class Chain:
    """V site-shard handles on cuda:0 with a thread-barrier all-gather."""

    def __init__(self, pkg, gl, pos, V, mode=None, raw=None, ranges=None):
        import torch
        dd = importlib.import_module("ngsf-hmm_amd.distributed")
        self.torch = torch
        self.V = V
        S, I = gl.shape[0] if gl is not None else raw.shape[0], (gl if gl is not None else raw).shape[1]
        self.ranges = list(ranges) if ranges is not None else dd.site_ranges_ragged(S, V)
        assert len(self.ranges) == V
        self.barrier = threading.Barrier(V)
        dev = torch.device("cuda", 0)
        self.h, self.send, self.recv = [], [], []
        self.gathers = [0] * V
        for r, (lo, hi) in enumerate(self.ranges):
            h = pkg.NgsFHMM(I, hi - lo, mode=pkg.MODE_FAST if mode is None else mode)
            if raw is not None:
                h.load_raw(np.ascontiguousarray(raw[lo:hi]), np.ascontiguousarray(pos[lo:hi]),
                           space=0, call_geno=True)
            else:
                h.load(np.ascontiguousarray(gl[lo:hi]), np.ascontiguousarray(pos[lo:hi]))
            n = h.site_shard_bytes()
            self.send.append(torch.zeros(n // 8, dtype=torch.float64, device=dev))
            self.recv.append(torch.zeros(V * (n // 8), dtype=torch.float64, device=dev))
            self.h.append(h)
        torch.cuda.synchronize()
        for r, h in enumerate(self.h):
            h.site_shard_setup(r, V, self.send[r].data_ptr(), self.recv[r].data_ptr(),
                               h.site_shard_bytes(), self._gather(r))

    def _gather(self, r):
        def cb(n):
            k = n // 8
            self.h[r].synchronize()            # this handle's stream has written send[r]
            self.barrier.wait()
            for q in range(self.V):
                self.recv[r][q * k:(q + 1) * k].copy_(self.send[q][:k])
            self.torch.cuda.synchronize()
            self.barrier.wait()                # nobody rewrites its send before all have read it
            self.gathers[r] += 1
        return cb

    def each(self, fn):
        """fn(r, handle) on every handle, one thread each; returns the results in rank order."""
        out, err = [None] * self.V, []

        def run(r):
            try:
                out[r] = fn(r, self.h[r])
            except BaseException as e:
                err.append(e)
                self.barrier.abort()
        th = [threading.Thread(target=run, args=(r,)) for r in range(self.V)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if err:
            raise err[0]
        return out

    def set_params(self, F, A, freq):
        for (lo, hi), h in zip(self.ranges, self.h):
            h.set_params(F, A, np.broadcast_to(freq, (self.ranges[-1][1],))[lo:hi])
            h.init_emission()

    def viterbi(self):
        scores = None
        for h in self.h:
            scores = h.viterbi_shard_forward(scores)
        state, parts = None, [None] * self.V
        for r in reversed(range(self.V)):
            state, parts[r] = self.h[r].viterbi_shard_back(state)
        return np.concatenate(parts, axis=1)

    def close(self):
        for h in self.h:
            h.close()
