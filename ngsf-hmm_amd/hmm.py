"""Host-side mirror of the reference's EM interface over the C ABI (include/nghmm.h).

Names follow the reference: ``EM`` (EM.cpp:27-135), ``iter_EM`` (EM.cpp:139-289),
``viterbi`` (shared/HMM.cpp:98-125), ``lkl`` (EM.cpp:449-464), the ``params`` fields
``indF / alpha / freq / marg_prob / ind_lkl / e_prob / path / tot_lkl``
(ngsF-HMM.hpp:13-52).  Errors the reference reports through ``error()`` +
``exit(-1)`` are raised as :class:`NgsFHMMError` carrying the same message.

All arithmetic happens in ``libnghmm.so`` (HIP kernels).  This module never
computes a result itself and has no fallback.
"""
from __future__ import annotations

import ctypes as C
import weakref
import math
import os
import subprocess

import numpy as np

MODE_EXACT = 0
MODE_FAST = 1
GENO_PACKED = 0x10   # OR-ed into the mode: called genotypes kept as 2-bit codes
# OR-ed into freq_est: --freq_est 2 / --e_prob 2 AS INTENDED (opt-in, parity unpinned: the
# reference aborts on both; include/nghmm.h)
LD_INTENDED = 0x20
EPROB_LD = 0x40

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

c_double_p = C.POINTER(C.c_double)
HOOK_FN = C.CFUNCTYPE(None, C.c_void_p)   # nghmm_hook_fn
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)   # nghmm_allgather_fn


class NgsFHMMError(RuntimeError):
    """A fatal condition of the reference (its message) or a runtime failure."""

    def __init__(self, code, message):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


class ModeCount(C.Structure):        # nghmm_mode_count (include/nghmm_debug.h)
    _fields_ = [("mode", C.c_uint32), ("ind_rounds", C.c_uint64)]


class MstepStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("points", C.c_uint64),
                ("ref_forward_calls", C.c_uint64), ("ind_rounds", C.c_uint64)]


def library_path():
    # NGHMM_LIB: another build of the same library (kernel tuning experiments)
    return os.environ.get("NGHMM_LIB") or os.path.join(_HERE, "libnghmm.so")


def build_library(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], check=True, stdout=out)
    return library_path()


def load_library():
    """dlopen libnghmm.so and declare every entry point of include/nghmm.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise NgsFHMMError(-11, f"{path} is missing: build it with "
                                "`python -c 'import __graft_entry__ as g; g.build()'` "
                                "(the hot path has no CPU fallback)")
    L = C.CDLL(path)
    vp, u64, u32, i32, d = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
    dp = c_double_p
    sig = {
        "nghmm_last_error": (C.c_char_p, []),
        "nghmm_strerror": (C.c_char_p, [i32]),
        "nghmm_has_hip": (i32, []),
        "nghmm_create": (i32, [C.POINTER(vp), u64, u64, i32, i32]),
        "nghmm_destroy": (i32, [vp]),
        "nghmm_create_replica": (i32, [C.POINTER(vp), vp]),
        "nghmm_load_gl": (i32, [vp, dp, dp]),
        "nghmm_load_gl_raw": (i32, [vp, dp, i32, i32, i32, dp]),
        "nghmm_get_gl": (i32, [vp, dp]),
        "nghmm_geno_posteriors": (i32, [vp, u64, u64, dp]),
        "nghmm_format_posteriors": (i32, [vp, u64, u64, C.c_char_p]),
        "nghmm_format_fixed6": (i32, [vp, dp, u64, u64, C.c_char_p]),
        "nghmm_load_gl_device": (i32, [vp, vp, vp]),
        "nghmm_load_begin": (i32, [vp, dp]),
        "nghmm_load_begin_dev": (i32, [vp, vp]),
        "nghmm_load_gl_raw_sites": (i32, [vp, u64, u64, dp, i32, i32, i32]),
        "nghmm_load_gl_raw_sites_dev": (i32, [vp, u64, u64, vp, i32, i32, i32]),
        "nghmm_load_geno_sites": (i32, [vp, u64, u64, C.POINTER(C.c_int8)]),
        "nghmm_load_end": (i32, [vp]),
        "nghmm_get_geno_codes_dev": (i32, [vp, u64, u64, vp]),
        "nghmm_load_geno_site_shard_dev": (i32, [vp, vp]),
        "nghmm_set_params": (i32, [vp, dp, dp, dp]),
        "nghmm_get_params": (i32, [vp, dp, dp, dp]),
        "nghmm_emission": (i32, [vp]),
        "nghmm_estep": (i32, [vp, dp]),
        "nghmm_lkl_batch": (i32, [vp, u32, C.POINTER(u32), dp, dp, dp]),
        "nghmm_mstep_indf": (i32, [vp, i32, i32, C.POINTER(MstepStats)]),
        "nghmm_bfgs_batch_host": (i32, [u64, dp, dp, i32, i32, vp, vp, C.POINTER(MstepStats)]),
        "nghmm_bfgs_batch_host2": (i32, [u64, dp, dp, i32, i32, vp, vp, C.POINTER(MstepStats), i32]),
        "nghmm_mstep_freq": (i32, [vp, i32]),
        "nghmm_estep_mstep": (i32, [vp, i32, i32, dp, C.POINTER(MstepStats), HOOK_FN, vp]),
        "nghmm_iter_em": (i32, [vp, i32, i32, i32, dp, C.POINTER(MstepStats)]),
        "nghmm_viterbi": (i32, [vp, C.POINTER(C.c_uint8)]),
        "nghmm_get_posteriors": (i32, [vp, dp]),
        "nghmm_get_emissions": (i32, [vp, dp]),
        "nghmm_shard_config": (i32, [vp, u64, u64, u64, u64]),
        "nghmm_load_gl_site_shard": (i32, [vp, dp]),
        "nghmm_load_gl_site_shard_dev": (i32, [vp, vp]),
        "nghmm_pack_posteriors_dev": (i32, [vp, u64, u64, vp]),
        "nghmm_mstep_freq_sites_dev": (i32, [vp, vp, vp]),
        "nghmm_set_freq_dev": (i32, [vp, vp]),
        "nghmm_group_setup": (i32, [C.POINTER(vp), i32]),
        "nghmm_group_iter_em": (i32, [C.POINTER(vp), i32, i32, i32, i32, dp, C.POINTER(MstepStats)]),
        "nghmm_group_mstep_freq": (i32, [C.POINTER(vp), i32, i32]),
        "nghmm_fast_layout": (i32, [vp, C.POINTER(u32), C.POINTER(u64)]),
        "nghmm_stream": (vp, [vp]),
        "nghmm_synchronize": (i32, [vp]),
        "nghmm_kernel_ms": (i32, [vp, i32, dp, C.POINTER(u32)]),
        "nghmm_set_switch": (i32, [vp, C.c_char_p, C.c_long]),
        "nghmm_debug_mode_counts": (i32, [vp, C.POINTER(ModeCount), u32, C.POINTER(u32), i32]),
        "nghmm_debug_estmaf_counts": (i32, [vp, C.POINTER(u64), i32]),
        "nghmm_alloc_host": (vp, [u64]),
        "nghmm_free_host": (None, [vp]),
        "nghmm_site_shard_bytes": (u64, [vp]),
        "nghmm_site_shard_setup": (i32, [vp, i32, i32, vp, vp, u64, ALLGATHER_FN, vp]),
        "nghmm_chain_setup": (i32, [C.POINTER(vp), i32]),
        "nghmm_chain_iter_em": (i32, [C.POINTER(vp), i32, i32, i32, i32, dp, C.POINTER(MstepStats)]),
        "nghmm_chain_mstep_freq": (i32, [C.POINTER(vp), i32, i32]),
        "nghmm_chain_viterbi": (i32, [C.POINTER(vp), i32, C.POINTER(C.c_uint8)]),
        "nghmm_viterbi_shard_forward": (i32, [vp, dp, dp]),
        "nghmm_viterbi_shard_back": (i32, [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                           C.POINTER(C.c_uint8)]),
        "nghmm_ibd_tracts": (i32, [vp, i32, d, u64, vp, u64, C.POINTER(u64)]),
        "nghmm_chain_ibd_tracts": (i32, [C.POINTER(vp), i32, i32, d, u64, vp, u64, C.POINTER(u64)]),
        "nghmm_sample_paths": (i32, [vp, u64, u32, vp, u32, C.POINTER(C.c_uint8)]),
        "nghmm_chain_sample_paths": (i32, [C.POINTER(vp), i32, u64, u32, vp, u32,
                                           C.POINTER(C.c_uint8)]),
        "nghmm_tract_support": (i32, [vp, vp, u64, vp]),
        "nghmm_chain_tract_support": (i32, [C.POINTER(vp), i32, vp, u64, vp]),
        "nghmm_tract_bounds": (i32, [vp, vp, u64, vp, dp, u32, vp, vp, vp]),
        "nghmm_chain_tract_bounds": (i32, [C.POINTER(vp), i32, vp, u64, vp, dp, u32, vp, vp, vp]),
        "nghmm_freq_info": (i32, [vp, u32, dp, vp, dp, dp]),
        "nghmm_chain_freq_info": (i32, [C.POINTER(vp), i32, u32, dp, vp, dp, dp]),
        "nghmm_geno_smooth": (i32, [vp, u64, C.POINTER(u64), C.POINTER(u64), vp, vp, dp,
                                    C.POINTER(C.c_uint8)]),
        "nghmm_chain_geno_smooth": (i32, [C.POINTER(vp), i32, u64, C.POINTER(u64), C.POINTER(u64), vp,
                                          vp, dp, C.POINTER(C.c_uint8)]),
        "nghmm_obs_info": (i32, [vp, dp, dp, vp]),
        "nghmm_chain_obs_info": (i32, [C.POINTER(vp), i32, dp, dp, vp]),
        "nghmm_ibd_summary": (i32, [vp, i32, d, u64, C.POINTER(u64), C.POINTER(u64), vp, vp]),
        "nghmm_chain_ibd_summary": (i32, [C.POINTER(vp), i32, i32, d, u64, C.POINTER(u64),
                                          C.POINTER(u64), vp, vp]),
        "nghmm_ibd_sharing": (i32, [vp, i32, d, u64, u64, C.POINTER(u64), C.POINTER(u64), dp]),
        "nghmm_chain_ibd_sharing": (i32, [C.POINTER(vp), i32, i32, d, u64, u64, C.POINTER(u64),
                                          C.POINTER(u64), dp]),
        "nghmm_ibd_expect": (i32, [vp, i32, u64, C.POINTER(u64), C.POINTER(u64), vp, vp]),
        "nghmm_chain_ibd_expect": (i32, [C.POINTER(vp), i32, i32, u64, C.POINTER(u64), C.POINTER(u64),
                                         vp, vp]),
        "nghmm_ibd_moments": (i32, [vp, i32, u64, C.POINTER(u64), C.POINTER(u64), vp]),
        "nghmm_chain_ibd_moments": (i32, [C.POINTER(vp), i32, i32, u64, C.POINTER(u64), C.POINTER(u64),
                                          vp]),
        "nghmm_ibd_by_length": (i32, [vp, i32, u32, dp, u64, C.POINTER(u64), C.POINTER(u64), vp]),
        "nghmm_chain_ibd_by_length": (i32, [C.POINTER(vp), i32, i32, u32, dp, u64, C.POINTER(u64),
                                            C.POINTER(u64), vp]),
        "nghmm_debug_bylength_qmax": (i32, [vp, dp]),
        "nghmm_ibd_longest": (i32, [vp, i32, u32, dp, u64, C.POINTER(u64), C.POINTER(u64), vp]),
        "nghmm_chain_ibd_longest": (i32, [C.POINTER(vp), i32, i32, u32, dp, u64, C.POINTER(u64),
                                          C.POINTER(u64), vp]),
        "nghmm_ibd_count": (i32, [vp, i32, u32, dp, u32, u64, C.POINTER(u64), C.POINTER(u64), dp]),
        "nghmm_ibd_long_moments": (i32, [vp, i32, u32, dp, u64, C.POINTER(u64), C.POINTER(u64), vp]),
        "nghmm_ibd_long": (i32, [vp, i32, u32, dp, d, u64, C.POINTER(u64), C.POINTER(u64), vp, vp, dp]),
        "nghmm_chain_ibd_long": (i32, [C.POINTER(vp), i32, i32, u32, dp, d, u64, C.POINTER(u64),
                                       C.POINTER(u64), vp, vp, dp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def _dp(a):
    return a.ctypes.data_as(c_double_p)


EXPORTED_SYMBOLS = [
    "nghmm_last_error", "nghmm_strerror", "nghmm_has_hip", "nghmm_create", "nghmm_destroy",
    "nghmm_create_replica",
    "nghmm_load_gl", "nghmm_load_gl_raw", "nghmm_get_gl", "nghmm_geno_posteriors",
    "nghmm_format_posteriors", "nghmm_format_fixed6",
    "nghmm_load_gl_device", "nghmm_load_begin", "nghmm_load_begin_dev", "nghmm_load_gl_raw_sites",
    "nghmm_load_gl_raw_sites_dev", "nghmm_load_geno_sites", "nghmm_load_end",
    "nghmm_get_geno_codes_dev", "nghmm_load_geno_site_shard_dev",
    "nghmm_set_params", "nghmm_get_params",
    "nghmm_emission", "nghmm_estep", "nghmm_lkl_batch", "nghmm_mstep_indf",
    "nghmm_bfgs_batch_host", "nghmm_bfgs_batch_host2", "nghmm_mstep_freq", "nghmm_estep_mstep",
    "nghmm_iter_em", "nghmm_viterbi", "nghmm_get_posteriors", "nghmm_get_emissions",
    "nghmm_shard_config", "nghmm_load_gl_site_shard", "nghmm_load_gl_site_shard_dev",
    "nghmm_pack_posteriors_dev",
    "nghmm_mstep_freq_sites_dev", "nghmm_set_freq_dev", "nghmm_group_setup", "nghmm_group_iter_em",
    "nghmm_group_mstep_freq",
    "nghmm_fast_layout", "nghmm_stream",
    "nghmm_synchronize",
    "nghmm_kernel_ms", "nghmm_set_switch", "nghmm_debug_mode_counts", "nghmm_debug_estmaf_counts",
    "nghmm_site_shard_bytes", "nghmm_site_shard_setup", "nghmm_viterbi_shard_forward",
    "nghmm_viterbi_shard_back", "nghmm_chain_setup", "nghmm_chain_iter_em", "nghmm_chain_mstep_freq",
    "nghmm_chain_viterbi", "nghmm_alloc_host", "nghmm_free_host",
    "nghmm_ibd_tracts", "nghmm_chain_ibd_tracts",
    "nghmm_sample_paths", "nghmm_chain_sample_paths",
    "nghmm_tract_support", "nghmm_chain_tract_support",
    "nghmm_tract_bounds", "nghmm_chain_tract_bounds",
    "nghmm_freq_info", "nghmm_chain_freq_info",
    "nghmm_geno_smooth", "nghmm_chain_geno_smooth",
    "nghmm_obs_info", "nghmm_chain_obs_info",
    "nghmm_ibd_summary", "nghmm_chain_ibd_summary",
    "nghmm_ibd_sharing", "nghmm_chain_ibd_sharing",
    "nghmm_ibd_expect", "nghmm_chain_ibd_expect",
    "nghmm_ibd_moments", "nghmm_chain_ibd_moments",
    "nghmm_ibd_by_length", "nghmm_chain_ibd_by_length", "nghmm_debug_bylength_qmax",
    "nghmm_ibd_longest", "nghmm_chain_ibd_longest",
    "nghmm_ibd_long",
    "nghmm_ibd_count",
    "nghmm_ibd_long_moments",
]
# (nghmm_chain_ibd_long is declared in include/nghmm_chain_long.h)

OBJECTIVE_FN = C.CFUNCTYPE(C.c_double, C.c_uint32, C.c_double, C.c_double, C.c_void_p)


def bfgs_batch_host(indF, alpha, objective, indF_fixed=False, alpha_fixed=False, det_pow=None,
                    device_solver=False):
    """Lock-step batched L-BFGS-B (the indF/alpha M-step's host half) with a Python
    objective ``objective(ind, F, alpha) -> forward log-likelihood``.  Returns
    (indF, alpha, stats).  det_pow: the finite-difference step by the library's own exp / log
    (fast mode's) instead of libm's pow; device_solver: the solver type k_bfgs_advance runs on
    the GPU, on the host (nghmm_bfgs_batch_host2)."""
    L = load_library()
    F = np.array(indF, dtype=np.float64)
    A = np.array(alpha, dtype=np.float64)
    st = MstepStats()
    cb = OBJECTIVE_FN(lambda i, f, a, _u: float(objective(i, f, a)))
    if det_pow is None and not device_solver:
        rc = L.nghmm_bfgs_batch_host(len(F), _dp(F), _dp(A), int(indF_fixed), int(alpha_fixed),
                                     C.cast(cb, C.c_void_p), None, C.byref(st))
    else:
        rc = L.nghmm_bfgs_batch_host2(len(F), _dp(F), _dp(A), int(indF_fixed), int(alpha_fixed),
                                      C.cast(cb, C.c_void_p), None, C.byref(st),
                                      (1 if det_pow else 0) | (2 if device_solver else 0))
    if rc != 0:
        raise NgsFHMMError(rc, L.nghmm_strerror(rc).decode())
    return F, A, st


TRACTS_VITERBI = 0    # nghmm_ibd_tracts sources (include/nghmm.h)
TRACTS_POSTERIOR = 1


class Tract(C.Structure):            # nghmm_tract (include/nghmm.h)
    _fields_ = [("first_site", C.c_uint64), ("n_sites", C.c_uint64), ("ind", C.c_uint32),
                ("reserved", C.c_uint32), ("post_sum", C.c_double)]


TRACT_DTYPE = np.dtype([("ind", np.uint32), ("first_site", np.uint64), ("n_sites", np.uint64),
                        ("post_sum", np.float64), ("post_mean", np.float64)])


def _tract_source(source):
    src = {"viterbi": TRACTS_VITERBI, "posterior": TRACTS_POSTERIOR}.get(source, source)
    if src not in (TRACTS_VITERBI, TRACTS_POSTERIOR):
        raise NgsFHMMError(-10, f"ibd_tracts: unknown source {source!r} ('viterbi' or 'posterior')")
    return src


def _tracts(call, check, source, threshold, min_sites):
    """One call for the count, one to fetch (nghmm_ibd_tracts / nghmm_chain_ibd_tracts)."""
    src = _tract_source(source)
    n = C.c_uint64(0)
    check(call(src, float(threshold), int(min_sites), None, 0, C.byref(n)))
    buf = (Tract * max(n.value, 1))()
    if n.value:
        got = C.c_uint64(0)
        check(call(src, float(threshold), int(min_sites), C.cast(buf, C.c_void_p), n.value,
                   C.byref(got)))
        assert got.value == n.value
    raw = np.frombuffer(buf, dtype=np.dtype([("first_site", np.uint64), ("n_sites", np.uint64),
                                             ("ind", np.uint32), ("reserved", np.uint32),
                                             ("post_sum", np.float64)]), count=n.value)
    out = np.empty(n.value, dtype=TRACT_DTYPE)
    for f in ("ind", "first_site", "n_sites", "post_sum"):
        out[f] = raw[f]
    out["post_mean"] = out["post_sum"] / np.maximum(out["n_sites"], 1)
    return out


def bed_lines(tracts, chrom_names, positions, ind_names):
    """BED text of tract records as scripts/convert_ibd.pl --ibd_pos prints it
    (convert_ibd.pl:99-130): ``CHR  START  END  IND_ID  LENGTH`` tab-separated, one line per
    tract, with START = pos[first] - 1, END = pos[last], LENGTH = END - START.
    chrom_names / positions: per site (global site index); ind_names: per individual."""
    lines = []
    for t in tracts:
        a = int(t["first_site"])
        b = a + int(t["n_sites"]) - 1
        start, end = int(positions[a]) - 1, int(positions[b])
        lines.append(f"{chrom_names[a]}\t{start}\t{end}\t{ind_names[int(t['ind'])]}\t{end - start}\n")
    return "".join(lines)


class TractScore(C.Structure):       # nghmm_tract_score (include/nghmm.h)
    _fields_ = [("log_p_ibd", C.c_double), ("log_p_non", C.c_double), ("post_min", C.c_double),
                ("post_min_site", C.c_uint64)]


# tract_support's records: nghmm_tract_score and the derived LOD, (log_p_ibd - log_p_non) / ln 10
TRACT_SCORE_DTYPE = np.dtype([("log_p_ibd", np.float64), ("log_p_non", np.float64),
                              ("post_min", np.float64), ("post_min_site", np.uint64),
                              ("lod", np.float64)])
_TRACT_RAW_DTYPE = np.dtype([("first_site", np.uint64), ("n_sites", np.uint64), ("ind", np.uint32),
                             ("reserved", np.uint32), ("post_sum", np.float64)])


def _tract_records(tracts, who):
    """tracts: ibd_tracts' structured array, or integers [n][3] of (ind, first_site, n_sites);
    as nghmm_tract records."""
    t = np.asarray(tracts)
    if t.dtype.names is None:
        if t.size == 0:
            t = t.reshape(0, 3)
        if t.ndim != 2 or t.shape[1] != 3 or not (np.issubdtype(t.dtype, np.integer) or t.size == 0):
            raise NgsFHMMError(-10, f"{who}: ranges are ibd_tracts' records or integers [n][3] "
                                    "of (ind, first_site, n_sites)")
        if t.size and (t.min() < 0 or t[:, 0].max() >= 2 ** 32):
            raise NgsFHMMError(-10, f"{who}: a negative value, or ind >= 2^32")
        cols = {"ind": t[:, 0], "first_site": t[:, 1], "n_sites": t[:, 2]}
    else:
        cols = {f: t[f] for f in ("ind", "first_site", "n_sites")}
    raw = np.zeros(len(t), dtype=_TRACT_RAW_DTYPE)
    for f, v in cols.items():
        raw[f] = v
    assert raw.itemsize == C.sizeof(Tract)
    return raw


def _tract_support(call, check, tracts):
    raw = _tract_records(tracts, "tract_support")
    n = len(raw)
    got = np.zeros(n, dtype=np.dtype([(f, TRACT_SCORE_DTYPE[f]) for f in TRACT_SCORE_DTYPE.names[:4]]))
    assert got.itemsize == C.sizeof(TractScore)
    check(call(C.c_void_p(raw.ctypes.data) if n else None, n, C.c_void_p(got.ctypes.data) if n else None))
    out = np.empty(n, dtype=TRACT_SCORE_DTYPE)
    for f in got.dtype.names:
        out[f] = got[f]
    with np.errstate(invalid="ignore"):     # (-inf) - (-inf): a range neither state can fill
        out["lod"] = (out["log_p_ibd"] - out["log_p_non"]) / math.log(10.0)
    return out


class TractBound(C.Structure):       # nghmm_tract_bound (include/nghmm.h)
    _fields_ = [("anchor", C.c_uint64), ("left_limit", C.c_uint64), ("right_limit", C.c_uint64),
                ("post_anchor", C.c_double), ("log_reach_left", C.c_double),
                ("log_reach_right", C.c_double)]


# tract_bounds' records: nghmm_tract_bound and the two reaches themselves, exp of their logarithms
TRACT_BOUND_DTYPE = np.dtype([("anchor", np.uint64), ("left_limit", np.uint64),
                              ("right_limit", np.uint64), ("post_anchor", np.float64),
                              ("log_reach_left", np.float64), ("log_reach_right", np.float64),
                              ("reach_left", np.float64), ("reach_right", np.float64)])
NO_ANCHOR = 2 ** 64 - 1     # an anchor the call resolves itself (UINT64_MAX)


def _tract_bounds(call, check, tracts, anchors, levels):
    raw = _tract_records(tracts, "tract_bounds")
    n = len(raw)
    lv = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float64)))
    if lv.ndim != 1:
        raise NgsFHMMError(-10, "tract_bounds: levels is a sequence of probabilities")
    m = len(lv)
    anc = None
    if anchors is not None:
        a = np.asarray(anchors)
        if a.shape != (n,) or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            raise NgsFHMMError(-10, "tract_bounds: anchors are integers [n], one per record")
        if a.size and a.min() < 0:
            raise NgsFHMMError(-10, "tract_bounds: a negative anchor")
        anc = np.ascontiguousarray(a, dtype=np.uint64)
    got = np.zeros(n, dtype=np.dtype([(f, TRACT_BOUND_DTYPE[f]) for f in TRACT_BOUND_DTYPE.names[:6]]))
    assert got.itemsize == C.sizeof(TractBound)
    start = np.zeros((n, m), dtype=np.uint64)
    end = np.zeros((n, m), dtype=np.uint64)
    ptr = lambda x: C.c_void_p(x.ctypes.data) if x is not None and x.size else None
    check(call(ptr(raw), n, ptr(anc), _dp(lv) if m else None, m, ptr(got), ptr(start), ptr(end)))
    out = np.empty(n, dtype=TRACT_BOUND_DTYPE)
    for f in got.dtype.names:
        out[f] = got[f]
    out["reach_left"] = np.exp(out["log_reach_left"])
    out["reach_right"] = np.exp(out["log_reach_right"])
    return out, start, end


# nghmm_freq_stat (include/nghmm.h): one record per site of freq_info
FREQ_STAT_DTYPE = np.dtype([("freq", np.float64), ("ll", np.float64), ("score", np.float64),
                            ("info", np.float64)])


def _freq_info(call, check, n_ind, n_sites, levels, cavity):
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.float64))
    if lv.ndim != 1:
        raise NgsFHMMError(-10, "freq_info: levels is a sequence of frequencies")
    m = len(lv)
    stats = np.zeros(n_sites, dtype=FREQ_STAT_DTYPE)
    curve = np.zeros((n_sites, m))
    cav = np.zeros((n_ind, n_sites)) if cavity else None
    check(call(m, _dp(lv) if m else None, C.c_void_p(stats.ctypes.data), _dp(curve) if m else None,
               _dp(cav) if cavity else None))
    return (stats, curve, cav) if cavity else (stats, curve)


def freq_std_errors(stats):
    """Standard errors of the allele frequencies from freq_info's records taken AT the estimates:
    1 / sqrt(info) where info > 0 and 0 < freq < 1, else NaN.  They are conditional on indF, alpha
    and the other sites' frequencies, which freq_info holds fixed."""
    info, f = np.asarray(stats["info"]), np.asarray(stats["freq"])
    ok = (info > 0) & (f > 0) & (f < 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, 1.0 / np.sqrt(np.where(ok, info, 1.0)), np.nan)


# nghmm_geno_site_stat and nghmm_geno_region_stat (include/nghmm.h): one record per site and one
# per (individual, region) of geno_smooth
GENO_SITE_STAT_DTYPE = np.dtype([(f, np.float64) for f in ("n0", "n1", "n2", "het_prior", "ibd", "alt_ibd")])
GENO_REGION_STAT_DTYPE = np.dtype([(f, np.float64) for f in ("het", "het_prior", "non_ibd", "dosage")])
assert GENO_SITE_STAT_DTYPE.itemsize == 48 and GENO_REGION_STAT_DTYPE.itemsize == 32


def _geno_smooth(call_fn, check, n_ind, n_sites, regions, sites, post, call):
    u64p = C.POINTER(C.c_uint64)
    if regions is None:
        reg = np.zeros((0, 2), dtype=np.uint64)
    else:
        reg = np.asarray(regions)
        if reg.size == 0:
            reg = reg.reshape(0, 2)
        if reg.ndim != 2 or reg.shape[1] != 2 or not np.issubdtype(reg.dtype, np.integer) or \
                (reg < 0).any():
            raise NgsFHMMError(-10, "geno_smooth: regions is an [R][2] array of site indices "
                                    "(begin, end)")
        reg = reg.astype(np.uint64)
    R = len(reg)
    begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    out = {}
    if R:
        out["regions"] = np.zeros((n_ind, R), dtype=GENO_REGION_STAT_DTYPE)
    if sites:
        out["sites"] = np.zeros(n_sites, dtype=GENO_SITE_STAT_DTYPE)
    if post:
        out["post"] = np.zeros((n_sites, n_ind, 3))
    if call:
        out["call"] = np.zeros((n_sites, n_ind), dtype=np.uint8)
    check(call_fn(R, begin.ctypes.data_as(u64p) if R else None, end.ctypes.data_as(u64p) if R else None,
                  C.c_void_p(out["regions"].ctypes.data) if R else None,
                  C.c_void_p(out["sites"].ctypes.data) if sites else None,
                  _dp(out["post"]) if post else None,
                  out["call"].ctypes.data_as(C.POINTER(C.c_uint8)) if call else None))
    return out


def geno_em_freq(site_stats, n_ind):
    """The exact EM update of every site's allele frequency under the model, from geno_smooth's
    site records: (n1 + 2 n2 - alt_ibd) / (2 n_ind - ibd), alternative allele copies over allele
    copies, an IBD individual carrying one copy; NaN where 2 n_ind - ibd is 0.  em_freq - freq is
    freq_info's score in frequency units: score f (1 - f) = (em_freq - f) (2 n_ind - ibd)."""
    st = site_stats
    num = np.asarray(st["n1"]) + 2 * np.asarray(st["n2"]) - np.asarray(st["alt_ibd"])
    den = 2.0 * n_ind - np.asarray(st["ibd"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0, np.nan, num / np.where(den == 0, 1.0, den))


def het_outside_ibd(region_stats):
    """Heterozygosity outside IBD per (individual, region) from geno_smooth's region records:
    het / non_ibd; NaN where non_ibd is 0."""
    het, non = np.asarray(region_stats["het"]), np.asarray(region_stats["non_ibd"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(non == 0, np.nan, het / np.where(non == 0, 1.0, non))


# nghmm_path_stats (include/nghmm.h): one record per (draw, individual) of sample_paths
PATH_STATS_DTYPE = np.dtype([("ibd_sites", np.uint64), ("n_tracts", np.uint64),
                             ("longest_sites", np.uint64), ("ibd_mb", np.float64)])


def _sample_paths(call, check, n_ind, n_sites, n_draws, seed, keep):
    n_draws, keep = int(n_draws), int(keep)
    if n_draws < 0 or keep < 0 or n_draws >= 2 ** 32 or keep >= 2 ** 32:
        raise NgsFHMMError(-10, f"sample_paths: n_draws = {n_draws}, keep = {keep}")
    stats = np.zeros((n_draws, n_ind), dtype=PATH_STATS_DTYPE)
    paths = np.zeros((keep, n_ind, n_sites), dtype=np.uint8)
    check(call(int(seed) & (2 ** 64 - 1), n_draws, C.c_void_p(stats.ctypes.data), keep,
               paths.ctypes.data_as(C.POINTER(C.c_uint8)) if keep else None))
    return stats, paths


def path_stats_summary(stats, q=(0.025, 0.5, 0.975)):
    """Per-individual quantiles over the draws of every field of sample_paths' records:
    {field: array [len(q)][I]}."""
    return {f: np.quantile(stats[f].astype(np.float64), q, axis=0) for f in PATH_STATS_DTYPE.names}


# nghmm_info (include/nghmm.h): one record per individual of obs_info
INFO_DTYPE = np.dtype([("lkl", np.float64), ("g_F", np.float64), ("g_A", np.float64),
                       ("h_FF", np.float64), ("h_FA", np.float64), ("h_AA", np.float64)])


def _obs_info(call, check, n_ind, indF, alpha):
    if (indF is None) != (alpha is None):
        raise NgsFHMMError(-10, "obs_info: indF and alpha are given both or neither")
    out = np.zeros(n_ind, dtype=INFO_DTYPE)
    if indF is None:
        check(call(None, None, C.c_void_p(out.ctypes.data)))
        return out
    F = np.ascontiguousarray(np.broadcast_to(np.asarray(indF, dtype=np.float64), (n_ind,)))
    A = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (n_ind,)))
    check(call(_dp(F), _dp(A), C.c_void_p(out.ctypes.data)))
    return out


def std_errors(info, indF, alpha):
    """Standard errors of indF and alpha and their correlation from obs_info's records taken AT
    the estimates (indF, alpha): (se_indF, se_alpha, corr), one value per individual.  They are
    conditional on the allele frequencies, which obs_info holds fixed.  The rule (the host's
    --indF_se applies the same one):

    * A parameter on its bound is treated as fixed: its se is NaN and it leaves the inversion.
      On its bound: indF < 1e-5 or indF > 1 - 1e-5 (the .indF file's NA rule, EM.cpp:293-310);
      alpha <= 1e-15 or alpha >= 10 (the optimizer's box).
    * indF on its bound makes all three NaN: alpha is then unidentified, which is why the
      reference prints NA for it.
    * A free block of -h (the observed information) that is not positive definite gives NaN for
      that block: both free, -h_FF > 0 and det(-h) > 0 are needed; alpha on its bound, -h_FF > 0.
    * Otherwise se = sqrt of the diagonal of (-h)^-1 over the free parameters, corr its
      off-diagonal over the product of the two se (NaN unless both are free)."""
    F = np.broadcast_to(np.asarray(indF, dtype=np.float64), info.shape)
    A = np.broadcast_to(np.asarray(alpha, dtype=np.float64), info.shape)
    n = len(info)
    se_F, se_A, corr = (np.full(n, np.nan) for _ in range(3))
    for i in range(n):
        if F[i] < 1e-5 or F[i] > 1 - 1e-5:
            continue
        a, b, d = -info["h_FF"][i], -info["h_FA"][i], -info["h_AA"][i]
        if A[i] <= 1e-15 or A[i] >= 10.0:
            if a > 0:
                se_F[i] = math.sqrt(1.0 / a)
            continue
        det = a * d - b * b
        if a > 0 and det > 0:
            se_F[i] = math.sqrt(d / det)
            se_A[i] = math.sqrt(a / det)
            corr[i] = -b / math.sqrt(a * d)
    return se_F, se_A, corr


SUMMARY_VITERBI = 1    # nghmm_ibd_summary sources, a bit mask (include/nghmm.h)
SUMMARY_POSTERIOR = 2
# sites per lane of the summary pass: kSummarySeg of csrc/kernels_summary.hpp.  A region is cut
# into pieces at the multiples of this number, which fixes the order its sums are added in.
SUMMARY_SEGMENT_SITES = 2048


class RegionStat(C.Structure):       # nghmm_region_stat (include/nghmm.h)
    _fields_ = [("vit_sites", C.c_uint64), ("post_sites", C.c_uint64), ("post_sum", C.c_double),
                ("vit_mb", C.c_double)]


class SiteStat(C.Structure):         # nghmm_site_stat (include/nghmm.h)
    _fields_ = [("vit_count", C.c_uint32), ("post_count", C.c_uint32), ("post_sum", C.c_double)]


REGION_STAT_DTYPE = np.dtype([("vit_sites", np.uint64), ("post_sites", np.uint64),
                              ("post_sum", np.float64), ("vit_mb", np.float64)])
SITE_STAT_DTYPE = np.dtype([("vit_count", np.uint32), ("post_count", np.uint32),
                            ("post_sum", np.float64)])
assert REGION_STAT_DTYPE.itemsize == C.sizeof(RegionStat) == 32
assert SITE_STAT_DTYPE.itemsize == C.sizeof(SiteStat) == 16


def _summary_what(what):
    if isinstance(what, (int, np.integer)):
        return int(what)
    names = {"viterbi": SUMMARY_VITERBI, "posterior": SUMMARY_POSTERIOR}
    mask = 0
    for w in ((what,) if isinstance(what, str) else what):
        if w not in names:
            raise NgsFHMMError(-10, f"ibd_summary: unknown source {w!r} ('viterbi' or 'posterior')")
        mask |= names[w]
    return mask


def _ibd_summary(call, check, n_ind, n_sites, regions, what, threshold, sites):
    u64p = C.POINTER(C.c_uint64)
    if regions is None:
        reg = np.zeros((0, 2), dtype=np.uint64)
    else:
        reg = np.asarray(regions)
        if reg.size == 0:
            reg = reg.reshape(0, 2)
        if reg.ndim != 2 or reg.shape[1] != 2 or not np.issubdtype(reg.dtype, np.integer) or \
                (reg < 0).any():
            raise NgsFHMMError(-10, "ibd_summary: regions is an [R][2] array of site indices "
                                    "(begin, end)")
        reg = reg.astype(np.uint64)
    R = len(reg)
    begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    region_stats = np.zeros((n_ind, R), dtype=REGION_STAT_DTYPE) if R else None
    site_stats = np.zeros(n_sites, dtype=SITE_STAT_DTYPE) if sites else None
    check(call(_summary_what(what), float(threshold), R,
               begin.ctypes.data_as(u64p) if R else None, end.ctypes.data_as(u64p) if R else None,
               C.c_void_p(region_stats.ctypes.data) if R else None,
               C.c_void_p(site_stats.ctypes.data) if sites else None))
    return region_stats, site_stats


EXPECT_VITERBI = 1     # nghmm_ibd_expect: also the posterior probability of the decoded path


class ExpectRegion(C.Structure):     # nghmm_expect_region (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("ibd", "starts", "switches", "ibd_mb", "entropy",
                                          "log_p_path")]


class ExpectSite(C.Structure):       # nghmm_expect_site (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("on", "off", "ibd", "entropy")]


EXPECT_REGION_DTYPE = np.dtype([(n, np.float64) for n, _ in ExpectRegion._fields_])
EXPECT_SITE_DTYPE = np.dtype([(n, np.float64) for n, _ in ExpectSite._fields_])
assert EXPECT_REGION_DTYPE.itemsize == C.sizeof(ExpectRegion) == 48
assert EXPECT_SITE_DTYPE.itemsize == C.sizeof(ExpectSite) == 32


def _ibd_expect(call, check, n_ind, n_sites, regions, sites, viterbi):
    u64p = C.POINTER(C.c_uint64)
    if regions is None:
        reg = np.array([[0, n_sites]], dtype=np.uint64)
    else:
        reg = np.asarray(regions)
        if reg.size == 0:
            reg = reg.reshape(0, 2)
        if reg.ndim != 2 or reg.shape[1] != 2 or not np.issubdtype(reg.dtype, np.integer) or \
                (reg < 0).any():
            raise NgsFHMMError(-10, "ibd_expect: regions is an [R][2] array of site indices "
                                    "(begin, end)")
        reg = reg.astype(np.uint64)
    R = len(reg)
    begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    region_stats = np.zeros((n_ind, R), dtype=EXPECT_REGION_DTYPE) if R else None
    site_stats = np.zeros(n_sites, dtype=EXPECT_SITE_DTYPE) if sites else None
    check(call(EXPECT_VITERBI if viterbi else 0, R,
               begin.ctypes.data_as(u64p) if R else None, end.ctypes.data_as(u64p) if R else None,
               C.c_void_p(region_stats.ctypes.data) if R else None,
               C.c_void_p(site_stats.ctypes.data) if sites else None))
    return region_stats, site_stats


def expect_tract_length(region_stats):
    """(sites, mb) of ibd_expect's region records: the expected IBD sites per expected tract and
    the expected Mb per expected tract, NaN where `starts` is 0."""
    st = np.asarray(region_stats["starts"], dtype=np.float64)
    sites = np.full(st.shape, np.nan)
    mb = np.full(st.shape, np.nan)
    np.divide(region_stats["ibd"], st, out=sites, where=st != 0)
    np.divide(region_stats["ibd_mb"], st, out=mb, where=st != 0)
    return sites, mb


MOMENTS_MB = 1         # nghmm_ibd_moments: A = IBD Mb instead of IBD sites


class MomentRegion(C.Structure):     # nghmm_moment_region (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("mean_a", "mean_t", "var_a", "cov_at", "var_t")]


MOMENT_REGION_DTYPE = np.dtype([(n, np.float64) for n, _ in MomentRegion._fields_])
assert MOMENT_REGION_DTYPE.itemsize == C.sizeof(MomentRegion) == 40


def _ibd_moments(call, check, n_ind, n_sites, regions, length):
    u64p = C.POINTER(C.c_uint64)
    if length not in ("sites", "mb"):
        raise NgsFHMMError(-10, "ibd_moments: length is 'sites' or 'mb'")
    if regions is None:
        reg = np.array([[0, n_sites]], dtype=np.uint64)
    else:
        reg = np.asarray(regions)
        if reg.size == 0:
            reg = reg.reshape(0, 2)
        if reg.ndim != 2 or reg.shape[1] != 2 or not np.issubdtype(reg.dtype, np.integer) or \
                (reg < 0).any():
            raise NgsFHMMError(-10, "ibd_moments: regions is an [R][2] array of site indices "
                                    "(begin, end)")
        reg = reg.astype(np.uint64)
    R = len(reg)
    begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    stats = np.zeros((n_ind, R), dtype=MOMENT_REGION_DTYPE)
    check(call(MOMENTS_MB if length == "mb" else 0, R,
               begin.ctypes.data_as(u64p) if R else None, end.ctypes.data_as(u64p) if R else None,
               C.c_void_p(stats.ctypes.data) if R else None))
    return stats


def moment_sd(stats):
    """What ibd_moments' records say about uncertainty, as a dict of arrays of stats' shape:
    sd_a, sd_t (posterior standard deviations), corr (NaN where a variance is 0), tract_length =
    mean_a / mean_t and tract_length_sd, its delta-method posterior sd
    sqrt(var_a - 2 R cov_at + R^2 var_t) / mean_t with R = tract_length (both NaN where mean_t is
    0)."""
    va = np.asarray(stats["var_a"], dtype=np.float64)
    vt = np.asarray(stats["var_t"], dtype=np.float64)
    cov = np.asarray(stats["cov_at"], dtype=np.float64)
    ma = np.asarray(stats["mean_a"], dtype=np.float64)
    mt = np.asarray(stats["mean_t"], dtype=np.float64)
    sd_a, sd_t = np.sqrt(va), np.sqrt(vt)
    corr = np.full(va.shape, np.nan)
    ok = (va > 0) & (vt > 0)
    np.divide(cov, sd_a * sd_t, out=corr, where=ok)
    ratio = np.full(va.shape, np.nan)
    np.divide(ma, mt, out=ratio, where=mt != 0)
    with np.errstate(invalid="ignore"):
        q = np.maximum(va - 2 * ratio * cov + ratio * ratio * vt, 0.0)
        length_sd = np.full(va.shape, np.nan)
        np.divide(np.sqrt(q), np.abs(mt), out=length_sd, where=mt != 0)
    return {"sd_a": sd_a, "sd_t": sd_t, "corr": corr, "tract_length": ratio,
            "tract_length_sd": length_sd}


BYLENGTH_MB = 1        # nghmm_ibd_by_length: thresholds and lengths in Mb instead of sites


class ByLengthStat(C.Structure):     # nghmm_bylength_stat (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("tracts", "length")]


BYLENGTH_DTYPE = np.dtype([(n, np.float64) for n, _ in ByLengthStat._fields_])
assert BYLENGTH_DTYPE.itemsize == C.sizeof(ByLengthStat) == 16


def _ibd_by_length(call, check, n_ind, n_sites, min_len, unit, regions, dtype=None,
                   name="ibd_by_length", mb_flag=None):
    """What ibd_by_length and ibd_longest share: the checks of unit, thresholds and regions, the
    record array [I][R][K] of `dtype` and the call; mb_flag is the entry's own bit for Mb."""
    u64p = C.POINTER(C.c_uint64)
    L, reg = _by_length_args(n_sites, min_len, unit, regions, name)
    R, K = len(reg), len(L)
    begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    stats = np.zeros((n_ind, R, K), dtype=BYLENGTH_DTYPE if dtype is None else dtype)
    mb_flag = BYLENGTH_MB if mb_flag is None else mb_flag
    check(call(mb_flag if unit == "mb" else 0, K, _dp(L) if K else None, R,
               begin.ctypes.data_as(u64p) if R else None, end.ctypes.data_as(u64p) if R else None,
               C.c_void_p(stats.ctypes.data) if R and K else None))
    return stats


def _by_length_args(n_sites, min_len, unit, regions, name):
    """The argument checks of ibd_by_length, ibd_longest and ibd_long: (thresholds float64 [K],
    regions uint64 [R][2]); regions None is one region over all sites."""
    if unit not in ("sites", "mb"):
        raise NgsFHMMError(-10, f"{name}: unit is 'sites' or 'mb'")
    L = np.ascontiguousarray(np.atleast_1d(np.asarray(min_len, dtype=np.float64)))
    if L.ndim != 1:
        raise NgsFHMMError(-10, f"{name}: min_len is a number or a list of numbers")
    if regions is None:
        reg = np.array([[0, n_sites]], dtype=np.uint64)
    else:
        reg = np.asarray(regions)
        if reg.size == 0:
            reg = reg.reshape(0, 2)
        if reg.ndim != 2 or reg.shape[1] != 2 or not np.issubdtype(reg.dtype, np.integer) or \
                (reg < 0).any():
            raise NgsFHMMError(-10, f"{name}: regions is an [R][2] array of site indices "
                                    "(begin, end)")
        reg = reg.astype(np.uint64)
    return L, reg


def by_length_classes(stats):
    """ibd_by_length's records [..][K] as length classes: a dict of float arrays [..][K], class k
    being [L_k, L_{k+1}) and the last one open: tracts and length as differences of successive
    thresholds, mean_length = length / tracts (NaN where tracts is 0)."""
    tr = np.asarray(stats["tracts"], dtype=np.float64)
    ln = np.asarray(stats["length"], dtype=np.float64)
    ct, cl = tr.copy(), ln.copy()
    ct[..., :-1] -= tr[..., 1:]
    cl[..., :-1] -= ln[..., 1:]
    mean = np.full(ct.shape, np.nan)
    np.divide(cl, ct, out=mean, where=ct != 0)
    return {"tracts": ct, "length": cl, "mean_length": mean}


LONGEST_MB = 1         # nghmm_ibd_longest: thresholds in Mb instead of sites


class LongestStat(C.Structure):      # nghmm_longest_stat (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("p_any", "p_none")]


LONGEST_DTYPE = np.dtype([(n, np.float64) for n, _ in LongestStat._fields_])
assert LONGEST_DTYPE.itemsize == C.sizeof(LongestStat) == 16


COUNT_MB = 1           # nghmm_ibd_count: thresholds in Mb instead of sites
COUNT_MAX = 16         # nghmm_ibd_count: the largest n_counts


def count_summary(prob, levels=(0.025, 0.5, 0.975)):
    """ibd_count's records [..][M + 1] in short: a dict of
    mean_lower [..]  sum of c p_c + M p_M: a lower bound of E[C], equal to it where prob[..., M] is 0;
    p_more [..]      prob[..., M], the probability of M runs or more;
    mode [..]        the most probable count (the first of equals; M stands for "M or more");
    quantiles [..][len(levels)]  integers: the smallest c whose cumulative probability reaches the
                     level, M meaning "M or more" (censored)."""
    p = np.asarray(prob, dtype=np.float64)
    if p.ndim < 1 or p.shape[-1] < 2:
        raise NgsFHMMError(-10, "count_summary: prob is [..][M + 1] with M >= 1")
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if lv.ndim != 1 or not ((lv >= 0) & (lv <= 1)).all():
        raise NgsFHMMError(-10, "count_summary: levels lie in [0, 1]")
    M = p.shape[-1] - 1
    cum = np.cumsum(p[..., :M], axis=-1)
    q = (cum[..., None, :] < lv[:, None]).sum(axis=-1).astype(np.int64)
    return {"mean_lower": (p * np.arange(M + 1)).sum(axis=-1), "p_more": p[..., M].copy(),
            "mode": np.argmax(p, axis=-1).astype(np.int64), "quantiles": q}


LONG_MOMENTS_MB = 1    # nghmm_ibd_long_moments: thresholds and lengths in Mb instead of sites


class LongMomentStat(C.Structure):   # nghmm_long_moment_stat (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("mean_a", "mean_t", "var_a", "cov_at", "var_t")]


LONG_MOMENT_DTYPE = np.dtype([(n, np.float64) for n, _ in LongMomentStat._fields_])
assert LONG_MOMENT_DTYPE.itemsize == C.sizeof(LongMomentStat) == 40


def long_moment_sd(stats, total=None):
    """What ibd_long_moments' records say about uncertainty, as a dict of arrays of stats' shape:
    moment_sd's sd_a, sd_t, corr (NaN where a variance is 0), tract_length = mean_a / mean_t and
    tract_length_sd, its delta-method posterior sd (both NaN where mean_t is 0); and with total --
    the sites or Mb of the region, a number or an array that broadcasts against stats -- share =
    mean_a / total (F_ROH above the threshold) and share_sd = sd_a / total (NaN where total is
    0)."""
    out = moment_sd(stats)
    if total is not None:
        tot = np.broadcast_to(np.asarray(total, dtype=np.float64), out["sd_a"].shape)
        for name, src in (("share", np.asarray(stats["mean_a"], dtype=np.float64)), ("share_sd", out["sd_a"])):
            v = np.full(tot.shape, np.nan)
            np.divide(src, tot, out=v, where=tot != 0)
            out[name] = v
    return out


LONG_MB = 1            # nghmm_ibd_long: thresholds in Mb instead of sites


class LongRegionStat(C.Structure):   # nghmm_long_region_stat (include/nghmm.h)
    _fields_ = [(n, C.c_double) for n in ("sites", "mb")]


class LongSiteStat(C.Structure):     # nghmm_long_site_stat (include/nghmm.h)
    _fields_ = [("sum", C.c_double), ("count", C.c_uint64)]


LONG_REGION_DTYPE = np.dtype([(n, np.float64) for n, _ in LongRegionStat._fields_])
LONG_SITE_DTYPE = np.dtype([("sum", np.float64), ("count", np.uint64)])
assert LONG_REGION_DTYPE.itemsize == C.sizeof(LongRegionStat) == 16
assert LONG_SITE_DTYPE.itemsize == C.sizeof(LongSiteStat) == 16


def _ibd_long(call, check, n_ind, n_sites, min_len, unit, regions, sites, post, threshold):
    """ibd_long of a handle or a chain: _ibd_by_length's argument checks, the arrays asked for,
    the call."""
    u64p = C.POINTER(C.c_uint64)
    name = "ibd_long"
    L, reg = _by_length_args(n_sites, min_len, unit, None if regions is False else regions, name)
    if regions is False:
        reg = reg[:0]
    R, K = len(reg), len(L)
    out = {}
    if R:
        out["regions"] = np.zeros((n_ind, R, K), dtype=LONG_REGION_DTYPE)
    if sites:
        out["sites"] = np.zeros((n_sites, K), dtype=LONG_SITE_DTYPE)
    if post:
        out["post"] = np.zeros((K, n_ind, n_sites))
    begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    ptr = lambda key: C.c_void_p(out[key].ctypes.data) if key in out and K else None
    check(call(LONG_MB if unit == "mb" else 0, K, _dp(L) if K else None, float(threshold), R,
               begin.ctypes.data_as(u64p) if R else None, end.ctypes.data_as(u64p) if R else None,
               ptr("regions"), ptr("sites"), _dp(out["post"]) if post and K else None))
    return out


def long_tracts(post_k, pos_dist, threshold=0.5, min_sites=1):
    """Tracts called from one plane of ibd_long's post, P_k [I][S]: the maximal runs of
    P_k >= threshold, cut at chromosome starts, of at least min_sites sites, in TRACT_DTYPE as
    ibd_tracts returns them (ordered by (ind, first_site); post_sum = the run's sum of P_k), so
    that bed_lines and tract_support take them as they are."""
    p = np.asarray(post_k, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != len(pos_dist):
        raise NgsFHMMError(-10, "long_tracts: post_k is [I][S] and pos_dist [S]")
    I, S = p.shape
    on = p >= threshold
    cs = np.isinf(np.asarray(pos_dist, dtype=np.float64))
    if S:
        cs[0] = True
    prev = np.concatenate([np.zeros((I, 1), dtype=bool), on[:, :-1]], axis=1)
    nxt_cs = np.r_[cs[1:], True] if S else cs
    nxt = np.concatenate([on[:, 1:], np.zeros((I, 1), dtype=bool)], axis=1)
    first = on & (~prev | cs[None, :])
    last = on & (~nxt | nxt_cs[None, :])
    ind, a = np.nonzero(first)
    _, b = np.nonzero(last)
    csum = np.concatenate([np.zeros((I, 1)), np.cumsum(np.where(on, p, 0.0), axis=1)], axis=1)
    n = (b - a + 1).astype(np.uint64)
    keep = n >= min_sites
    out = np.empty(int(keep.sum()), dtype=TRACT_DTYPE)
    out["ind"], out["first_site"], out["n_sites"] = ind[keep], a[keep], n[keep]
    out["post_sum"] = (csum[ind, b + 1] - csum[ind, a])[keep]
    out["post_mean"] = out["post_sum"] / np.maximum(out["n_sites"], 1)
    return out


def longest_classes(stats):
    """ibd_longest's records [..][K] as the distribution of the longest run: a float array
    [..][K + 1] -- class 0: the longest run is below L_1 (p_none of the first threshold, which
    includes no run at all), class k: it lies in [L_k, L_{k+1}) (a difference of p_any), class K:
    it is at least L_K.  The classes add up to 1 to the accuracy of p_any + p_none."""
    pa = np.asarray(stats["p_any"], dtype=np.float64)
    out = np.empty(pa.shape[:-1] + (pa.shape[-1] + 1,))
    out[..., 0] = np.asarray(stats["p_none"], dtype=np.float64)[..., 0]
    out[..., 1:-1] = pa[..., :-1] - pa[..., 1:]
    out[..., -1] = pa[..., -1]
    return out


SHARING_VITERBI = 1    # nghmm_ibd_sharing sources, a bit mask (include/nghmm.h)
SHARING_POSTERIOR = 2
# the least sites per K-split of the sharing kernels: kSharingSplit of csrc/kernels_sharing.hpp.
# The splits' partial matrices are added in site order, which fixes the order of post_prod's sum.
SHARING_SPLIT_SITES = 1024


def sharing_splits(n_ind, site_begin, site_end):
    """(first, length, number) of the K-splits nghmm_ibd_sharing cuts [site_begin, site_end) into:
    sharing_plan of csrc/kernels_sharing.hpp (include/nghmm.h states the rule)."""
    first = site_begin // 64 * 64
    span = site_end - first
    cap = max(1, min(1024, (1 << 28) // (8 * n_ind * n_ind)))
    n = min(-(-span // SHARING_SPLIT_SITES), cap)
    length = -(-(-(-span // n)) // 64) * 64
    return first, length, -(-span // length)


def _ibd_sharing(call, check, n_ind, n_sites, what, threshold, site_begin, site_end):
    names = {"viterbi": SHARING_VITERBI, "posterior": SHARING_POSTERIOR,
             "vit_both": SHARING_VITERBI, "post_both": SHARING_POSTERIOR,
             "post_prod": SHARING_POSTERIOR}
    outputs = {"viterbi": ("vit_both",), "posterior": ("post_both", "post_prod")}
    mask, asked = 0, []
    for w in ((what,) if isinstance(what, str) else what):
        if w not in names:
            raise NgsFHMMError(-10, f"ibd_sharing: unknown source {w!r} ('viterbi', 'posterior', or "
                                    "one output: 'vit_both', 'post_both', 'post_prod')")
        mask |= names[w]
        asked += [o for o in outputs.get(w, (w,)) if o not in asked]
    out = {o: np.zeros((n_ind, n_ind), dtype=np.float64 if o == "post_prod" else np.uint64)
           for o in ("vit_both", "post_both", "post_prod") if o in asked}
    u64p = C.POINTER(C.c_uint64)
    end = n_sites if site_end is None else site_end
    if site_begin < 0 or end < 0:
        raise NgsFHMMError(-10, "ibd_sharing: negative site index")
    check(call(mask, float(threshold), int(site_begin), int(end),
               out["vit_both"].ctypes.data_as(u64p) if "vit_both" in out else None,
               out["post_both"].ctypes.data_as(u64p) if "post_both" in out else None,
               _dp(out["post_prod"]) if "post_prod" in out else None))
    return out


def sharing_jaccard(both):
    """both[i][j] / (both[i][i] + both[j][j] - both[i][j]) of a sharing matrix (vit_both,
    post_both): the shared IBD sites over the sites at which either is IBD; 0 where neither is
    IBD anywhere."""
    b = np.asarray(both, dtype=np.float64)
    if b.ndim != 2 or b.shape[0] != b.shape[1]:
        raise NgsFHMMError(-10, "sharing_jaccard: both is an [I][I] matrix")
    dg = np.diag(b)
    den = dg[:, None] + dg[None, :] - b
    out = np.zeros_like(b)
    np.divide(b, den, out=out, where=den != 0)
    return out


def chromosome_regions(pos_dist):
    """One region per chromosome, [R][2] (begin, end) site indices: a chromosome starts at site 0
    and at every site whose distance is +inf."""
    d = np.asarray(pos_dist, dtype=np.float64)
    if d.ndim != 1 or len(d) == 0:
        raise NgsFHMMError(-10, "chromosome_regions: pos_dist is a non-empty [S] array")
    start = np.isinf(d)
    start[0] = True
    begin = np.flatnonzero(start)
    return np.stack([begin, np.r_[begin[1:], len(d)]], axis=1).astype(np.int64)


def window_regions(pos_dist, n_sites):
    """Windows of n_sites sites, [R][2] (begin, end) site indices, that restart at every
    chromosome start: no window spans two chromosomes, and the last window of a chromosome holds
    what is left of it."""
    n_sites = int(n_sites)
    if n_sites < 1:
        raise NgsFHMMError(-10, f"window_regions: n_sites = {n_sites}")
    out = []
    for a, b in chromosome_regions(pos_dist):
        begin = np.arange(a, b, n_sites)
        out.append(np.stack([begin, np.minimum(begin + n_sites, b)], axis=1))
    return np.concatenate(out).astype(np.int64)


KERNEL_SLOTS = {"emission": 0, "forward": 1, "backward": 2, "lkl_batch": 3, "est_maf": 4,
                "viterbi": 5, "lkl_first": 6, "bfgs": 7}


class NgsFHMM:
    """Device-resident EM state of one GPU (the reference's ``params`` + ``EM``)."""

    def __init__(self, n_ind, n_sites, device=0, mode=MODE_EXACT, _replica_of=None):
        self.lib = load_library()
        self.n_ind, self.n_sites = int(n_ind), int(n_sites)
        self.mode = mode
        self._h = C.c_void_p()
        self._parent = _replica_of          # keeps the parent alive
        self._replicas = weakref.WeakSet()  # a parent closes its live replicas before itself
        if _replica_of is not None:
            self._check(self.lib.nghmm_create_replica(C.byref(self._h), _replica_of._h))
            _replica_of._replicas.add(self)
        else:
            self._check(self.lib.nghmm_create(C.byref(self._h), self.n_ind, self.n_sites, device,
                                              mode))
        self.tot_lkl = 0.0        # parse_args.cpp:31-32
        self.prev_tot_lkl = 0.0
        self.ind_lkl = np.full(self.n_ind, -math.inf)  # parse_args.cpp:412
        self.last_stats = None
        self.iterations = 0

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc):
        err = getattr(self, "_shard_err", None)
        if err:                      # raised inside the site-shard all-gather callback
            e = err[0]
            del err[:]
            raise e
        if rc != 0:
            msg = self.lib.nghmm_last_error().decode() or self.lib.nghmm_strerror(rc).decode()
            raise NgsFHMMError(rc, msg)

    def replica(self):
        """A handle that shares this one's (loaded) data and owns its own EM state and stream
        (nghmm_create_replica): multi-start runs, ngsF-HMM.sh:77-101."""
        return NgsFHMM(self.n_ind, self.n_sites, mode=self.mode, _replica_of=self)

    def close(self, _finalizing=False):
        """Destroys the handle.  A parent whose replicas are still open refuses, as the library
        does (they share its data): close them first.  Garbage collection (no order is
        guaranteed there) closes a parent's remaining replicas before the parent."""
        if getattr(self, "_h", None) is not None and self._h:
            live = [r for r in list(getattr(self, "_replicas", ())) if not r.closed]
            if live and not _finalizing:
                raise NgsFHMMError(-10, f"{len(live)} replica(s) of this handle are still open: "
                                        "close them first")
            for r in live:
                r.close(_finalizing=True)
            self._check(self.lib.nghmm_destroy(self._h))
            self._h = C.c_void_p()

    @property
    def closed(self):
        return not self._h

    def set_switch(self, name, value):
        """A measurement / debugging switch of this handle (nghmm_set_switch, include/nghmm_debug.h)."""
        self._check(self.lib.nghmm_set_switch(self._h, name.encode(), int(value)))

    def __del__(self):
        try:
            self.close(_finalizing=True)
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    # -- data --------------------------------------------------------------
    def load(self, gl, pos_dist):
        """gl: [S][I][3] normalised natural-log GLs (binary --geno order);
        pos_dist: [S] distances in Mb, inf at chromosome starts."""
        gl = np.ascontiguousarray(gl, dtype=np.float64)
        pos_dist = np.ascontiguousarray(pos_dist, dtype=np.float64)
        if gl.shape != (self.n_sites, self.n_ind, 3) or pos_dist.shape != (self.n_sites,):
            raise NgsFHMMError(-10, f"load: shapes {gl.shape} {pos_dist.shape} do not match "
                                    f"({self.n_sites}, {self.n_ind}, 3)")
        self._check(self.lib.nghmm_load_gl(self._h, _dp(gl), _dp(pos_dist)))

    def load_raw(self, gl_raw, pos_dist, space=0, call_geno=False, check_nan=False):
        """Raw genotype likelihoods as read from the input file; conversion to log space,
        normalisation and optional genotype calling happen on the device
        (nghmm_load_gl_raw).  space: 0 log, 1 normal space from a binary file, 2 normal
        space from a text file."""
        gl_raw = np.ascontiguousarray(gl_raw, dtype=np.float64)
        pos_dist = np.ascontiguousarray(pos_dist, dtype=np.float64)
        if gl_raw.shape != (self.n_sites, self.n_ind, 3) or pos_dist.shape != (self.n_sites,):
            raise NgsFHMMError(-10, f"load_raw: shapes {gl_raw.shape} {pos_dist.shape} do not "
                                    f"match ({self.n_sites}, {self.n_ind}, 3)")
        self._check(self.lib.nghmm_load_gl_raw(self._h, _dp(gl_raw), int(space), int(call_geno),
                                               int(check_nan), _dp(pos_dist)))

    @property
    def gl(self):
        """[S][I][3] prepared (natural-log, normalised) genotype likelihoods."""
        out = np.empty((self.n_sites, self.n_ind, 3))
        self._check(self.lib.nghmm_get_gl(self._h, _dp(out)))
        return out

    def geno_posteriors(self, site_begin=0, n_sites=None):
        """[n_sites][I][3] genotype posteriors of the .geno output (EM.cpp:367-376), from the
        path of the last viterbi() call."""
        n = self.n_sites - site_begin if n_sites is None else n_sites
        out = np.empty((n, self.n_ind, 3))
        self._check(self.lib.nghmm_geno_posteriors(self._h, int(site_begin), int(n), _dp(out)))
        return out

    def format_fixed6(self, values):
        """printf("%f") of a [rows][cols] array of values in [0, 1], on the device: tab-separated,
        one line per row, as bytes."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        rows, cols = v.shape
        buf = C.create_string_buffer(rows * cols * 9)
        self._check(self.lib.nghmm_format_fixed6(self._h, _dp(v), rows, cols, buf))
        return buf.raw

    def format_posteriors(self, ind_begin=0, n_ind=None):
        """The .ibd file's posterior lines of individuals [ind_begin, ind_begin + n_ind) as
        bytes: "%f" values, tab-separated, one line per individual (EM.cpp:347-353)."""
        n = self.n_ind - ind_begin if n_ind is None else n_ind
        buf = C.create_string_buffer(n * 9 * self.n_sites)
        self._check(self.lib.nghmm_format_posteriors(self._h, int(ind_begin), int(n), buf))
        return buf.raw

    def load_chunks(self, pos_dist, chunks, space=0, call_geno=False, check_nan=False):
        """Chunked loading (nghmm_load_begin / _sites / _end): ``chunks`` yields
        ``(site_begin, array)`` with raw likelihoods [n][I][3] (float64) or reader genotypes
        [n][I] (int8: -1 missing, 0, 1, 2)."""
        pos_dist = np.ascontiguousarray(pos_dist, dtype=np.float64)
        self._check(self.lib.nghmm_load_begin(self._h, _dp(pos_dist)))
        for s0, a in chunks:
            if a.dtype == np.int8:
                a = np.ascontiguousarray(a)
                self._check(self.lib.nghmm_load_geno_sites(
                    self._h, int(s0), a.shape[0], a.ctypes.data_as(C.POINTER(C.c_int8))))
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
                self._check(self.lib.nghmm_load_gl_raw_sites(
                    self._h, int(s0), a.shape[0], _dp(a), int(space), int(call_geno),
                    int(check_nan)))
        self._check(self.lib.nghmm_load_end(self._h))

    def load_chunks_device(self, pos_ptr, chunks, space=0, call_geno=False):
        """The same from device buffers: ``chunks`` yields (site_begin, n_sites, data_ptr) of
        raw likelihoods [n][I][3]."""
        self._check(self.lib.nghmm_load_begin_dev(self._h, C.c_void_p(pos_ptr)))
        for s0, n, ptr in chunks:
            self._check(self.lib.nghmm_load_gl_raw_sites_dev(self._h, int(s0), int(n),
                                                             C.c_void_p(ptr), int(space),
                                                             int(call_geno), 0))
        self._check(self.lib.nghmm_load_end(self._h))

    def load_device(self, gl_ptr, pos_ptr):
        """Same as load() from raw device pointers (e.g. torch tensors' data_ptr())."""
        self._check(self.lib.nghmm_load_gl_device(self._h, C.c_void_p(gl_ptr), C.c_void_p(pos_ptr)))

    def set_params(self, indF=None, alpha=None, freq=None):
        def prep(a, n):
            if a is None:
                return None
            return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))
        a, b, c = prep(indF, self.n_ind), prep(alpha, self.n_ind), prep(freq, self.n_sites)
        self._check(self.lib.nghmm_set_params(self._h, _dp(a) if a is not None else None,
                                              _dp(b) if b is not None else None,
                                              _dp(c) if c is not None else None))

    def _get(self, which):
        out = np.empty(self.n_sites if which == 2 else self.n_ind)
        args = [None, None, None]
        args[which] = _dp(out)
        self._check(self.lib.nghmm_get_params(self._h, *args))
        return out

    @property
    def indF(self):
        return self._get(0)

    @property
    def alpha(self):
        return self._get(1)

    @property
    def freq(self):
        return self._get(2)

    @property
    def marg_prob(self):
        """[I][S] posterior of the IBD state (marg_prob[i][s][1]) of the last E-step."""
        out = np.empty((self.n_ind, self.n_sites))
        self._check(self.lib.nghmm_get_posteriors(self._h, _dp(out)))
        return out

    @property
    def e_prob(self):
        """[I][S][2] log emission probabilities."""
        out = np.empty((self.n_ind, self.n_sites, 2))
        self._check(self.lib.nghmm_get_emissions(self._h, _dp(out)))
        return out

    # -- the hot path ------------------------------------------------------
    def init_emission(self):
        """parse_args.cpp:372-387."""
        self._check(self.lib.nghmm_emission(self._h))

    def estep(self):
        """EM.cpp:147-185; returns ind_lkl."""
        self._check(self.lib.nghmm_estep(self._h, _dp(self.ind_lkl)))
        return self.ind_lkl

    def lkl(self, ind, F, alpha):
        """Forward log-likelihood of (individual, F, alpha) points (EM.cpp:449-464 negated)."""
        ind = np.ascontiguousarray(ind, dtype=np.uint32)
        F = np.ascontiguousarray(F, dtype=np.float64)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        out = np.empty(len(ind))
        self._check(self.lib.nghmm_lkl_batch(self._h, len(ind),
                                             ind.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(F),
                                             _dp(alpha), _dp(out)))
        return out

    def mstep_indf(self, indF_fixed=False, alpha_fixed=False):
        st = MstepStats()
        self._check(self.lib.nghmm_mstep_indf(self._h, int(indF_fixed), int(alpha_fixed),
                                              C.byref(st)))
        self.last_stats = st
        return st

    def mstep_freq(self, freq_est=1):
        self._check(self.lib.nghmm_mstep_freq(self._h, int(freq_est)))

    def layout(self):
        """(waves per individual, sites per lane) of the fast-mode site layout; (0, 0) in
        exact mode."""
        c, t = C.c_uint32(0), C.c_uint64(0)
        self._check(self.lib.nghmm_fast_layout(self._h, C.byref(c), C.byref(t)))
        return int(c.value), int(t.value)

    def estep_mstep(self, indF_fixed=False, alpha_fixed=False, after_estep=None):
        """E-step and indF/alpha M-step of one iteration in one call (nghmm_estep_mstep);
        ``after_estep()`` runs as soon as the posteriors are final.  An exception raised
        in it is re-raised here after the call returns."""
        st = MstepStats()
        err = []

        def _hook(_user):
            try:
                after_estep()
            except BaseException as e:      # must not propagate through the C frame
                err.append(e)

        cb = HOOK_FN(_hook) if after_estep is not None else C.cast(None, HOOK_FN)
        rc = self.lib.nghmm_estep_mstep(self._h, int(indF_fixed), int(alpha_fixed),
                                        _dp(self.ind_lkl), C.byref(st), cb, None)
        if err:
            raise err[0]
        self._check(rc)
        self.last_stats = st
        return st

    def iter_EM(self, freq_est=1, indF_fixed=False, alpha_fixed=False):
        """One EM iteration (EM.cpp:139-289)."""
        st = MstepStats()
        self._check(self.lib.nghmm_iter_em(self._h, int(freq_est), int(indF_fixed),
                                           int(alpha_fixed), _dp(self.ind_lkl), C.byref(st)))
        self.last_stats = st
        return st

    def EM(self, freq_est=1, indF_fixed=False, alpha_fixed=False, min_iters=10, max_iters=100,
           min_epsilon=1e-5, callback=None):
        """The iteration loop and convergence test of EM.cpp:27-103 (host control only).
        Returns the number of iterations run."""
        it = 0
        max_lkl_epsilon = -math.inf
        prev_ind_lkl = np.full(self.n_ind, -math.inf)
        while ((self.prev_tot_lkl - self.tot_lkl > min_epsilon or max_lkl_epsilon > min_epsilon
                or it < min_iters) and it < max_iters):
            it += 1
            self.iter_EM(freq_est, indF_fixed, alpha_fixed)
            self.prev_tot_lkl = self.tot_lkl
            tot = 0.0
            for v in self.ind_lkl:          # EM.cpp:77-79: summation in individual order
                tot += float(v)
            self.tot_lkl = tot
            with np.errstate(invalid="ignore", divide="ignore"):
                eps = (self.ind_lkl - prev_ind_lkl) / np.abs(prev_ind_lkl)
            # array_max_pos (gen_func.cpp:73-84): strict '>' from -inf, NaN never wins
            best, mx = 0, -math.inf
            for i, v in enumerate(eps):
                if v > mx:
                    best, mx = i, v
            max_lkl_epsilon = float(eps[best])
            prev_ind_lkl = self.ind_lkl.copy()
            if callback:
                callback(it, self)
        self.iterations = it
        return it

    # -- site shards (include/nghmm.h, "shard the SITES") ----------------------
    def site_shard_bytes(self):
        return int(self.lib.nghmm_site_shard_bytes(self._h))

    def site_shard_setup(self, rank, world, send_ptr, recv_ptr, nbytes, allgather):
        """This handle's sites are range `rank` of `world`; ``allgather(n_bytes)`` gathers the
        first n_bytes of the send buffer of every range into the receive buffer, ordered on
        the handle's stream (nghmm_site_shard_setup).  An exception raised in it makes the
        library call that needed it fail; it is re-raised by _check."""
        self._shard_err = []

        def _cb(_user, n):
            try:
                allgather(int(n))
                return 0
            except BaseException as e:      # must not propagate through the C frame
                self._shard_err.append(e)
                return 1

        self._shard_cb = ALLGATHER_FN(_cb) if world > 1 else C.cast(None, ALLGATHER_FN)
        self._check(self.lib.nghmm_site_shard_setup(self._h, int(rank), int(world), C.c_void_p(send_ptr),
                                                    C.c_void_p(recv_ptr), int(nbytes), self._shard_cb,
                                                    None))

    def viterbi_shard_forward(self, scores_in=None):
        """Forward half of the decoding over a chain of site shards: scores_in = what the range
        before ended with ([I][2]; None on the first range); returns this range's."""
        out = np.empty((self.n_ind, 2))
        if scores_in is not None:
            scores_in = np.ascontiguousarray(scores_in, dtype=np.float64).reshape(self.n_ind, 2)
        self._check(self.lib.nghmm_viterbi_shard_forward(
            self._h, _dp(scores_in) if scores_in is not None else None, _dp(out)))
        return out

    def viterbi_shard_back(self, state_after=None):
        """Backward half: state_after = the state the range after found for this range's last
        site ([I]; None on the last range); returns (state at the site in front of this range's
        first [I], path [I][n_sites])."""
        u8p = C.POINTER(C.c_uint8)
        before = np.empty(self.n_ind, dtype=np.uint8)
        path = np.empty((self.n_ind, self.n_sites), dtype=np.uint8)
        if state_after is not None:
            state_after = np.ascontiguousarray(state_after, dtype=np.uint8).reshape(self.n_ind)
        self._check(self.lib.nghmm_viterbi_shard_back(
            self._h, state_after.ctypes.data_as(u8p) if state_after is not None else None,
            before.ctypes.data_as(u8p), path.ctypes.data_as(u8p)))
        return before, path

    def viterbi(self):
        """[I][S] most probable IBD path (EM.cpp:105-116)."""
        path = np.empty((self.n_ind, self.n_sites), dtype=np.uint8)
        self._check(self.lib.nghmm_viterbi(self._h, path.ctypes.data_as(C.POINTER(C.c_uint8))))
        return path

    def ibd_tracts(self, source="viterbi", threshold=0.5, min_sites=1):
        """IBD tracts called on the device (nghmm_ibd_tracts): maximal runs of the IBD state
        within one chromosome, from the last Viterbi decode ("viterbi") or from posteriors
        >= threshold ("posterior").  Structured array with fields ind, first_site, n_sites,
        post_sum, post_mean, ordered by (ind, first_site)."""
        return _tracts(lambda *a: self.lib.nghmm_ibd_tracts(self._h, *a), self._check, source,
                       threshold, min_sites)

    def sample_paths(self, n_draws, seed=0, keep=0):
        """n_draws IBD paths per individual drawn from the joint posterior P(z | data, theta) at
        the current parameters (nghmm_sample_paths).  Returns (stats, paths): a structured array
        [n_draws][I] of PATH_STATS_DTYPE and the first `keep` draws as uint8 [keep][I][S].  Draw d
        depends on (seed, d) alone."""
        return _sample_paths(lambda *a: self.lib.nghmm_sample_paths(self._h, *a), self._check,
                             self.n_ind, self.n_sites, n_draws, seed, keep)

    def tract_support(self, tracts):
        """How far to trust each of `tracts` (nghmm_tract_support): the log of the joint posterior
        probability that the individual is IBD at every site of the range (log_p_ibd), that it is
        non-IBD at every site (log_p_non), their log-odds to base 10 (lod), the smallest per-site
        posterior in the range and the lowest site that has it -- at the CURRENT parameters.
        tracts: what ibd_tracts returns, or integers [n][3] of (ind, first_site, n_sites), ordered
        by (ind, first_site) and disjoint within an individual.  A structured array [n] of
        TRACT_SCORE_DTYPE, aligned with the input."""
        return _tract_support(lambda *a: self.lib.nghmm_tract_support(self._h, *a), self._check, tracts)

    def tract_bounds(self, tracts, anchors=None, levels=(0.975, 0.5, 0.025)):
        """Where each of `tracts` really starts and ends (nghmm_tract_bounds), at the CURRENT
        parameters.  Given that the individual is IBD at a record's anchor (anchors[k], or with
        anchors None / NO_ANCHOR the site of the range least likely to be non-IBD), G(s) is the
        probability that the IBD run through the anchor reaches down to at least site s and H(s)
        that it reaches up to s.  Returns (bounds, start, end): bounds, a structured array [n] of
        TRACT_BOUND_DTYPE (anchor, the limits of the two searches -- the chromosome's edge or the
        neighbouring record's anchor --, post_anchor, and the reach to either limit: towards a
        neighbour's anchor the probability that the two tracts are one); start / end, uint64
        [n][len(levels)]: the lowest site with G >= level and the highest with H >= level, so that
        start[:, 2] .. start[:, 0] with the default levels is the 95 % interval of the start with
        its median in between, and end[:, 0] .. end[:, 2] that of the end.  levels: at most 8, in
        (0, 1), strictly descending.  tracts as for tract_support."""
        return _tract_bounds(lambda *a: self.lib.nghmm_tract_bounds(self._h, *a), self._check, tracts,
                             anchors, levels)

    def freq_info(self, levels=(), cavity=False):
        """Per site the log-likelihood of the whole cohort as a function of that site's allele
        frequency alone, at the CURRENT indF, alpha and freq (nghmm_freq_info).  Returns (stats,
        curve), or with cavity=True (stats, curve, cavity): stats, a structured array [S] of
        FREQ_STAT_DTYPE (freq, the leave-one-site-out log-likelihood ll of the site's data, its
        derivative score and minus its second derivative info at freq); curve [S][len(levels)],
        the log-likelihood at every level minus the one at freq (levels: at most 8, in [0, 1]; at
        0 or 1, -2 curve is a likelihood-ratio statistic against a monomorphic site); cavity
        [I][S], P(IBD at the site | all data of the individual except the site's).
        freq_std_errors turns the records into standard errors."""
        return _freq_info(lambda *a: self.lib.nghmm_freq_info(self._h, *a), self._check, self.n_ind,
                          self.n_sites, levels, cavity)

    def geno_smooth(self, regions=None, sites=True, post=False, call=False):
        """Genotype posteriors under the HMM, at the CURRENT indF, alpha and freq (nghmm_geno_smooth):
        per cell P(genotype | all data of the individual), the IBD state of the site summed out
        exactly.  Returns a dict of the arrays asked for: "regions" [I][R] of
        GENO_REGION_STAT_DTYPE (het, het_prior, non_ibd, dosage summed over the sites of every
        region; regions as ibd_summary takes them), "sites" [S] of GENO_SITE_STAT_DTYPE (n0, n1, n2,
        het_prior, ibd, alt_ibd summed over the individuals), "post" [S][I][3] and "call" [S][I]
        uint8 (3: no posterior).  geno_em_freq and het_outside_ibd turn the records into the exact
        EM update of the frequencies and the heterozygosity outside IBD.  Conditional on indF,
        alpha and the frequencies."""
        return _geno_smooth(lambda *a: self.lib.nghmm_geno_smooth(self._h, *a), self._check, self.n_ind,
                            self.n_sites, regions, sites, post, call)

    def obs_info(self, indF=None, alpha=None):
        """Per individual the log-likelihood, its gradient and its Hessian in (indF, alpha) under
        the current emissions, from exact derivatives (nghmm_obs_info): a structured array [I] of
        INFO_DTYPE.  indF / alpha: the points ([I] or a scalar each); neither: the current
        parameters.  The allele frequencies are held fixed; std_errors turns the records into
        standard errors."""
        return _obs_info(lambda *a: self.lib.nghmm_obs_info(self._h, *a), self._check, self.n_ind,
                         indF, alpha)

    def ibd_summary(self, regions=None, what=("viterbi", "posterior"), threshold=0.5, sites=True):
        """IBD per region and per site, reduced on the device (nghmm_ibd_summary).  regions: [R][2]
        integer array of half-open site ranges (begin, end), sorted and disjoint
        (chromosome_regions, window_regions); what: "viterbi" (the last decode), "posterior"
        (>= threshold) or both.  Returns (region_stats, site_stats): structured arrays [I][R] of
        REGION_STAT_DTYPE and [S] of SITE_STAT_DTYPE; None for the one not asked for (no regions,
        sites=False).  The fields of a source that was not asked for are 0."""
        return _ibd_summary(lambda *a: self.lib.nghmm_ibd_summary(self._h, *a), self._check,
                            self.n_ind, self.n_sites, regions, what, threshold, sites)

    def ibd_expect(self, regions=None, sites=True, viterbi=False):
        """Exact expectations over IBD paths (nghmm_ibd_expect): (region_stats, site_stats), the
        first [I][R] of EXPECT_REGION_DTYPE (ibd, starts, switches, ibd_mb, entropy, log_p_path;
        regions as ibd_summary takes them, None = one region over all sites), the second [S] of
        EXPECT_SITE_DTYPE (on, off, ibd, entropy; None unless sites).  viterbi: also the log
        posterior probability of the last decoded path (log_p_path, else 0)."""
        return _ibd_expect(lambda *a: self.lib.nghmm_ibd_expect(self._h, *a), self._check,
                           self.n_ind, self.n_sites, regions, sites, viterbi)

    def ibd_moments(self, regions=None, length="sites"):
        """Exact posterior means and covariances of (IBD length, number of tracts) per individual
        and region (nghmm_ibd_moments): [I][R] of MOMENT_REGION_DTYPE (mean_a, mean_t, var_a,
        cov_at, var_t; regions as ibd_summary takes them, None = one region over all sites).
        length: "sites" (A = IBD sites) or "mb" (A = IBD Mb).  Conditional on indF, alpha and the
        frequencies; moment_sd turns the records into standard deviations."""
        return _ibd_moments(lambda *a: self.lib.nghmm_ibd_moments(self._h, *a), self._check,
                            self.n_ind, self.n_sites, regions, length)

    def ibd_by_length(self, min_len, unit="sites", regions=None):
        """Expected IBD above a minimum tract length, exactly (nghmm_ibd_by_length): [I][R][K] of
        BYLENGTH_DTYPE -- tracts, the expected number of IBD tracts of at least min_len[k] that
        begin in the region, and length, their expected total length.  min_len: 1 to 8 strictly
        increasing thresholds in sites (whole numbers >= 1) or, with unit="mb", in Mb (>= 0; a
        tract's Mb run from its first site to its last); regions as ibd_summary takes them, None
        = one region over all sites.  by_length_classes turns the records into length classes."""
        return _ibd_by_length(lambda *a: self.lib.nghmm_ibd_by_length(self._h, *a), self._check,
                              self.n_ind, self.n_sites, min_len, unit, regions)

    def ibd_longest(self, min_len, unit="sites", regions=None):
        """The distribution of the longest IBD run, exactly (nghmm_ibd_longest): [I][R][K] of
        LONGEST_DTYPE -- p_any, the probability that some IBD run of the region is of at least
        min_len[k], and p_none, that none is (from its own sum).  min_len, unit and regions as
        ibd_by_length takes them; a run is cut at chromosome starts and at the region's edges.
        longest_classes turns the records into the classes of the longest run."""
        return _ibd_by_length(lambda *a: self.lib.nghmm_ibd_longest(self._h, *a), self._check,
                              self.n_ind, self.n_sites, min_len, unit, regions, LONGEST_DTYPE,
                              "ibd_longest", LONGEST_MB)

    def ibd_count(self, min_len, unit="sites", regions=None, max_count=8):
        """The distribution of the number of long IBD runs, exactly (nghmm_ibd_count): a float64
        array [I][R][K][max_count + 1] -- per individual, region and threshold the probabilities
        that exactly 0, 1, .., max_count - 1 IBD runs of the region are of at least min_len[k]
        (sites, or Mb with unit="mb"), and last that max_count or more are; each from its own sum.
        Arguments as ibd_longest; 1 <= max_count <= 16.  count_summary gives mean, mode and
        quantiles."""
        u64p = C.POINTER(C.c_uint64)
        L, reg = _by_length_args(self.n_sites, min_len, unit, regions, "ibd_count")
        if isinstance(max_count, bool) or not isinstance(max_count, (int, np.integer)) or \
                not 0 <= int(max_count) < 2 ** 32:
            raise NgsFHMMError(-10, "ibd_count: max_count is a whole number from 1 to 16")
        R, K, M = len(reg), len(L), int(max_count)
        begin, end = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
        prob = np.zeros((self.n_ind, R, K, M + 1))
        self._check(self.lib.nghmm_ibd_count(self._h, COUNT_MB if unit == "mb" else 0, K, _dp(L) if K else None,
                                             M, R, begin.ctypes.data_as(u64p) if R else None,
                                             end.ctypes.data_as(u64p) if R else None,
                                             _dp(prob) if R and K else None))
        return prob

    def ibd_long_moments(self, min_len, unit="sites", regions=None):
        """Exact posterior mean and covariance of (total length, number) of the long IBD runs
        (nghmm_ibd_long_moments): [I][R][K] of LONG_MOMENT_DTYPE -- mean_a and var_a of the sites
        (Mb with unit="mb") of the region inside IBD runs of at least min_len[k], mean_t and var_t
        of the number of such runs, and cov_at.  min_len, unit and regions as ibd_count takes them;
        a run is cut at chromosome starts and at the region's edges.  Conditional on indF, alpha
        and the frequencies; long_moment_sd turns the records into standard deviations and the
        share of a region."""
        return _ibd_by_length(lambda *a: self.lib.nghmm_ibd_long_moments(self._h, *a), self._check,
                              self.n_ind, self.n_sites, min_len, unit, regions, LONG_MOMENT_DTYPE,
                              "ibd_long_moments", LONG_MOMENTS_MB)

    def ibd_long(self, min_len, unit="sites", regions=None, sites=True, post=False, threshold=0.5):
        """The posterior of every site of lying in an IBD tract of at least min_len[k], exactly
        (nghmm_ibd_long).  min_len and unit as ibd_by_length takes them.  Returns a dict of the
        arrays asked for: "regions" [I][R][K] of LONG_REGION_DTYPE -- sites and mb, the expected
        sites and Mb of the region inside such tracts (regions as ibd_summary takes them, None =
        one region over all sites, False = none); "sites" [S][K] of LONG_SITE_DTYPE -- sum over
        the individuals and the count of those at or above threshold (sites=True); "post"
        [K][I][S], each plane like marg_prob (post=True).  long_tracts calls tracts from a plane."""
        return _ibd_long(lambda *a: self.lib.nghmm_ibd_long(self._h, *a), self._check, self.n_ind,
                         self.n_sites, min_len, unit, regions, sites, post, threshold)

    def by_length_qmax(self):
        """The largest |Q| the last ibd_by_length met (nghmm_debug_bylength_qmax): times 2^-53 the
        absolute error in the exponent of a window's probability."""
        q = C.c_double(0.0)
        self._check(self.lib.nghmm_debug_bylength_qmax(self._h, C.byref(q)))
        return q.value

    def ibd_sharing(self, what=("viterbi", "posterior"), threshold=0.5, site_begin=0, site_end=None):
        """Pairwise IBD sharing over the sites [site_begin, site_end) (default: all), reduced on
        the matrix cores (nghmm_ibd_sharing).  what: "viterbi" (vit_both, from the last decode),
        "posterior" (post_both at >= threshold, and post_prod), or single outputs by name.
        Returns a dict of the [I][I] arrays that were asked for: vit_both and post_both uint64,
        post_prod float64; full, symmetric, the diagonal included."""
        return _ibd_sharing(lambda *a: self.lib.nghmm_ibd_sharing(self._h, *a), self._check,
                            self.n_ind, self.n_sites, what, threshold, site_begin, site_end)

    # -- measurement -------------------------------------------------------
    def kernel_ms(self, name):
        """(milliseconds, launches) of a kernel family in the last call that ran it.  Fast mode's
        M-step and fused iteration time their kernels only after ``set_switch("spans", 1)`` (the
        events cost 0.05 ms per iteration) and report 0 without it; include/nghmm.h."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self.lib.nghmm_kernel_ms(self._h, KERNEL_SLOTS[name], C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def synchronize(self):
        self._check(self.lib.nghmm_synchronize(self._h))

    @staticmethod
    def mode_name(mode):
        """A loop-body version of the objective kernels as debug_modes prints it: 2F2As2 = two F
        probes, two alpha probes, small-alpha (kappa) form, degree-2 alpha probes."""
        if mode == 0xffffffff:
            return "rounds_of_mixed_versions"
        if mode == 0:
            return "general"
        return (f"{(mode >> 2) & 3}F{mode & 3}A" + ("s" if mode & 0x200 else "") +
                ("2" if mode & 0x400 else "") + ("e" if mode & 0x800 else ""))

    def mode_counts(self, reset=False):
        """{kernel version: individual-rounds it evaluated} of the objective rounds so far
        (nghmm_debug_mode_counts)."""
        buf = (ModeCount * 160)()
        n = C.c_uint32(0)
        self._check(self.lib.nghmm_debug_mode_counts(self._h, buf, 160, C.byref(n), int(reset)))
        return {self.mode_name(buf[k].mode): int(buf[k].ind_rounds) for k in range(min(n.value, 160))}

    def estmaf_counts(self, reset=False):
        """Sites of the allele-frequency step that left its common route (nghmm_debug_estmaf_counts)."""
        v = (C.c_uint64 * 5)()
        self._check(self.lib.nghmm_debug_estmaf_counts(self._h, v, int(reset)))
        return {"check_failed": int(v[0]), "second_interval": int(v[1]), "third_interval": int(v[2]),
                "log_space": int(v[3]), "exact_tail": int(v[4])}


class Group:
    """n handles of one process as one cohort (nghmm_group_setup / nghmm_group_iter_em): handle
    r holds the individuals [r I, (r+1) I) for all sites."""

    def __init__(self, handles):
        self.handles = list(handles)
        self.lib = self.handles[0].lib
        n = len(self.handles)
        self._arr = (C.c_void_p * n)(*[h._h for h in self.handles])
        self.handles[0]._check(self.lib.nghmm_group_setup(self._arr, n))
        self.ind_lkl = np.full(n * self.handles[0].n_ind, -math.inf)

    def _members_open(self):
        # the group keeps its members alive; one that was closed by hand leaves a dangling
        # pointer in the array the library is given
        if any(h.closed for h in self.handles):
            raise NgsFHMMError(-10, "a member of this group has been closed")

    def mstep_freq(self, freq_est=1):
        self._members_open()
        self.handles[0]._check(self.lib.nghmm_group_mstep_freq(self._arr, len(self.handles),
                                                               int(freq_est)))

    def iter_EM(self, freq_est=1, indF_fixed=False, alpha_fixed=False):
        self._members_open()
        st = MstepStats()
        self.handles[0]._check(self.lib.nghmm_group_iter_em(
            self._arr, len(self.handles), int(freq_est), int(indF_fixed), int(alpha_fixed),
            _dp(self.ind_lkl), C.byref(st)))
        return st


class Chain:
    """n fast-mode handles of one process as one data set cut along the SITE axis
    (nghmm_chain_setup / nghmm_chain_iter_em): handle r holds all individuals for the r-th
    site range; log-likelihoods, indF and alpha are the chain's and equal on every handle."""

    def __init__(self, handles):
        self.handles = list(handles)
        self.lib = self.handles[0].lib
        n = len(self.handles)
        self._arr = (C.c_void_p * n)(*[h._h for h in self.handles])
        self.handles[0]._check(self.lib.nghmm_chain_setup(self._arr, n))
        self.n_ind = self.handles[0].n_ind
        self.n_sites = sum(h.n_sites for h in self.handles)
        self.ind_lkl = np.full(self.n_ind, -math.inf)

    def _members_open(self):
        if any(h.closed for h in self.handles):
            raise NgsFHMMError(-10, "a member of this chain has been closed")

    def mstep_freq(self, freq_est=1):
        self._members_open()
        self.handles[0]._check(self.lib.nghmm_chain_mstep_freq(self._arr, len(self.handles),
                                                               int(freq_est)))

    def iter_EM(self, freq_est=1, indF_fixed=False, alpha_fixed=False):
        self._members_open()
        st = MstepStats()
        self.handles[0]._check(self.lib.nghmm_chain_iter_em(
            self._arr, len(self.handles), int(freq_est), int(indF_fixed), int(alpha_fixed),
            _dp(self.ind_lkl), C.byref(st)))
        return st

    def viterbi(self):
        self._members_open()
        path = np.empty((self.n_ind, self.n_sites), dtype=np.uint8)
        self.handles[0]._check(self.lib.nghmm_chain_viterbi(
            self._arr, len(self.handles), path.ctypes.data_as(C.POINTER(C.c_uint8))))
        return path

    def ibd_tracts(self, source="viterbi", threshold=0.5, min_sites=1):
        """NgsFHMM.ibd_tracts over the chain (nghmm_chain_ibd_tracts): global site indices, a
        tract across a shard boundary joined into one, min_sites applied after joining."""
        self._members_open()
        return _tracts(lambda *a: self.lib.nghmm_chain_ibd_tracts(self._arr, len(self.handles), *a),
                       self.handles[0]._check, source, threshold, min_sites)

    def sample_paths(self, n_draws, seed=0, keep=0):
        """NgsFHMM.sample_paths over the chain (nghmm_chain_sample_paths): the single handle's
        draws, global site indices."""
        self._members_open()
        return _sample_paths(
            lambda *a: self.lib.nghmm_chain_sample_paths(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, n_draws, seed, keep)

    def tract_support(self, tracts):
        """NgsFHMM.tract_support over the chain (nghmm_chain_tract_support): global site indices,
        a range across a shard boundary is one range."""
        self._members_open()
        return _tract_support(
            lambda *a: self.lib.nghmm_chain_tract_support(self._arr, len(self.handles), *a),
            self.handles[0]._check, tracts)

    def tract_bounds(self, tracts, anchors=None, levels=(0.975, 0.5, 0.025)):
        """NgsFHMM.tract_bounds over the chain (nghmm_chain_tract_bounds): global site indices, a
        search across a shard boundary is one search."""
        self._members_open()
        return _tract_bounds(
            lambda *a: self.lib.nghmm_chain_tract_bounds(self._arr, len(self.handles), *a),
            self.handles[0]._check, tracts, anchors, levels)

    def freq_info(self, levels=(), cavity=False):
        """NgsFHMM.freq_info over the chain (nghmm_chain_freq_info): global site order."""
        self._members_open()
        return _freq_info(lambda *a: self.lib.nghmm_chain_freq_info(self._arr, len(self.handles), *a),
                          self.handles[0]._check, self.n_ind, self.n_sites, levels, cavity)

    def geno_smooth(self, regions=None, sites=True, post=False, call=False):
        """NgsFHMM.geno_smooth over the chain (nghmm_chain_geno_smooth): global site indices, a
        region across a shard boundary is one region."""
        self._members_open()
        return _geno_smooth(lambda *a: self.lib.nghmm_chain_geno_smooth(self._arr, len(self.handles), *a),
                            self.handles[0]._check, self.n_ind, self.n_sites, regions, sites, post, call)

    def obs_info(self, indF=None, alpha=None):
        """NgsFHMM.obs_info over the chain (nghmm_chain_obs_info)."""
        self._members_open()
        return _obs_info(lambda *a: self.lib.nghmm_chain_obs_info(self._arr, len(self.handles), *a),
                         self.handles[0]._check, self.n_ind, indF, alpha)

    def ibd_summary(self, regions=None, what=("viterbi", "posterior"), threshold=0.5, sites=True):
        """NgsFHMM.ibd_summary over the chain (nghmm_chain_ibd_summary): global site indices, a
        region across a shard boundary is one region."""
        self._members_open()
        return _ibd_summary(
            lambda *a: self.lib.nghmm_chain_ibd_summary(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, regions, what, threshold, sites)

    def ibd_expect(self, regions=None, sites=True, viterbi=False):
        """NgsFHMM.ibd_expect over the chain (nghmm_chain_ibd_expect): global site indices, a region
        across a shard boundary is one region; within rounding of a single handle's values."""
        self._members_open()
        return _ibd_expect(
            lambda *a: self.lib.nghmm_chain_ibd_expect(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, regions, sites, viterbi)

    def ibd_moments(self, regions=None, length="sites"):
        """NgsFHMM.ibd_moments over the chain (nghmm_chain_ibd_moments): global site indices, a
        region across a shard boundary is one region; within rounding of a single handle's values."""
        self._members_open()
        return _ibd_moments(
            lambda *a: self.lib.nghmm_chain_ibd_moments(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, regions, length)

    def ibd_by_length(self, min_len, unit="sites", regions=None):
        """NgsFHMM.ibd_by_length over the chain (nghmm_chain_ibd_by_length): global site indices, a
        region across a shard boundary is one region, a window may reach into the next shard but
        not past it; within rounding of a single handle's values."""
        self._members_open()
        return _ibd_by_length(
            lambda *a: self.lib.nghmm_chain_ibd_by_length(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, min_len, unit, regions)

    def ibd_long(self, min_len, unit="sites", regions=None, sites=True, post=False, threshold=0.5):
        """NgsFHMM.ibd_long over the chain (nghmm_chain_ibd_long): global site indices, a region
        across a shard boundary is one region, a window may reach into the neighbouring shard on
        either side but not past it; within rounding of a single handle's values."""
        self._members_open()
        return _ibd_long(lambda *a: self.lib.nghmm_chain_ibd_long(self._arr, len(self.handles), *a),
                         self.handles[0]._check, self.n_ind, self.n_sites, min_len, unit, regions,
                         sites, post, threshold)

    def ibd_longest(self, min_len, unit="sites", regions=None):
        """NgsFHMM.ibd_longest over the chain (nghmm_chain_ibd_longest): global site indices; the
        lane state crosses the cuts, so the records are the single handle's bytes and a threshold
        may reach past any number of shards."""
        self._members_open()
        return _ibd_by_length(
            lambda *a: self.lib.nghmm_chain_ibd_longest(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, min_len, unit, regions, LONGEST_DTYPE,
            "ibd_longest", LONGEST_MB)

    def ibd_sharing(self, what=("viterbi", "posterior"), threshold=0.5, site_begin=0, site_end=None):
        """NgsFHMM.ibd_sharing over the chain (nghmm_chain_ibd_sharing): global site indices, the
        shards' matrices added in rank order."""
        self._members_open()
        return _ibd_sharing(
            lambda *a: self.lib.nghmm_chain_ibd_sharing(self._arr, len(self.handles), *a),
            self.handles[0]._check, self.n_ind, self.n_sites, what, threshold, site_begin, site_end)

    @property
    def freq(self):
        return np.concatenate([h.freq for h in self.handles])

    @property
    def marg_prob(self):
        return np.concatenate([h.marg_prob for h in self.handles], axis=1)
