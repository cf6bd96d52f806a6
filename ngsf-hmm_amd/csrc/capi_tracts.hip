// capi_tracts.hip -- IBD tracts of one handle (nghmm_ibd_tracts; the chain's merge is in
// capi_multi.hip): count, scan, emit, finish and -- with min_sites > 1 -- compaction on the
// device (kernels_tracts.hip), the records copied out once.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_internal.hpp"

static_assert(sizeof(nghmm_tract) == sizeof(TractRec) &&
                  offsetof(nghmm_tract, n_sites) == offsetof(TractRec, n_sites) &&
                  offsetof(nghmm_tract, ind) == offsetof(TractRec, ind) &&
                  offsetof(nghmm_tract, post_sum) == offsetof(TractRec, post_sum),
              "the device records are nghmm_tract");
static_assert(NGHMM_TRACTS_VITERBI == TRACTS_SRC_VITERBI &&
                  NGHMM_TRACTS_POSTERIOR == TRACTS_SRC_POSTERIOR,
              "tract sources");

namespace capi {

int tracts_check_args(nghmm_t* h, int source, double threshold, const char* who) {
  if (!h || !h->loaded) {
    set_error("%s: the handle holds no data", who);
    return NGHMM_ERR_ARG;
  }
  if (source == NGHMM_TRACTS_VITERBI) {
    if (!h->path_decoded) {
      set_error("%s: no Viterbi decode since the data were loaded (run nghmm_viterbi first)", who);
      return NGHMM_ERR_ARG;
    }
  } else if (source == NGHMM_TRACTS_POSTERIOR) {
    if (!(threshold > 0.0 && threshold <= 1.0)) {
      set_error("%s: the posterior threshold %g is not in (0, 1]", who, threshold);
      return NGHMM_ERR_ARG;
    }
  } else {
    set_error("%s: unknown source %d (NGHMM_TRACTS_VITERBI or NGHMM_TRACTS_POSTERIOR)", who, source);
    return NGHMM_ERR_ARG;
  }
  return NGHMM_OK;
}

namespace {

// The passes on the handle's stream; *d_out = the records on the device, *n_out = their number.
// Arguments checked by the caller.
int tracts_device(nghmm_t* h, int source, double thr, uint64_t min_sites, const TractRec** d_out,
                  uint64_t* n_out) {
  int rc;
  if ((rc = use_device(h))) return rc;
  // fast mode: the site-major copy of the tile-major posteriors (kept until the next E-step;
  // the .ibd writer has made it already)
  if ((rc = ensure_marg(h))) return rc;
  const uint64_t S = h->S, I = h->I, nseg = tract_segments(S), nb = I * nseg, nblk = (S + 15) / 16;
  const uint64_t scr = tract_scan_scratch(nb);
  // d_tseg: offsets [nb + 1] | scan scratch | carried sums [nb] | chromosome-start mask [nblk]
  if ((rc = h->d_tseg.reserve((nb + 1 + scr) * 8 + nb * 8 + nblk * 4))) return rc;
  uint64_t* off = reinterpret_cast<uint64_t*>(h->d_tseg.p);
  uint64_t* scratch = off + nb + 1;
  double* carry = reinterpret_cast<double*>(scratch + scr);
  uint32_t* mask = reinterpret_cast<uint32_t*>(carry + nb);
  const uint8_t* path = source == NGHMM_TRACTS_VITERBI ? h->d_path_sites : nullptr;
  launch_tract_chrom_mask(h->stream, h->d_pos, S, mask);
  launch_tract_count(h->stream, source, path, h->d_marg, thr, mask, S, I, off);
  launch_tract_scan(h->stream, off, nb, scratch);
  HIP_TRY(hipGetLastError());
  uint64_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, off + nb, sizeof n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));
  // d_trec: records [n] | (min_sites > 1:) compacted records [n] | their offsets [n + 1] | scratch
  const bool filter = min_sites > 1;
  const uint64_t kscr = filter ? tract_scan_scratch(n) : 0;
  const size_t bytes = n * sizeof(TractRec) + (filter ? n * sizeof(TractRec) + (n + 1 + kscr) * 8 : 0);
  if ((rc = h->d_trec.reserve(bytes))) return rc;
  TractRec* rec = reinterpret_cast<TractRec*>(h->d_trec.p);
  *d_out = rec;
  *n_out = n;
  if (n == 0) return NGHMM_OK;
  launch_tract_emit(h->stream, source, path, h->d_marg, thr, mask, S, I, off, rec, carry);
  if (!filter) {
    launch_tract_finish(h->stream, rec, n, carry, S, min_sites, nullptr);
    HIP_TRY(hipGetLastError());
    return NGHMM_OK;
  }
  TractRec* out = rec + n;
  uint64_t* keep = reinterpret_cast<uint64_t*>(out + n);
  launch_tract_finish(h->stream, rec, n, carry, S, min_sites, keep);
  launch_tract_scan(h->stream, keep, n, keep + n + 1);
  launch_tract_compact(h->stream, rec, n, min_sites, keep, out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(n_out, keep + n, sizeof *n_out, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));
  *d_out = out;
  return NGHMM_OK;
}

}  // namespace

int tracts_to_host(nghmm_t* h, int source, double threshold, uint64_t min_sites,
                   std::vector<nghmm_tract>& out) {
  const TractRec* d = nullptr;
  uint64_t n = 0;
  int rc;
  if ((rc = tracts_device(h, source, threshold, min_sites, &d, &n))) return rc;
  out.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(out.data(), d, n * sizeof(TractRec), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));
  return NGHMM_OK;
}

}  // namespace capi

int nghmm_ibd_tracts(nghmm_t* h, int source, double threshold, uint64_t min_sites,
                     nghmm_tract* out, uint64_t cap, uint64_t* n_total) {
  g_last_error.clear();
  if (!n_total || (cap && !out)) {
    set_error("nghmm_ibd_tracts: n_total is NULL, or out is NULL with cap > 0");
    return NGHMM_ERR_ARG;
  }
  int rc;
  if ((rc = tracts_check_args(h, source, threshold, "nghmm_ibd_tracts"))) return rc;
  const TractRec* d = nullptr;
  uint64_t n = 0;
  if ((rc = tracts_device(h, source, threshold, min_sites, &d, &n))) return rc;
  const uint64_t m = cap < n ? cap : n;
  if (m) HIP_TRY(hipMemcpyAsync(out, d, m * sizeof(TractRec), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));
  *n_total = n;
  return NGHMM_OK;
}
