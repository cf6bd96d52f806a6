// capi_sharing.hip -- pairwise IBD sharing of one handle (nghmm_ibd_sharing; the chain's merge is
// in capi_multi.hip): the site range cut into K-splits, per output one matrix-core kernel over
// the splits and one finish kernel that adds them in site order (kernels_sharing.hip), the
// [I][I] matrices copied out once.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_internal.hpp"

static_assert(NGHMM_SHARING_VITERBI == SHARING_VITERBI && NGHMM_SHARING_POSTERIOR == SHARING_POSTERIOR,
              "sharing sources");

namespace capi {

int sharing_check_args(nghmm_t* h, int what, double threshold, const void* vit_both,
                       const void* post_both, const void* post_prod, const char* who) {
  if (!h || !h->loaded) {
    set_error("%s: the handle holds no data", who);
    return NGHMM_ERR_ARG;
  }
  if (what == 0 || (what & ~(NGHMM_SHARING_VITERBI | NGHMM_SHARING_POSTERIOR))) {
    set_error("%s: what = %d is not a mask of NGHMM_SHARING_VITERBI and NGHMM_SHARING_POSTERIOR", who,
              what);
    return NGHMM_ERR_ARG;
  }
  const bool vit = (what & NGHMM_SHARING_VITERBI) != 0, post = (what & NGHMM_SHARING_POSTERIOR) != 0;
  if (vit != (vit_both != nullptr) || post != (post_both != nullptr || post_prod != nullptr)) {
    set_error("%s: vit_both is NULL iff NGHMM_SHARING_VITERBI is not asked for; post_both and "
              "post_prod are both NULL iff NGHMM_SHARING_POSTERIOR is not", who);
    return NGHMM_ERR_ARG;
  }
  if (vit && !h->path_decoded) {
    set_error("%s: no Viterbi decode since the data were loaded (run nghmm_viterbi first)", who);
    return NGHMM_ERR_ARG;
  }
  if (post_both && !(threshold > 0.0 && threshold <= 1.0)) {
    set_error("%s: the posterior threshold %g is not in (0, 1]", who, threshold);
    return NGHMM_ERR_ARG;
  }
  return NGHMM_OK;
}

int sharing_check_range(uint64_t S, uint64_t site_begin, uint64_t site_end, const char* who) {
  if (!(site_begin < site_end) || site_end > S) {
    set_error("%s: the sites [%llu, %llu) are none, or end behind the last of the %llu sites", who,
              (unsigned long long)site_begin, (unsigned long long)site_end, (unsigned long long)S);
    return NGHMM_ERR_ARG;
  }
  return NGHMM_OK;
}

// Arguments checked by the caller.
int sharing_to_host(nghmm_t* h, double thr, uint64_t begin, uint64_t end, uint64_t* vit_both,
                    uint64_t* post_both, double* post_prod) {
  int rc;
  if ((rc = use_device(h))) return rc;
  // fast mode: the site-major copy of the tile-major posteriors (kept until the next E-step)
  if ((post_both || post_prod) && (rc = ensure_marg(h))) return rc;
  const uint64_t I = h->I;
  const SharingPlan plan = sharing_plan(I, begin, end);
  if (plan.len >= (1ull << 31)) {   // (a split's counts are int32)
    set_error("nghmm_ibd_sharing: %llu sites a split", (unsigned long long)plan.len);
    return NGHMM_ERR_ARG;
  }
  // d_share: the splits' partial matrices [n][I][I] (8 bytes an entry; the counts use half) |
  // the result [I][I] | the thresholded bytes of the range's blocks (16-byte loads: aligned)
  const size_t cells = (size_t)I * I;
  const size_t o_out = plan.n * cells * 8, o_bytes = (o_out + cells * 8 + 255) / 256 * 256;
  const uint64_t block0 = begin / 16, nblk = (end + 15) / 16 - block0;
  if ((rc = h->d_share.reserve(o_bytes + (post_both ? nblk * I * 16 : 0)))) return rc;
  uint8_t* base = h->d_share.p;
  // one output after the other on the handle's stream, so that they share the scratch
  if (vit_both) {
    launch_sharing_count(h->stream, h->d_path_sites, 0, I, begin, end, plan,
                         reinterpret_cast<int32_t*>(base));
    launch_sharing_finish_count(h->stream, reinterpret_cast<const int32_t*>(base), plan.n, I,
                                reinterpret_cast<uint64_t*>(base + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(vit_both, base + o_out, cells * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (post_both) {
    launch_sharing_threshold(h->stream, h->d_marg, I, begin, end, thr, base + o_bytes);
    launch_sharing_count(h->stream, base + o_bytes, block0, I, begin, end, plan,
                         reinterpret_cast<int32_t*>(base));
    launch_sharing_finish_count(h->stream, reinterpret_cast<const int32_t*>(base), plan.n, I,
                                reinterpret_cast<uint64_t*>(base + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(post_both, base + o_out, cells * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (post_prod) {
    launch_sharing_prod(h->stream, h->d_marg, I, begin, end, plan, reinterpret_cast<double*>(base));
    launch_sharing_finish_prod(h->stream, reinterpret_cast<const double*>(base), plan.n, I,
                               reinterpret_cast<double*>(base + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(post_prod, base + o_out, cells * 8, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(sync_stream(h));
  return NGHMM_OK;
}

}  // namespace capi

int nghmm_ibd_sharing(nghmm_t* h, int what, double threshold, uint64_t site_begin, uint64_t site_end,
                      uint64_t* vit_both, uint64_t* post_both, double* post_prod) {
  g_last_error.clear();
  int rc;
  if ((rc = sharing_check_args(h, what, threshold, vit_both, post_both, post_prod, "nghmm_ibd_sharing")))
    return rc;
  if ((rc = sharing_check_range(h->S, site_begin, site_end, "nghmm_ibd_sharing"))) return rc;
  return sharing_to_host(h, threshold, site_begin, site_end, vit_both, post_both, post_prod);
}
