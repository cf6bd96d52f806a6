// capi_chain.hip -- the entry checks of the chain calls and the relay of the boundary vectors
// (capi_chain.hpp has the declarations and what they promise).
#include "capi_chain.hpp"
#include "kernels_sample.hpp"
#include "kernels_support.hpp"

namespace capi {

int chain_entry_check(nghmm_t** hs, int n, const char* who) {
  if (!hs || n < 1) {
    set_error("%s: no handles", who);
    return NGHMM_ERR_ARG;
  }
  if (n > 1) {
    struct ChainCtx* cx = hs[0] ? hs[0]->chain : nullptr;
    bool ok = cx != nullptr;
    for (int r = 0; ok && r < n; ++r)
      ok = hs[r] && hs[r]->chain == cx && hs[r]->fast.shard.rank == (uint32_t)r &&
           hs[r]->fast.shard.world == (uint32_t)n;
    if (!ok) {
      set_error("%s: call nghmm_chain_setup on these handles first", who);
      return NGHMM_ERR_ARG;
    }
  }
  return NGHMM_OK;
}

int chain_check_loaded(nghmm_t** hs, int n, const char* who, uint64_t* S_tot) {
  uint64_t S = 0;
  for (int r = 0; r < n; ++r) {
    if (!hs[r] || !hs[r]->loaded) {
      set_error("%s: the handle holds no data", who);
      return NGHMM_ERR_ARG;
    }
    S += hs[r]->S;
  }
  if (S_tot) *S_tot = S;
  return NGHMM_OK;
}

int chain_check_fast(nghmm_t** hs, int n, const char* who) {
  if (n > 1 && hs[0]->mode != NGHMM_MODE_FAST) {
    set_error("%s: site shards are a fast-mode layout", who);
    return NGHMM_ERR_ARG;
  }
  return NGHMM_OK;
}

int fast_layout_error(const nghmm_t* h, const char* who) {
  set_error("%s: the fast layout (T = %llu sites per lane) is not one the walk knows, or a kernel "
            "launch failed", who, (unsigned long long)h->fast.T);
  return NGHMM_ERR_HIP;
}

ChainRelay::ChainRelay(nghmm_t** hs, int n, bool two_vectors)
    : hs_(hs), n_(n), fast_(hs[0]->mode == NGHMM_MODE_FAST), two_(two_vectors), I_(hs[0]->I), v_(n),
      vec_((size_t)hs[0]->I * 2) {}

void ChainRelay::add(Carver& cv, int r) {
  Vecs& v = v_[r];
  cv.add(&v.vin, I_ * 2);
  cv.add(&v.vout, I_ * 2);
  if (two_) return;
  cv.add(&v.win, I_ * 2);
  cv.add(&v.wout, I_ * 2);
}

int ChainRelay::forward(int r) {
  nghmm_t* h = hs_[r];
  const Vecs& v = v_[r];
  const size_t bytes = I_ * 2 * sizeof(double);
  int rc;
  if ((rc = clear_flags(h))) return rc;
  if (fast_) {
    if ((rc = ensure_emissions(h))) return rc;
    if (r > 0) HIP_TRY(hipMemcpyAsync(v.vin, vec_.data(), bytes, hipMemcpyHostToDevice, h->stream));
    if (!sample_fast_forward(h->fast, h->stream, h->d_indF, h->d_alpha, r ? v.vin : nullptr, v.vout))
      return NGHMM_ERR_HIP;
    if (r + 1 < n_) HIP_TRY(hipMemcpyAsync(vec_.data(), v.vout, bytes, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipGetLastError());
  return check_flags(h);   // (waits for the stream)
}

int ChainRelay::backward_upload(int r) {
  nghmm_t* h = hs_[r];
  if (r < n_ - 1)
    HIP_TRY(hipMemcpyAsync(win(r), vec_.data(), I_ * 2 * sizeof(double),
                           hipMemcpyHostToDevice, h->stream));
  return NGHMM_OK;
}

int ChainRelay::backward_bounds(int r, const char* who) {
  nghmm_t* h = hs_[r];
  if (support_fast_bounds(h->fast, h->stream, r < n_ - 1 ? win(r) : nullptr, r > 0 ? wout(r) : nullptr))
    return NGHMM_OK;
  return who ? fast_layout_error(h, who) : NGHMM_ERR_HIP;
}

int ChainRelay::backward_end(int r) {
  nghmm_t* h = hs_[r];
  if (r > 0)
    HIP_TRY(hipMemcpyAsync(vec_.data(), wout(r), I_ * 2 * sizeof(double),
                           hipMemcpyDeviceToHost, h->stream));
  return NGHMM_OK;
}

}  // namespace capi
