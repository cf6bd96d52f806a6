// capi_cavity.hip -- cavity_walks: the cavity weights (1 - c, c) of every cell of a handle or a
// chain of site shards at the current parameters, which nghmm_freq_info (capi_freqinfo.hip) and
// nghmm_geno_smooth (capi_genosmooth.hip) both start from.  One handle: the segments (the
// chromosomes' parts it holds, from one copy of the distances), the forward walk, the backward
// walk that leaves the weights.  A chain: the forward walks from the first shard to the last, each
// starting from the vector the shard before ended with, then the backward walks from the last to
// the first, I x 2 doubles per boundary through the host; every vector is a plain site-by-site
// recursion (kernels_freqinfo.hip), so the shards continue the single handle's arithmetic bit for
// bit.  (capi_internal.hpp has the declaration, the handle and the shared helpers.)
#include "capi_chain_host.hpp"
#include "capi_internal.hpp"
#include "kernels_freqinfo.hpp"

namespace {

// a shard's scratch (hs[r]->*owner), carved
struct Carve {
  double *vin, *vout, *cav;
  uint8_t* extra;
  uint64_t* seg;
  uint64_t n_seg = 0;
};

int carve(nghmm_t* h, DevScratch<uint8_t>& own, uint64_t n_seg, uint64_t b_extra, Carve& c) {
  const uint64_t I = h->I, S = h->S;
  Carver cv;
  cv.add(&c.vin, I * 2);
  cv.add(&c.vout, I * 2);
  cv.add(&c.seg, n_seg + 1);
  cv.add(&c.cav, S * I * 2);
  cv.add(&c.extra, b_extra);
  c.n_seg = n_seg;
  return cv.reserve(own);
}

}  // namespace

namespace capi {

int cavity_walks(nghmm_t** hs, int n, DevScratch<uint8_t> nghmm_handle::*owner,
                 const std::function<uint64_t(int)>& extra_bytes,
                 const std::function<int(int, const double*, uint8_t*)>& shard_done, const char* who) {
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  const uint64_t I = hs[0]->I;
  int rc;
  std::vector<Carve> cv(n);
  std::vector<double> vec((size_t)I * 2);
  // scratch and segments; the forward walks, first shard to last
  std::vector<double> pos;
  std::vector<uint64_t> seg;
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    const uint64_t S = h->S;
    if ((rc = use_device(h))) return rc;
    if (fast) {
      pos.resize(S);
      HIP_TRY(hipMemcpyAsync(pos.data(), h->d_pos, S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(sync_stream(h));
      seg.clear();
      for (uint64_t s = 0; s < S; ++s)
        if (s == 0 || freqinfo_chrom_start(pos[s])) seg.push_back(s);
      seg.push_back(S);
    }
    if ((rc = carve(h, h->*owner, fast ? seg.size() - 1 : 0, align256(extra_bytes(r)), cv[r]))) return rc;
    if ((rc = clear_flags(h))) return rc;
    if (!fast) continue;
    const Carve& c = cv[r];
    HIP_TRY(hipMemcpyAsync(c.seg, seg.data(), seg.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if (r > 0) HIP_TRY(hipMemcpyAsync(c.vin, vec.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (!freqinfo_fast_walks(h->stream, fast_gl_lin(h->fast), h->d_freq, h->d_pos, c.seg, c.n_seg, S, I,
                             h->d_indF, h->d_alpha, r ? c.vin : nullptr, r + 1 < n ? c.vout : nullptr,
                             nullptr, nullptr, c.cav, h->d_flags, false)) {
      set_error("%s: a kernel launch failed", who);
      return NGHMM_ERR_HIP;
    }
    if (r + 1 < n)
      HIP_TRY(hipMemcpyAsync(vec.data(), c.vout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(sync_stream(h));   // (seg and vec are the host's to reuse)
  }
  // the backward walks, last shard to first; behind each what the caller makes of the weights
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    const Carve& c = cv[r];
    const uint64_t S = h->S;
    const bool last = r == n - 1;
    if ((rc = use_device(h))) return rc;
    if (fast) {
      if (!last) HIP_TRY(hipMemcpyAsync(c.vin, vec.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (!freqinfo_fast_walks(h->stream, fast_gl_lin(h->fast), h->d_freq, h->d_pos, c.seg, c.n_seg, S, I,
                               h->d_indF, h->d_alpha, nullptr, nullptr, last ? nullptr : c.vin,
                               r > 0 ? c.vout : nullptr, c.cav, h->d_flags, true)) {
        set_error("%s: a kernel launch failed", who);
        return NGHMM_ERR_HIP;
      }
      if (r > 0) HIP_TRY(hipMemcpyAsync(vec.data(), c.vout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
      launch_freqinfo_exact(h->stream, own_gl(h), h->d_freq, h->d_pos, h->d_fw, S, I, h->d_indF, h->d_alpha,
                            c.cav, h->d_flags);
      HIP_TRY(hipGetLastError());
    }
    if ((rc = shard_done(r, c.cav, c.extra))) return rc;
    HIP_TRY(sync_stream(h));   // (vec has arrived; the caller's host buffers are its own again)
  }
  return NGHMM_OK;
}

}  // namespace capi
