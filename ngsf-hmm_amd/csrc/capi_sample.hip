// capi_sample.hip -- nghmm_sample_paths / nghmm_chain_sample_paths: IBD paths drawn from the joint
// posterior (kernels_sample.hip), in batches of kSampleBatch draws that share their walks.  A
// chain is walked like nghmm_chain_viterbi: the forward vectors from the first shard to the last,
// then per batch the sampled states from the last shard to the first; the shards' statistics are
// merged on the host (seg_merge, the rule the device uses between lane-chunks).
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_chain.hpp"
#include "kernels_sample.hpp"

static_assert(sizeof(nghmm_path_stats) == 32, "nghmm_path_stats is 32 bytes");

namespace {

nghmm_path_stats seg_stats(const SampleSeg& s) {
  nghmm_path_stats o;
  o.ibd_sites = s.ones;
  o.n_tracts = s.inner_n + (s.full ? 1 : (s.head > 0) + (s.tail > 0));
  o.longest_sites = std::max(s.inner_longest, std::max(s.head, s.tail));
  o.ibd_mb = s.mb;
  return o;
}

struct Shard {
  SampleScratch scr;
  double *d_vin = nullptr, *d_vout = nullptr, *d_lkl = nullptr;
  uint64_t base = 0;   // global index of its first site
  double d0 = 0;       // distance in front of its first site
  std::vector<SampleSeg> seg;
};

int sample_impl(nghmm_t** hs, int n, uint64_t seed, uint32_t n_draws, nghmm_path_stats* stats,
                uint32_t n_keep, uint8_t* paths, const char* who) {
  int rc;
  if ((rc = chain_check_loaded(hs, n, who))) return rc;
  if (n_draws == 0 || n_keep > n_draws || (n_keep > 0) != (paths != nullptr)) {
    set_error("%s: n_draws = %u, n_keep = %u, paths %s: n_draws >= 1, n_keep <= n_draws and paths "
              "NULL exactly when n_keep == 0 are needed", who, n_draws, n_keep, paths ? "given" : "NULL");
    return NGHMM_ERR_ARG;
  }
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  const uint64_t I = hs[0]->I;
  const uint32_t keep_batch = std::min(n_keep, kSampleBatch);
  std::vector<Shard> sh(n);
  uint64_t S_tot = 0;
  // scratch, and the forward half: first shard to last
  std::vector<double> vec((size_t)I * 2);
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    x.base = S_tot;
    S_tot += h->S;
    if ((rc = use_device(h))) return rc;
    const uint64_t J = fast ? h->fast.J : 0, pitch = fast ? h->fast.Spad : h->S;
    const uint64_t body = sample_scratch_bytes(I, J, pitch, keep_batch);
    if ((rc = h->d_samp.reserve(body + I * 5 * sizeof(double)))) return rc;
    x.scr = sample_scratch_carve(h->d_samp, I, J, pitch);
    x.d_vin = reinterpret_cast<double*>(h->d_samp.p + body);
    x.d_vout = x.d_vin + I * 2;
    x.d_lkl = x.d_vout + I * 2;
    x.seg.resize((size_t)kSampleBatch * I);
    HIP_TRY(hipMemcpyAsync(&x.d0, h->d_pos, sizeof x.d0, hipMemcpyDeviceToHost, h->stream));
    if ((rc = clear_flags(h))) return rc;
    if (fast) {
      if ((rc = ensure_emissions(h))) return rc;
      if (r > 0)
        HIP_TRY(hipMemcpyAsync(x.d_vin, vec.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (!sample_fast_forward(h->fast, h->stream, h->d_indF, h->d_alpha, r ? x.d_vin : nullptr, x.d_vout))
        return NGHMM_ERR_HIP;
      if (r + 1 < n)
        HIP_TRY(hipMemcpyAsync(vec.data(), x.d_vout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
      (h->fast.sw.exact_serial ? launch_forward_exact : launch_forward_exact_pc)(
          h->stream, h->d_eprob, h->d_pos, h->S, h->I, (uint32_t)h->I, nullptr, h->d_indF, h->d_alpha,
          x.d_lkl, h->d_fw, h->d_flags);
    }
    HIP_TRY(hipGetLastError());
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
  }
  // the backward half, a batch of draws at a time: last shard to first
  std::vector<uint8_t> state((size_t)kSampleBatch * I);
  for (uint32_t draw0 = 0; draw0 < n_draws; draw0 += kSampleBatch) {
    const uint32_t nd = std::min(kSampleBatch, n_draws - draw0);
    const uint32_t np = draw0 < n_keep ? std::min(nd, n_keep - draw0) : 0;
    for (int r = n - 1; r >= 0; --r) {
      nghmm_t* h = hs[r];
      Shard& x = sh[r];
      const bool last = r == n - 1;
      if ((rc = use_device(h))) return rc;
      if (fast) {
        if (!last)
          HIP_TRY(hipMemcpyAsync(x.scr.state_in, state.data(), (size_t)nd * I, hipMemcpyHostToDevice, h->stream));
        if (!sample_fast_backward(h->fast, h->stream, h->d_indF, h->d_alpha, seed, draw0, nd, x.base, last,
                                  last ? 0.0 : sh[r + 1].d0, np, x.scr))
          return NGHMM_ERR_HIP;
        if (r > 0)
          HIP_TRY(hipMemcpyAsync(state.data(), x.scr.state_out, (size_t)nd * I, hipMemcpyDeviceToHost, h->stream));
      } else {
        launch_sample_exact(h->stream, h->d_fw, h->d_pos, h->S, I, h->d_indF, h->d_alpha, seed, draw0, nd,
                            np, x.scr);
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(x.seg.data(), x.scr.seg, (size_t)nd * I * sizeof(SampleSeg),
                             hipMemcpyDeviceToHost, h->stream));
      if (np && x.scr.pitch == h->S && S_tot == h->S)
        // one handle in exact mode: the rows follow each other on both sides, one plain copy (the
        // strided one to pageable memory makes the runtime keep staging memory of its own, 2 MiB
        // at a time, when a second stream of the process has done it too)
        HIP_TRY(hipMemcpyAsync(paths + (size_t)draw0 * I * S_tot, x.scr.paths, (size_t)np * I * h->S,
                               hipMemcpyDeviceToHost, h->stream));
      else if (np)
        HIP_TRY(hipMemcpy2DAsync(paths + (size_t)draw0 * I * S_tot + x.base, S_tot, x.scr.paths,
                                 x.scr.pitch, h->S, (size_t)np * I, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(sync_stream(h));
    }
    if (stats)
      for (uint64_t k = 0; k < (uint64_t)nd * I; ++k) {
        SampleSeg acc = sh[0].seg[k];
        for (int r = 1; r < n; ++r)
          acc = seg_merge(acc, sh[r].seg[k], !(sh[r].d0 < 1e22), sh[r].d0);
        stats[(size_t)draw0 * I + k] = seg_stats(acc);
      }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_sample_paths(nghmm_t* h, uint64_t seed, uint32_t n_draws, nghmm_path_stats* stats,
                       uint32_t n_keep, uint8_t* paths) {
  g_last_error.clear();
  return sample_impl(&h, 1, seed, n_draws, stats, n_keep, paths, "nghmm_sample_paths");
}

int nghmm_chain_sample_paths(nghmm_t** hs, int n, uint64_t seed, uint32_t n_draws,
                             nghmm_path_stats* stats, uint32_t n_keep, uint8_t* paths) {
  g_last_error.clear();
  const char* who = "nghmm_chain_sample_paths";
  const int rc = chain_entry_check(hs, n, who);
  return rc ? rc : sample_impl(hs, n, seed, n_draws, stats, n_keep, paths, who);
}
