// capi_freqinfo.hip -- nghmm_freq_info / nghmm_chain_freq_info: per site the log-likelihood of the
// cohort in that site's allele frequency, its first two derivatives and its values at a few levels
// (kernels_freqinfo.hip).  One handle: the segments (the chromosomes' parts it holds, from one copy
// of the distances), the forward walk, the backward walk that leaves the cavity weights, the site
// pass, the copies.  A chain: the forward walks from the first shard to the last, each starting
// from the vector the shard before ended with, then the backward walks from the last to the first,
// I x 2 doubles per boundary; every vector is a plain site-by-site recursion, so the shards
// continue the single handle's arithmetic bit for bit and the outputs are the concatenation of the
// shards'.  The walks and their vectors are cavity_walks (capi_cavity.hip), which
// capi_genosmooth.hip drives too; what this file makes of the weights is the site pass.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_chain.hpp"
#include "kernels_freqinfo.hpp"

static_assert(sizeof(nghmm_freq_stat) == 32, "nghmm_freq_stat is 32 bytes");
static_assert(sizeof(FreqStat) == sizeof(nghmm_freq_stat), "the device's record is nghmm_freq_stat");

namespace {

int freqinfo_impl(nghmm_t** hs, int n, uint32_t n_levels, const double* levels, nghmm_freq_stat* stats,
                  double* curve, double* cavity, const char* who) {
  int rc;
  if ((rc = chain_check_loaded(hs, n, who))) return rc;
  if (n_levels > FREQINFO_MAX_LEVELS) {
    set_error("%s: n_levels = %u: at most %u levels", who, n_levels, FREQINFO_MAX_LEVELS);
    return NGHMM_ERR_ARG;
  }
  if ((n_levels > 0) != (curve != nullptr) || (n_levels > 0 && !levels)) {
    set_error("%s: n_levels = %u, levels %s, curve %s: curve is NULL exactly when there are no levels", who,
              n_levels, levels ? "given" : "NULL", curve ? "given" : "NULL");
    return NGHMM_ERR_ARG;
  }
  if (!stats && !curve && !cavity) {
    set_error("%s: stats, curve and cavity are all NULL: nothing is asked for", who);
    return NGHMM_ERR_ARG;
  }
  FreqLevels lv{};
  lv.n = n_levels;
  for (uint32_t k = 0; k < n_levels; ++k) {
    if (!(levels[k] >= 0.0 && levels[k] <= 1.0)) {
      set_error("%s: levels[%u] = %g is outside [0, 1]", who, k, levels[k]);
      return NGHMM_ERR_ARG;
    }
    lv.f[k] = levels[k];
  }
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  const uint64_t I = hs[0]->I;
  uint64_t S_tot = 0;
  std::vector<uint64_t> base(n);
  for (int r = 0; r < n; ++r) {
    base[r] = S_tot;
    S_tot += hs[r]->S;
  }
  // the caller's bytes of a shard: the site records | the curve | c of every cell [I][S]
  auto b_stats = [&](int r) { return align256(hs[r]->S * sizeof(FreqStat)); };
  auto b_curve = [&](int r) { return align256(hs[r]->S * n_levels * sizeof(double)); };
  auto extra_bytes = [&](int r) {
    return b_stats(r) + b_curve(r) + (cavity ? align256(hs[r]->S * I * sizeof(double)) : 0);
  };
  std::vector<double> rows;
  // behind a shard's backward walk: its site pass and its copies
  auto shard_done = [&](int r, const double* d_cav, uint8_t* extra) -> int {
    nghmm_t* h = hs[r];
    const uint64_t S = h->S;
    int rc;
    FreqStat* d_stats = reinterpret_cast<FreqStat*>(extra);
    double* d_curve = reinterpret_cast<double*>(extra + b_stats(r));
    double* d_cav_out = reinterpret_cast<double*>(extra + b_stats(r) + b_curve(r));
    if (!freqinfo_sites(h->stream, d_cav, fast ? fast_gl_lin(h->fast) : own_gl(h), !fast, h->d_freq, S, I, lv,
                        d_stats, d_curve) ||
        (cavity && !freqinfo_cavity_out(h->stream, d_cav, S, I, d_cav_out))) {
      set_error("%s: a kernel launch failed", who);
      return NGHMM_ERR_HIP;
    }
    HIP_TRY(hipGetLastError());
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    if (stats)
      HIP_TRY(hipMemcpyAsync(stats + base[r], d_stats, S * sizeof(FreqStat), hipMemcpyDeviceToHost, h->stream));
    if (curve)
      HIP_TRY(hipMemcpyAsync(curve + base[r] * n_levels, d_curve, S * n_levels * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
    if (cavity) {
      double* dst = cavity;
      if (n > 1) {
        rows.resize((size_t)I * S);
        dst = rows.data();
      }
      HIP_TRY(hipMemcpyAsync(dst, d_cav_out, I * S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(sync_stream(h));
    if (cavity && n > 1)
      for (uint64_t i = 0; i < I; ++i)
        std::memcpy(cavity + i * S_tot + base[r], rows.data() + i * S, S * sizeof(double));
    return NGHMM_OK;
  };
  return cavity_walks(hs, n, &nghmm_handle::d_finfo, extra_bytes, shard_done, who);
}

}  // namespace

int nghmm_freq_info(nghmm_t* h, uint32_t n_levels, const double* levels, nghmm_freq_stat* stats,
                    double* curve, double* cavity) {
  g_last_error.clear();
  return freqinfo_impl(&h, 1, n_levels, levels, stats, curve, cavity, "nghmm_freq_info");
}

int nghmm_chain_freq_info(nghmm_t** hs, int n_handles, uint32_t n_levels, const double* levels,
                          nghmm_freq_stat* stats, double* curve, double* cavity) {
  g_last_error.clear();
  const char* who = "nghmm_chain_freq_info";
  const int rc = chain_entry_check(hs, n_handles, who);
  return rc ? rc : freqinfo_impl(hs, n_handles, n_levels, levels, stats, curve, cavity, who);
}
