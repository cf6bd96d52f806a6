// capi_freqinfo.hip -- nghmm_freq_info / nghmm_chain_freq_info: per site the log-likelihood of the
// cohort in that site's allele frequency, its first two derivatives and its values at a few levels
// (kernels_freqinfo.hip).  One handle: the segments (the chromosomes' parts it holds, from one copy
// of the distances), the forward walk, the backward walk that leaves the cavity weights, the site
// pass, the copies.  A chain: the forward walks from the first shard to the last, each starting
// from the vector the shard before ended with, then the backward walks from the last to the first,
// I x 2 doubles per boundary; every vector is a plain site-by-site recursion, so the shards
// continue the single handle's arithmetic bit for bit and the outputs are the concatenation of the
// shards'.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_internal.hpp"
#include "kernels_freqinfo.hpp"

static_assert(sizeof(nghmm_freq_stat) == 32, "nghmm_freq_stat is 32 bytes");
static_assert(sizeof(FreqStat) == sizeof(nghmm_freq_stat), "the device's record is nghmm_freq_stat");

namespace {

uint64_t align256(uint64_t n) { return (n + 255) & ~255ull; }

// the handle's scratch (h->d_finfo), carved
struct Carve {
  double *vin, *vout, *cav, *curve, *cav_out;
  FreqStat* stats;
  uint64_t* seg;
  uint64_t n_seg = 0;
};

int carve(nghmm_t* h, uint64_t n_seg, uint32_t n_levels, bool want_cavity, Carve& c) {
  const uint64_t I = h->I, S = h->S;
  const uint64_t b_vec = align256(I * 2 * sizeof(double));
  const uint64_t b_cav = align256(S * I * 2 * sizeof(double)), b_seg = align256((n_seg + 1) * sizeof(uint64_t));
  const uint64_t b_stats = align256(S * sizeof(FreqStat)), b_curve = align256(S * n_levels * sizeof(double));
  const uint64_t b_out = want_cavity ? align256(S * I * sizeof(double)) : 0;
  int rc;
  if ((rc = h->d_finfo.reserve(2 * b_vec + b_seg + b_cav + b_stats + b_curve + b_out))) return rc;
  uint8_t* p = h->d_finfo.p;
  c.vin = reinterpret_cast<double*>(p);
  p += b_vec;
  c.vout = reinterpret_cast<double*>(p);
  p += b_vec;
  c.seg = reinterpret_cast<uint64_t*>(p);
  p += b_seg;
  c.n_seg = n_seg;
  c.cav = reinterpret_cast<double*>(p);
  p += b_cav;
  c.stats = reinterpret_cast<FreqStat*>(p);
  p += b_stats;
  c.curve = reinterpret_cast<double*>(p);
  p += b_curve;
  c.cav_out = reinterpret_cast<double*>(p);
  return NGHMM_OK;
}

int freqinfo_impl(nghmm_t** hs, int n, uint32_t n_levels, const double* levels, nghmm_freq_stat* stats,
                  double* curve, double* cavity, const char* who) {
  for (int r = 0; r < n; ++r)
    if (!hs[r] || !hs[r]->loaded) {
      set_error("%s: the handle holds no data", who);
      return NGHMM_ERR_ARG;
    }
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
  if (n > 1 && !fast) {
    set_error("%s: site shards are a fast-mode layout", who);
    return NGHMM_ERR_ARG;
  }
  const uint64_t I = hs[0]->I;
  uint64_t S_tot = 0;
  std::vector<uint64_t> base(n);
  for (int r = 0; r < n; ++r) {
    base[r] = S_tot;
    S_tot += hs[r]->S;
  }
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
    if ((rc = carve(h, fast ? seg.size() - 1 : 0, n_levels, cavity != nullptr, cv[r]))) return rc;
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
  // the backward walks, last shard to first; behind each the shard's site pass
  std::vector<double> rows;
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
                               r > 0 ? c.vout : nullptr, c.cav, h->d_flags, true) ||
          !freqinfo_sites(h->stream, c.cav, fast_gl_lin(h->fast), false, h->d_freq, S, I, lv, c.stats,
                          c.curve)) {
        set_error("%s: a kernel launch failed", who);
        return NGHMM_ERR_HIP;
      }
      if (r > 0) HIP_TRY(hipMemcpyAsync(vec.data(), c.vout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
      launch_freqinfo_exact(h->stream, own_gl(h), h->d_freq, h->d_pos, h->d_fw, S, I, h->d_indF, h->d_alpha,
                            c.cav, h->d_flags);
      HIP_TRY(hipGetLastError());
      if (!freqinfo_sites(h->stream, c.cav, own_gl(h), true, h->d_freq, S, I, lv, c.stats, c.curve)) {
        set_error("%s: a kernel launch failed", who);
        return NGHMM_ERR_HIP;
      }
    }
    if (cavity && !freqinfo_cavity_out(h->stream, c.cav, S, I, c.cav_out)) {
      set_error("%s: a kernel launch failed", who);
      return NGHMM_ERR_HIP;
    }
    HIP_TRY(hipGetLastError());
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    if (stats)
      HIP_TRY(hipMemcpyAsync(stats + base[r], c.stats, S * sizeof(FreqStat), hipMemcpyDeviceToHost, h->stream));
    if (curve)
      HIP_TRY(hipMemcpyAsync(curve + base[r] * n_levels, c.curve, S * n_levels * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
    if (cavity) {
      double* dst = cavity;
      if (n > 1) {
        rows.resize((size_t)I * S);
        dst = rows.data();
      }
      HIP_TRY(hipMemcpyAsync(dst, c.cav_out, I * S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(sync_stream(h));
    if (cavity && n > 1)
      for (uint64_t i = 0; i < I; ++i)
        std::memcpy(cavity + i * S_tot + base[r], rows.data() + i * S, S * sizeof(double));
  }
  return NGHMM_OK;
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
  if (!hs || n_handles < 1) {
    set_error("nghmm_chain_freq_info: no handles");
    return NGHMM_ERR_ARG;
  }
  if (n_handles > 1) {
    struct ChainCtx* cx = hs[0] ? hs[0]->chain : nullptr;
    bool ok = cx != nullptr;
    for (int r = 0; ok && r < n_handles; ++r)
      ok = hs[r] && hs[r]->chain == cx && hs[r]->fast.shard.rank == (uint32_t)r &&
           hs[r]->fast.shard.world == (uint32_t)n_handles;
    if (!ok) {
      set_error("nghmm_chain_freq_info: call nghmm_chain_setup on these handles first");
      return NGHMM_ERR_ARG;
    }
  }
  return freqinfo_impl(hs, n_handles, n_levels, levels, stats, curve, cavity, "nghmm_chain_freq_info");
}
