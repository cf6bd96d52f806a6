// capi_long_moments.hip -- nghmm_ibd_long_moments: per individual, region and threshold the mean and
// the covariance matrix of the total length and the number of the IBD runs of the region that reach
// the threshold (kernels_long_moments.hip).  The host checks the arguments, forms the table b_k(a),
// the regions' parts per chromosome and the rings exactly as nghmm_ibd_count does
// (capi_longest_host.hpp), runs nghmm_ibd_longest's backward walk into the handle's planes (the
// scratch is shared with it: every call fills what it reads) and the forward walk of
// kernels_long_moments.hip, and adds a region's parts in site order: chromosomes are independent.
// One handle only: the lane state is not carried across a shard cut.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_longest_host.hpp"
#include "kernels_long_moments.hpp"

static_assert(sizeof(nghmm_long_moment_stat) == sizeof(LongMomentRec), "the record of kernels_long_moments.hpp");

int nghmm_ibd_long_moments(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, uint64_t n_regions,
                           const uint64_t* region_begin, const uint64_t* region_end, nghmm_long_moment_stat* stats) {
  g_last_error.clear();
  const char* who = "nghmm_ibd_long_moments";
  const uint32_t K = n_lengths;
  uint64_t S_tot = 0;
  int rc;
  if ((rc = chain_check_loaded(&h, 1, who, &S_tot))) return rc;
  if (what & ~NGHMM_LONG_MOMENTS_MB) {
    set_error("%s: what = %d is not 0 or NGHMM_LONG_MOMENTS_MB", who, what);
    return NGHMM_ERR_ARG;
  }
  const bool mb = (what & NGHMM_LONG_MOMENTS_MB) != 0;
  if ((rc = longest_host::check_lengths(mb, K, min_length, who))) return rc;
  const uint64_t I = h->I, S = h->S, R = n_regions;
  if ((rc = summary_check_regions(S_tot, I, R, region_begin, region_end, stats, nullptr, who))) return rc;
  const bool fast = h->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(&h, 1, who))) return rc;
  if ((rc = longest_host::check_site_count(S_tot, who))) return rc;
  longest_host::Axis ax;
  if ((rc = longest_host::read_axis(&h, 1, S_tot, ax))) return rc;
  longest_host::window_table(ax, mb, K, min_length);
  longest_host::region_parts(ax, R, region_begin, region_end);
  const uint64_t P = ax.parts.size();
  std::vector<uint64_t> seg, roff;
  std::vector<uint32_t> rcap;
  const uint64_t E = longest_host::shard_rings(ax, 0, S, K, seg, roff, rcap);
  const uint64_t n_seg = seg.size() - 1;
  // len(a, s) = (cum[s] - cum[a]) + len_add and delta_s per site
  std::vector<double> cum(S), step(S);
  for (uint64_t s = 0; s < S; ++s) {
    cum[s] = mb ? ax.cum[s] : (double)s;
    step[s] = mb ? (ax.is_start(s) ? 0.0 : ax.pos[s]) : 1.0;
  }
  // device scratch: nghmm_ibd_longest's three owners
  uint64_t* d_seg = nullptr;
  double *d_piseg = nullptr, *d_ring = nullptr, *d_cum = nullptr, *d_step = nullptr;
  LongMomentRec* d_rec = nullptr;
  uint32_t *d_btab = nullptr, *d_rcap = nullptr;
  LongestPart* d_part = nullptr;
  uint64_t* d_roff = nullptr;
  int* d_ovf = nullptr;
  if ((rc = use_device(h))) return rc;
  Carver cv;
  cv.add(&d_seg, n_seg + 1);
  cv.add(&d_piseg, n_seg * I * 2);
  cv.add(&d_cum, S);
  cv.add(&d_step, S);
  cv.add(&d_btab, (uint64_t)K * S_tot);
  cv.add(&d_part, P);
  cv.add(&d_roff, n_seg * K);
  cv.add(&d_rcap, n_seg * K);
  cv.add(&d_rec, I * P * K);
  cv.add(&d_ovf, 1);
  if ((rc = cv.reserve(h->d_lng))) return rc;
  Carver cr;
  cr.add(&d_ring, E * kLongMomentEntry * I);
  if ((rc = cr.reserve(h->d_lng_ring))) return rc;
  if ((rc = h->d_lng_cell.reserve(longest_plane_bytes(S, I)))) return rc;
  // the backward walk: nghmm_ibd_longest's
  if ((rc = clear_flags(h))) return rc;
  const LongestPlanes pl = longest_carve(h->d_lng_cell.p, S, I);
  HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), seg.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  if (fast) {
    if (!longest_fast_bwd(h->stream, fast_gl_lin(h->fast), h->d_freq, h->d_pos, d_seg, n_seg, S, I, h->d_indF,
                          h->d_alpha, true, nullptr, nullptr, pl, d_piseg, h->d_flags)) {
      set_error("%s: a kernel launch failed", who);
      return NGHMM_ERR_HIP;
    }
  } else {
    launch_longest_bwd_exact(h->stream, own_gl(h), h->d_freq, h->d_pos, S, I, n_seg, h->d_indF, h->d_alpha, pl,
                             d_piseg, h->d_flags);
  }
  HIP_TRY(hipGetLastError());
  if ((rc = check_flags(h))) return rc;
  // the forward walk
  std::vector<LongMomentRec> part_rec((size_t)I * P * K);
  HIP_TRY(hipMemcpyAsync(d_btab, ax.bt.data(), ax.bt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_cum, cum.data(), S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_step, step.data(), S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (P) HIP_TRY(hipMemcpyAsync(d_part, ax.parts.data(), P * sizeof(LongestPart), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_roff, roff.data(), roff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_rcap, rcap.data(), rcap.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  int overflow = 0;
  HIP_TRY(hipMemsetAsync(d_ovf, 0, sizeof(int), h->stream));
  const CountRings rings{d_ring, d_roff, d_rcap};
  if (!long_moments_fwd(h->stream, !fast, d_seg, n_seg, S, I, K, d_btab, d_part, P, pl, d_piseg, rings, d_cum,
                        d_step, mb ? 0.0 : 1.0, d_rec, d_ovf)) {
    set_error("%s: a kernel launch failed", who);
    return NGHMM_ERR_HIP;
  }
  HIP_TRY(hipGetLastError());
  if (P)
    HIP_TRY(hipMemcpyAsync(part_rec.data(), d_rec, part_rec.size() * sizeof(LongMomentRec), hipMemcpyDeviceToHost,
                           h->stream));
  HIP_TRY(hipMemcpyAsync(&overflow, d_ovf, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));
  if (overflow) {
    set_error("%s: a lane's ring was full at a push: the rings were sized wrongly (internal error)", who);
    return NGHMM_ERR_HIP;
  }
  // A region's parts in site order: chromosomes are independent given the parameters, so means,
  // variances and the covariance of the region are the sums of the parts'
  {
    uint64_t prev_owner = ~0ull;
    for (uint64_t p = 0; p < P; ++p) {
      const uint64_t o = ax.owner[p];
      for (uint64_t i = 0; i < I; ++i)
        for (uint32_t k = 0; k < K; ++k) {
          LongMomentRec s = part_rec[(i * P + p) * K + k];
          nghmm_long_moment_stat* d = stats + (i * R + o) * K + k;
          // no window of the threshold fits into the part (b_k is non-decreasing: the first start's
          // is the earliest end): no long run, exactly
          const uint32_t b0 = ax.bt[(size_t)k * S_tot + ax.parts[p].begin];
          if (b0 == kLongestNone || b0 >= ax.parts[p].end) s = LongMomentRec{0.0, 0.0, 0.0, 0.0, 0.0};
          if (o != prev_owner) {
            *d = nghmm_long_moment_stat{s.mean_a, s.mean_t, s.var_a, s.cov_at, s.var_t};
            continue;
          }
          d->mean_a += s.mean_a;
          d->mean_t += s.mean_t;
          d->var_a += s.var_a;
          d->cov_at += s.cov_at;
          d->var_t += s.var_t;
        }
      prev_owner = o;
    }
  }
  return NGHMM_OK;
}
