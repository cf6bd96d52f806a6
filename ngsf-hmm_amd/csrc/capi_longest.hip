// capi_longest.hip -- nghmm_ibd_longest / nghmm_chain_ibd_longest: per individual, region and
// threshold the probability that some IBD run of the region reaches the threshold, and that none
// does (kernels_longest.hip).  The host checks the arguments, forms cum and the table b_k(a) once
// per call over the whole site axis exactly as capi_bylength.hip does, cuts the regions into their
// parts per chromosome, and sizes every lane's ring from the table.  The backward walks go from the
// last shard to the first (beta across the cuts, I x 2 doubles), the forward walks from the first
// to the last (the lane state across the cuts: pi, Q and per threshold N, V, Hit, ap and the ring's
// live entries); every walk is a plain site-by-site recursion, so a shard continues the single
// handle's arithmetic bit for bit.  A region's parts are combined on the host in site order.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_longest_host.hpp"

static_assert(sizeof(nghmm_longest_stat) == 16, "nghmm_longest_stat is 16 bytes");
static_assert(sizeof(nghmm_longest_stat) == sizeof(LongestRec) &&
                  offsetof(nghmm_longest_stat, p_any) == offsetof(LongestRec, p_any) &&
                  offsetof(nghmm_longest_stat, p_none) == offsetof(LongestRec, p_none),
              "the device's record is nghmm_longest_stat");

namespace {

struct Shard {
  uint64_t base = 0;
  bool cont = false;                 // its first site goes on from the shard before
  std::vector<uint64_t> seg;         // first sites of its segments, then S
  std::vector<uint64_t> roff;        // [n_seg][K] first ring entry
  std::vector<uint32_t> rcap;        // [n_seg][K] ring entries
  uint64_t ring_entries = 0;
  std::vector<LongestRec> rec;       // [I][P][K]
  // device scratch (h->d_lng)
  uint64_t* d_seg = nullptr;
  double *d_win = nullptr, *d_wout = nullptr, *d_piseg = nullptr;
  uint32_t* d_btab = nullptr;
  LongestPart* d_part = nullptr;
  uint64_t* d_roff = nullptr;
  uint32_t* d_rcap = nullptr;
  LongestCarry *d_cin = nullptr, *d_cout = nullptr;
  LongestRec* d_rec = nullptr;
  int* d_ovf = nullptr;              // raised by a lane whose ring was full at a push
  // (h->d_lng_ring)
  double2 *d_ring = nullptr, *d_rin = nullptr;
};

int longest_impl(nghmm_t** hs, int n, int what, uint32_t K, const double* min_len, uint64_t n_regions,
                 const uint64_t* begin, const uint64_t* end, nghmm_longest_stat* stats, const char* who) {
  uint64_t S_tot = 0;
  int rc;
  if ((rc = chain_check_loaded(hs, n, who, &S_tot))) return rc;
  if (what & ~NGHMM_LONGEST_MB) {
    set_error("%s: what = %d is not 0 or NGHMM_LONGEST_MB", who, what);
    return NGHMM_ERR_ARG;
  }
  const bool mb = (what & NGHMM_LONGEST_MB) != 0;
  if ((rc = longest_host::check_lengths(mb, K, min_len, who))) return rc;
  const uint64_t I = hs[0]->I, R = n_regions;
  if ((rc = summary_check_regions(S_tot, I, R, begin, end, stats, nullptr, who))) return rc;
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  if ((rc = longest_host::check_site_count(S_tot, who))) return rc;
  // the distances of the whole site axis, cum and the chromosomes' edges; b_k(a); the regions' parts
  // per chromosome (capi_longest_host.hpp)
  std::vector<Shard> sh(n);
  longest_host::Axis ax;
  if ((rc = longest_host::read_axis(hs, n, S_tot, ax))) return rc;
  for (int r = 0; r < n; ++r) sh[r].base = ax.base[r];
  longest_host::window_table(ax, mb, K, min_len);
  longest_host::region_parts(ax, R, begin, end);
  auto is_start = [&](uint64_t s) { return ax.is_start(s); };
  const std::vector<uint32_t>& bt = ax.bt;
  const std::vector<LongestPart>& parts = ax.parts;
  const std::vector<uint64_t>& owner = ax.owner;
  const uint64_t P = parts.size();
  // segments, rings and scratch of every shard
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const uint64_t S = h->S;
    if ((rc = use_device(h))) return rc;
    x.cont = r > 0 && !is_start(x.base);
    const uint64_t E = longest_host::shard_rings(ax, x.base, S, K, x.seg, x.roff, x.rcap);
    const uint64_t n_seg = x.seg.size() - 1;
    x.ring_entries = E;
    x.rec.resize((size_t)I * P * K);
    const uint64_t rin_entries = x.cont ? sh[r - 1].ring_entries - sh[r - 1].roff[sh[r - 1].roff.size() - K] : 0;
    Carver cv;
    cv.add(&x.d_seg, n_seg + 1);
    cv.add(&x.d_win, I * 2);
    cv.add(&x.d_wout, I * 2);
    cv.add(&x.d_piseg, n_seg * I * 2);
    cv.add(&x.d_btab, (uint64_t)K * S_tot);
    cv.add(&x.d_part, P);
    cv.add(&x.d_roff, n_seg * K);
    cv.add(&x.d_rcap, n_seg * K);
    cv.add(&x.d_cin, I);
    cv.add(&x.d_cout, I);
    cv.add(&x.d_rec, I * P * K);
    cv.add(&x.d_ovf, 1);
    if ((rc = cv.reserve(h->d_lng))) return rc;
    Carver cr;
    cr.add(&x.d_ring, E * I);
    cr.add(&x.d_rin, rin_entries * I);
    if ((rc = cr.reserve(h->d_lng_ring))) return rc;
    if ((rc = h->d_lng_cell.reserve(longest_plane_bytes(S, I)))) return rc;
  }
  // the backward walks, last shard to first
  std::vector<double> vec((size_t)I * 2);
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const uint64_t S = h->S, n_seg = x.seg.size() - 1;
    const bool last = r == n - 1;
    if ((rc = use_device(h))) return rc;
    if ((rc = clear_flags(h))) return rc;
    const LongestPlanes pl = longest_carve(h->d_lng_cell.p, S, I);
    HIP_TRY(hipMemcpyAsync(x.d_seg, x.seg.data(), x.seg.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if (fast) {
      if (!last) HIP_TRY(hipMemcpyAsync(x.d_win, vec.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (!longest_fast_bwd(h->stream, fast_gl_lin(h->fast), h->d_freq, h->d_pos, x.d_seg, n_seg, S, I, h->d_indF,
                            h->d_alpha, r == 0, last ? nullptr : x.d_win, r > 0 ? x.d_wout : nullptr, pl,
                            x.d_piseg, h->d_flags)) {
        set_error("%s: a kernel launch failed", who);
        return NGHMM_ERR_HIP;
      }
      if (r > 0) HIP_TRY(hipMemcpyAsync(vec.data(), x.d_wout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
      launch_longest_bwd_exact(h->stream, own_gl(h), h->d_freq, h->d_pos, S, I, n_seg, h->d_indF, h->d_alpha, pl,
                               x.d_piseg, h->d_flags);
    }
    HIP_TRY(hipGetLastError());
    if ((rc = check_flags(h))) return rc;   // (waits for the stream: vec has arrived)
  }
  // the forward walks, first shard to last
  std::vector<LongestCarry> carry;
  std::vector<double2> ring_h;
  // NGHMM_LONGEST_SPLIT=0 / 1 (for measurements) overrides the rule that gives the thresholds
  // lanes of their own; the records are the same bits either way
  const char* split_env = std::getenv("NGHMM_LONGEST_SPLIT");
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const uint64_t S = h->S, n_seg = x.seg.size() - 1;
    const bool give = r + 1 < n && sh[r + 1].cont;
    if ((rc = use_device(h))) return rc;
    const LongestPlanes pl = longest_carve(h->d_lng_cell.p, S, I);
    HIP_TRY(hipMemcpyAsync(x.d_btab, bt.data(), bt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (P) HIP_TRY(hipMemcpyAsync(x.d_part, parts.data(), P * sizeof(LongestPart), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(x.d_roff, x.roff.data(), x.roff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(x.d_rcap, x.rcap.data(), x.rcap.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    LongestRingIn rin{};
    if (x.cont) {
      const Shard& pv = sh[r - 1];
      const uint64_t g0 = pv.roff.size() - K;
      for (uint32_t k = 0; k < K; ++k) {
        rin.off[k] = pv.roff[g0 + k] - pv.roff[g0];
        rin.cap[k] = pv.rcap[g0 + k];
      }
      rin.ring = x.d_rin;
      HIP_TRY(hipMemcpyAsync(x.d_cin, carry.data(), I * sizeof(LongestCarry), hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(x.d_rin, ring_h.data(), ring_h.size() * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    }
    const LongestRings rings{x.d_ring, x.d_roff, x.d_rcap};
    const bool split = (split_env && (split_env[0] == '0' || split_env[0] == '1'))
                           ? split_env[0] == '1' && K > 1
                           : longest_split_lanes(n_seg, I, K);
    int overflow = 0;
    HIP_TRY(hipMemsetAsync(x.d_ovf, 0, sizeof(int), h->stream));
    if (!longest_fwd(h->stream, !fast, split, x.d_seg, n_seg, S, I, x.base, S_tot, K, x.d_btab, x.d_part, P, pl,
                     x.d_piseg, rings, x.cont ? x.d_cin : nullptr, rin, give ? x.d_cout : nullptr, x.d_rec, x.d_ovf)) {
      set_error("%s: a kernel launch failed", who);
      return NGHMM_ERR_HIP;
    }
    HIP_TRY(hipGetLastError());
    if (P)
      HIP_TRY(hipMemcpyAsync(x.rec.data(), x.d_rec, I * P * K * sizeof(LongestRec), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&overflow, x.d_ovf, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(sync_stream(h));   // (carry and ring_h are the host's again)
    if (overflow) {
      set_error("%s: a lane's ring was full at a push in shard %d: the rings were sized wrongly (internal error)",
                who, r);
      return NGHMM_ERR_HIP;
    }
    if (give) {
      const uint64_t e0 = x.roff[x.roff.size() - K];
      carry.resize(I);
      ring_h.resize((size_t)(x.ring_entries - e0) * I);
      HIP_TRY(hipMemcpyAsync(carry.data(), x.d_cout, I * sizeof(LongestCarry), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipMemcpyAsync(ring_h.data(), x.d_ring + e0 * I, ring_h.size() * sizeof(double2), hipMemcpyDeviceToHost,
                             h->stream));
      HIP_TRY(sync_stream(h));
    }
  }
  // a region's parts in site order: chromosomes are independent given the parameters
  {
    int r = 0;
    uint64_t prev_owner = ~0ull;
    for (uint64_t p = 0; p < P; ++p) {
      const uint64_t last_site = parts[p].end - 1;
      while (last_site >= sh[r].base + hs[r]->S) ++r;   // (the parts are sorted)
      const uint64_t o = owner[p];
      for (uint64_t i = 0; i < I; ++i)
        for (uint32_t k = 0; k < K; ++k) {
          const LongestRec& s = sh[r].rec[(i * P + p) * K + k];
          nghmm_longest_stat& d = stats[(i * R + o) * K + k];
          if (o != prev_owner) {
            d.p_any = s.p_any;
            d.p_none = s.p_none;
          } else {
            d.p_any = d.p_any + d.p_none * s.p_any;
            d.p_none = d.p_none * s.p_none;
          }
        }
      prev_owner = o;
    }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_ibd_longest(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, uint64_t n_regions,
                      const uint64_t* region_begin, const uint64_t* region_end, nghmm_longest_stat* stats) {
  g_last_error.clear();
  return longest_impl(&h, 1, what, n_lengths, min_length, n_regions, region_begin, region_end, stats,
                      "nghmm_ibd_longest");
}

int nghmm_chain_ibd_longest(nghmm_t** hs, int n_handles, int what, uint32_t n_lengths, const double* min_length,
                            uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_longest_stat* stats) {
  g_last_error.clear();
  const char* who = "nghmm_chain_ibd_longest";
  const int rc = chain_entry_check(hs, n_handles, who);
  if (rc) return rc;
  return longest_impl(hs, n_handles, what, n_lengths, min_length, n_regions, region_begin, region_end, stats, who);
}
