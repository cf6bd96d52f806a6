// capi_bylength.hip -- nghmm_ibd_by_length / nghmm_chain_ibd_by_length: expected IBD above a
// minimum tract length (kernels_bylength.hip).  The host checks the arguments, forms cum and the
// table b_k(a) once per call over the whole site axis (two pointers per threshold), cuts the
// regions at the shard boundaries and numbers their pieces as capi_expect.hip does; the device does
// the rest.  A chain is walked like nghmm_chain_ibd_expect: the forward vectors from the first
// shard to the last; then from the last to the first the backward vectors, M and D at the cut
// (I x 2 doubles each) and the halo -- Q, n and rem of the first sites of the shard behind, as far
// as this shard's windows reach; a region across a cut is the sum of its parts in rank order.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_chain.hpp"
#include "kernels_bounds.hpp"
#include "kernels_bylength.hpp"

static_assert(sizeof(nghmm_bylength_stat) == sizeof(ByLenRec) &&
                  offsetof(nghmm_bylength_stat, tracts) == offsetof(ByLenRec, tracts) &&
                  offsetof(nghmm_bylength_stat, length) == offsetof(ByLenRec, length),
              "the device's record is nghmm_bylength_stat");

namespace {

struct Shard {
  uint64_t base = 0, H = 0;          // global index of its first site; sites of the halo
  std::vector<ExpectRegion> reg;     // its parts of the regions, handle-local
  std::vector<uint64_t> owner;       // the region a part belongs to
  std::vector<ByLenRec> rec;         // [I][reg.size()][K]
  uint64_t n_pieces = 0;
  // device scratch (h->d_byl)
  ExpectRegion* d_reg = nullptr;
  ByLenRec *d_piece = nullptr, *d_rec = nullptr;
  uint8_t* d_ch = nullptr;           // fast mode: the lane-chunk maps and scans, ch
  ByLenChunks ch{};
  uint32_t* d_btab = nullptr;
  double *d_cum = nullptr, *d_cum_halo = nullptr, *d_qmax = nullptr;
  double *d_cin = nullptr, *d_cout = nullptr;   // M and D at the cut, beside the relay's vectors
  double *d_hq = nullptr, *d_hrem = nullptr;   // the halo this shard reads, [I][H]
  uint32_t* d_hn = nullptr;
  double *d_oq = nullptr, *d_orem = nullptr;   // the halo this shard gives, [I][H of the shard in front]
  uint32_t* d_on = nullptr;
};

int bylength_impl(nghmm_t** hs, int n, int what, uint32_t K, const double* min_len, uint64_t n_regions,
                  const uint64_t* begin, const uint64_t* end, nghmm_bylength_stat* stats, const char* who) {
  uint64_t S_tot = 0;
  int rc;
  if ((rc = chain_check_loaded(hs, n, who, &S_tot))) return rc;
  if (what & ~NGHMM_BYLENGTH_MB) {
    set_error("%s: what = %d is not 0 or NGHMM_BYLENGTH_MB", who, what);
    return NGHMM_ERR_ARG;
  }
  const bool mb = (what & NGHMM_BYLENGTH_MB) != 0;
  if (K < 1 || K > kByLenMaxK || !min_len) {
    set_error("%s: n_lengths = %u with min_length %s: 1 to %u thresholds are needed", who, K,
              min_len ? "given" : "NULL", kByLenMaxK);
    return NGHMM_ERR_ARG;
  }
  for (uint32_t k = 0; k < K; ++k) {
    const double L = min_len[k];
    const bool ok = std::isfinite(L) && (mb ? L >= 0.0 : (L >= 1.0 && L == std::floor(L))) &&
                    (k == 0 || L > min_len[k - 1]);
    if (!ok) {
      set_error("%s: min_length[%u] = %g: thresholds are finite, strictly increasing and %s", who, k, L,
                mb ? ">= 0 Mb" : "whole numbers of sites >= 1");
      return NGHMM_ERR_ARG;
    }
  }
  const uint64_t I = hs[0]->I, R = n_regions;
  if ((rc = summary_check_regions(S_tot, I, R, begin, end, stats, nullptr, who))) return rc;
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  if (S_tot >= 0xfffffff0ull) {
    set_error("%s: %llu sites: the table of window ends holds 32-bit site indices", who,
              (unsigned long long)S_tot);
    return NGHMM_ERR_ARG;
  }
  // the distances of the whole site axis, cum and the chromosome ends
  std::vector<Shard> sh(n);
  std::vector<double> pos(S_tot), cum(S_tot);
  {
    uint64_t base = 0;
    for (int r = 0; r < n; ++r) {
      nghmm_t* h = hs[r];
      if ((rc = use_device(h))) return rc;
      sh[r].base = base;
      HIP_TRY(hipMemcpyAsync(pos.data() + base, h->d_pos, h->S * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
      HIP_TRY(sync_stream(h));
      base += h->S;
    }
  }
  std::vector<uint64_t> chrom_end(S_tot);   // the site behind the last of s's chromosome
  {
    double c = 0.0;
    for (uint64_t s = 0; s < S_tot; ++s) {
      c = (s == 0 || bounds_chrom_start(pos[s])) ? 0.0 : c + pos[s];
      cum[s] = c;
    }
    uint64_t e = S_tot;
    for (uint64_t s = S_tot; s-- > 0;) {
      chrom_end[s] = e;
      if (s == 0 || bounds_chrom_start(pos[s])) e = s;
    }
  }
  // b_k(a), global: non-decreasing in a inside a chromosome, so two pointers
  std::vector<uint64_t> bt((size_t)K * S_tot);
  for (uint32_t k = 0; k < K; ++k) {
    const double L = min_len[k];
    uint64_t b = 0;
    for (uint64_t a = 0; a < S_tot; ++a) {
      const uint64_t e = chrom_end[a];
      if (b < a) b = a;
      if (mb) {
        while (b < e && !(cum[b] - cum[a] >= L)) ++b;
      } else {
        // (a whole number of sites beyond the data has no window; the cast of one beyond 2^64 is
        // not defined)
        const uint64_t want = a + (L >= (double)S_tot ? S_tot : (uint64_t)L) - 1;
        b = want < e ? want : e;
      }
      bt[(size_t)k * S_tot + a] = b < e ? b : ~0ull;
    }
  }
  // how far every shard's windows reach into the shard behind it
  for (int r = 0; r < n; ++r) {
    const uint64_t lo = sh[r].base, hi = lo + hs[r]->S;
    uint64_t far = 0;
    for (uint32_t k = 0; k < K; ++k)
      for (uint64_t a = hi; a-- > lo;) {
        const uint64_t b = bt[(size_t)k * S_tot + a];
        if (b == ~0ull) continue;
        if (b < hi) break;   // (b_k is non-decreasing in a; a window that has no end lies further right)
        far = std::max(far, b - hi + 1);
      }
    sh[r].H = far;
    if (far && far > hs[r + 1]->S) {
      set_error("%s: a window that begins in shard %d reaches %llu sites past its end, but shard %d holds "
                "only %llu: a threshold may not reach past the next shard", who, r, (unsigned long long)far,
                r + 1, (unsigned long long)hs[r + 1]->S);
      return NGHMM_ERR_ARG;
    }
  }
  // cut the regions at the shard boundaries; number the pieces
  for (int r = 0; r < n; ++r) {
    Shard& x = sh[r];
    x.n_pieces = cut_regions(begin, end, R, x.base, x.base + hs[r]->S, fast ? hs[r]->fast.T : 0, x.reg, x.owner);
    x.rec.resize((size_t)I * x.reg.size() * K);
  }
  ChainRelay relay(hs, n);
  std::vector<double> carry((size_t)I * 2), qmax_h;
  std::vector<uint32_t> tab;
  std::vector<double> cum_il;
  // scratch, the tables, and the forward half: first shard to last
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t S = h->S, m = x.reg.size();
    const uint64_t J = fast ? h->fast.J : 0, Spad = fast ? J * h->fast.T : S;
    const uint64_t Hout = r > 0 ? sh[r - 1].H : 0;
    const uint64_t n_q = fast ? I * h->fast.C : I;
    Carver cv;
    cv.add(&x.d_reg, m);
    cv.add(&x.d_piece, I * x.n_pieces * K);
    cv.add(&x.d_rec, I * m * K);
    cv.add(&x.d_ch, fast ? bylength_chunk_bytes(I, J) : 0);
    cv.add(&x.d_btab, (uint64_t)K * Spad);
    cv.add(&x.d_cum, mb ? Spad : 0);
    cv.add(&x.d_cum_halo, mb ? x.H : 0);
    cv.add(&x.d_qmax, n_q);
    relay.add(cv, r);
    cv.add(&x.d_cin, I * 2);
    cv.add(&x.d_cout, I * 2);
    cv.add(&x.d_hq, I * x.H);
    cv.add(&x.d_hrem, I * x.H);
    cv.add(&x.d_hn, I * x.H);
    cv.add(&x.d_oq, I * Hout);
    cv.add(&x.d_orem, I * Hout);
    cv.add(&x.d_on, I * Hout);
    if ((rc = cv.reserve(h->d_byl))) return rc;
    const uint64_t cells = bylength_cell_count(fast ? &h->fast : nullptr, S, I);
    if ((rc = h->d_byl_cell.reserve(bylength_cell_bytes(cells)))) return rc;
    if (fast) x.ch = bylength_carve_chunks(x.d_ch, I, J);
    // the shard's tables: handle-local ends (S + h in the halo), tile-major in fast mode
    tab.assign((size_t)K * Spad, kByLenNone);
    if (mb) cum_il.assign(Spad, 0.0);
    const uint64_t T = fast ? h->fast.T : 1;
    for (uint64_t s = 0; s < S; ++s) {
      const uint64_t j = s / T, t = s % T;
      const uint64_t o = fast ? ((j >> 6) * T + t) * 64 + (j & 63) : s;
      for (uint32_t k = 0; k < K; ++k) {
        const uint64_t b = bt[(size_t)k * S_tot + x.base + s];
        if (b != ~0ull) tab[(size_t)k * Spad + o] = (uint32_t)(b - x.base);
      }
      if (mb) cum_il[o] = cum[x.base + s];
    }
    HIP_TRY(hipMemcpyAsync(x.d_btab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (mb) {
      HIP_TRY(hipMemcpyAsync(x.d_cum, cum_il.data(), Spad * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (x.H)
        HIP_TRY(hipMemcpyAsync(x.d_cum_halo, cum.data() + x.base + S, x.H * sizeof(double), hipMemcpyHostToDevice,
                               h->stream));
    }
    if (m) HIP_TRY(hipMemcpyAsync(x.d_reg, x.reg.data(), m * sizeof(ExpectRegion), hipMemcpyHostToDevice, h->stream));
    if ((rc = relay.forward(r))) return rc;   // (waits for the stream: tab and cum_il are free again)
  }
  // the backward half: last shard to first
  std::vector<double> halo_q, halo_rem;
  std::vector<uint32_t> halo_n;
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const bool last = r == n - 1;
    const uint64_t m = x.reg.size();
    if ((rc = use_device(h))) return rc;
    const uint64_t cells = bylength_cell_count(fast ? &h->fast : nullptr, h->S, I);
    const ByLenCells cl = bylength_carve(h->d_byl_cell.p, cells);
    const uint64_t n_q = fast ? I * h->fast.C : I;
    if (fast) {
      if ((rc = relay.backward_upload(r))) return rc;
      if (!last) {
        HIP_TRY(hipMemcpyAsync(x.d_cin, carry.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (x.H) {
          HIP_TRY(hipMemcpyAsync(x.d_hq, halo_q.data(), I * x.H * sizeof(double), hipMemcpyHostToDevice, h->stream));
          HIP_TRY(hipMemcpyAsync(x.d_hrem, halo_rem.data(), I * x.H * sizeof(double), hipMemcpyHostToDevice,
                                 h->stream));
          HIP_TRY(hipMemcpyAsync(x.d_hn, halo_n.data(), I * x.H * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 h->stream));
        }
      }
      ByLenHalo halo;
      halo.H = x.H;
      halo.q = x.d_hq;
      halo.rem = x.d_hrem;
      halo.n = x.d_hn;
      if ((rc = relay.backward_bounds(r, who))) return rc;
      if (!bylength_fast_cells(h->fast, h->stream, h->d_indF, h->d_alpha, r > 0, mb, cl, x.ch,
                               last ? nullptr : x.d_cin, r > 0 ? x.d_cout : nullptr, x.d_qmax) ||
          !bylength_fast_terms(h->fast, h->stream, mb, K, cl, x.d_btab, x.d_cum, x.d_cum_halo, halo, x.d_reg, m,
                               x.n_pieces, x.d_piece, x.d_rec))
        return fast_layout_error(h, who);
      if ((rc = relay.backward_end(r))) return rc;
      if (r > 0) {
        HIP_TRY(hipMemcpyAsync(carry.data(), x.d_cout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        const uint64_t Ho = sh[r - 1].H;
        if (Ho) {
          bylength_fast_halo(h->fast, h->stream, mb, cl, Ho, x.d_oq, x.d_on, x.d_orem);
          halo_q.resize((size_t)I * Ho);
          halo_rem.resize((size_t)I * Ho);
          halo_n.resize((size_t)I * Ho);
          HIP_TRY(hipMemcpyAsync(halo_q.data(), x.d_oq, I * Ho * sizeof(double), hipMemcpyDeviceToHost, h->stream));
          HIP_TRY(hipMemcpyAsync(halo_rem.data(), x.d_orem, I * Ho * sizeof(double), hipMemcpyDeviceToHost,
                                 h->stream));
          HIP_TRY(hipMemcpyAsync(halo_n.data(), x.d_on, I * Ho * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                 h->stream));
        }
      }
    } else {
      launch_bylength_exact(h->stream, h->d_eprob, h->d_pos, h->d_fw, h->S, I, h->d_indF, h->d_alpha, mb, K, cl,
                            x.d_btab, x.d_cum, x.d_reg, m, x.d_rec, x.d_qmax, h->d_flags);
      HIP_TRY(hipGetLastError());
      if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    }
    HIP_TRY(hipGetLastError());
    if (m)
      HIP_TRY(hipMemcpyAsync(x.rec.data(), x.d_rec, I * m * K * sizeof(ByLenRec), hipMemcpyDeviceToHost, h->stream));
    qmax_h.resize(n_q);
    HIP_TRY(hipMemcpyAsync(qmax_h.data(), x.d_qmax, n_q * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(sync_stream(h));
    h->byl_qmax = 0.0;
    for (double q : qmax_h) h->byl_qmax = std::max(h->byl_qmax, q);
  }
  // the shards' parts of every region in rank order, the first part's value first
  std::vector<uint8_t> seen(R, 0);
  for (int r = 0; r < n; ++r) {
    const Shard& x = sh[r];
    const uint64_t m = x.reg.size();
    for (uint64_t g = 0; g < m; ++g) {
      const uint64_t o = x.owner[g];
      for (uint64_t i = 0; i < I; ++i)
        for (uint32_t k = 0; k < K; ++k) {
          const ByLenRec& s = x.rec[(i * m + g) * K + k];
          nghmm_bylength_stat& d = stats[(i * R + o) * K + k];
          assign_or_add(!seen[o], [&](auto op) {
            op(d.tracts, s.tracts);
            op(d.length, s.length);
          });
        }
      seen[o] = 1;
    }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_ibd_by_length(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length,
                        uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end,
                        nghmm_bylength_stat* stats) {
  g_last_error.clear();
  return bylength_impl(&h, 1, what, n_lengths, min_length, n_regions, region_begin, region_end, stats,
                       "nghmm_ibd_by_length");
}

int nghmm_chain_ibd_by_length(nghmm_t** hs, int n_handles, int what, uint32_t n_lengths,
                              const double* min_length, uint64_t n_regions, const uint64_t* region_begin,
                              const uint64_t* region_end, nghmm_bylength_stat* stats) {
  g_last_error.clear();
  const char* who = "nghmm_chain_ibd_by_length";
  const int rc = chain_entry_check(hs, n_handles, who);
  if (rc) return rc;
  return bylength_impl(hs, n_handles, what, n_lengths, min_length, n_regions, region_begin, region_end, stats, who);
}

int nghmm_debug_bylength_qmax(nghmm_t* h, double* qmax) {
  g_last_error.clear();
  if (!h || !qmax) return NGHMM_ERR_ARG;
  *qmax = h->byl_qmax;
  return NGHMM_OK;
}
