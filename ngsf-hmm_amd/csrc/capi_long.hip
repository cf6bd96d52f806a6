// capi_long.hip -- nghmm_ibd_long / nghmm_chain_ibd_long: the per-site posterior of lying in an IBD
// tract of at least L_k (kernels_long.hip).  The host checks the arguments, forms cum and the
// tables b_k(a) and lo_k(s) once per call over the whole site axis (two pointers per threshold),
// cuts the regions at the shard boundaries and numbers their pieces as capi_bylength.hip does; the
// device does the rest, one threshold at a time.  A chain is walked three times: the forward
// vectors from the first shard to the last; from the last to the first the backward vectors, the
// cells of every shard and the halo to the right -- Q and n of the first sites of the shard behind,
// as far as this shard's windows b_k reach; then from the first to the last the thresholds, with
// the halo to the left -- pi, the sum of ln rho and the blocked steps to the cut and T_k of the last
// sites of the shard in front, as far as this shard's windows lo_k reach, and its U at the cut.  A
// region across a cut is the sum of its parts in rank order; post and the site records are the
// concatenation of the shards'.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "../../include/nghmm_chain_long.h"
#include "capi_chain.hpp"
#include "kernels_bounds.hpp"
#include "kernels_long.hpp"

static_assert(sizeof(nghmm_long_region_stat) == sizeof(LongRec) &&
                  offsetof(nghmm_long_region_stat, sites) == offsetof(LongRec, sites) &&
                  offsetof(nghmm_long_region_stat, mb) == offsetof(LongRec, mb),
              "the device's record is nghmm_long_region_stat");
static_assert(sizeof(nghmm_long_site_stat) == sizeof(LongSite) &&
                  offsetof(nghmm_long_site_stat, sum) == offsetof(LongSite, sum) &&
                  offsetof(nghmm_long_site_stat, count) == offsetof(LongSite, count),
              "the device's record is nghmm_long_site_stat");

namespace {

struct Shard {
  uint64_t base = 0, H = 0, HL = 0;  // global index of its first site; sites of the halo right, left
  std::vector<ExpectRegion> reg;     // its parts of the regions, handle-local
  std::vector<uint64_t> owner;       // the region a part belongs to
  std::vector<LongRec> rec;          // [I][reg.size()][K]
  uint64_t n_pieces = 0;
  std::vector<double> hq;            // the halo to the right as the shard behind gave it, [I][H]
  std::vector<uint32_t> hn;
  // device scratch (h->d_long)
  ExpectRegion* d_reg = nullptr;
  LongRec *d_piece = nullptr, *d_rec = nullptr;
  LongSite* d_site = nullptr;
  uint8_t *d_ch = nullptr, *d_lch = nullptr;   // fast mode: the lane-chunk maps and scans
  ByLenChunks ch{};
  LongChunks lch{};
  uint32_t *d_btab = nullptr, *d_lotab = nullptr;
  double* d_qmax = nullptr;
  double *d_hq = nullptr, *d_oq = nullptr, *d_orem = nullptr;   // the halo to the right: read, given
  uint32_t *d_hn = nullptr, *d_on = nullptr;
  double *d_lpi = nullptr, *d_lqc = nullptr, *d_lsuf = nullptr, *d_lall = nullptr;   // to the left: read
  uint32_t* d_lnc = nullptr;
  double *d_opi = nullptr, *d_oqc = nullptr, *d_ot = nullptr, *d_oall = nullptr;     // ... given
  uint32_t* d_onc = nullptr;
};

int long_impl(nghmm_t** hs, int n, int what, uint32_t K, const double* min_len, double thr, uint64_t n_regions,
              const uint64_t* begin, const uint64_t* end, nghmm_long_region_stat* region_stats,
              nghmm_long_site_stat* site_stats, double* post, const char* who) {
  uint64_t S_tot = 0;
  int rc;
  if ((rc = chain_check_loaded(hs, n, who, &S_tot))) return rc;
  if (what & ~NGHMM_LONG_MB) {
    set_error("%s: what = %d is not 0 or NGHMM_LONG_MB", who, what);
    return NGHMM_ERR_ARG;
  }
  const bool mb = (what & NGHMM_LONG_MB) != 0;
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
  if (!(thr >= 0.0 && thr <= 1.0)) {
    set_error("%s: threshold = %g is not in [0, 1]", who, thr);
    return NGHMM_ERR_ARG;
  }
  if (!region_stats && !site_stats && !post) {
    set_error("%s: none of region_stats, site_stats and post is asked for", who);
    return NGHMM_ERR_ARG;
  }
  const uint64_t I = hs[0]->I, R = n_regions;
  if ((rc = summary_check_regions(S_tot, I, R, begin, end, region_stats, site_stats ? (void*)site_stats : (void*)post,
                                  who)))
    return rc;
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  if (S_tot >= 0xfffffff0ull) {
    set_error("%s: %llu sites: the tables of window ends hold 32-bit site indices", who,
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
  // b_k(a) and lo_k(s), global: both non-decreasing inside a chromosome, so two pointers each.
  // (a <= lo_k(s) iff len(a, s) >= L_k iff b_k(a) <= s: the same comparison forms both.)
  std::vector<uint64_t> bt((size_t)K * S_tot), lt((size_t)K * S_tot);
  for (uint32_t k = 0; k < K; ++k) {
    const double L = min_len[k];
    // (a whole number of sites beyond the data has no window; the cast of one beyond 2^64 is not defined)
    const uint64_t Ls = mb ? 0 : (L > (double)S_tot ? S_tot + 1 : (uint64_t)L);
    uint64_t b = 0;
    for (uint64_t a = 0; a < S_tot; ++a) {
      const uint64_t e = chrom_end[a];
      if (b < a) b = a;
      if (mb) {
        while (b < e && !(cum[b] - cum[a] >= L)) ++b;
      } else {
        const uint64_t want = a + (Ls > S_tot ? S_tot : Ls) - 1;
        b = want < e ? want : e;
      }
      bt[(size_t)k * S_tot + a] = b < e ? b : ~0ull;
    }
    uint64_t c0 = 0, a = 0;
    for (uint64_t s = 0; s < S_tot; ++s) {
      if (s == 0 || bounds_chrom_start(pos[s])) c0 = a = s;
      uint64_t lo = ~0ull;
      if (mb) {
        while (a < s && cum[s] - cum[a + 1] >= L) ++a;
        if (cum[s] - cum[a] >= L) lo = a;
      } else if (Ls <= S_tot && s + 1 >= c0 + Ls) {
        lo = s + 1 - Ls;
      }
      lt[(size_t)k * S_tot + s] = lo;
    }
  }
  // how far every shard's windows reach into the shard behind it and into the one in front of it
  for (int r = 0; r < n; ++r) {
    const uint64_t lo = sh[r].base, hi = lo + hs[r]->S;
    uint64_t far = 0, back = 0;
    for (uint32_t k = 0; k < K; ++k) {
      for (uint64_t a = hi; a-- > lo;) {
        const uint64_t b = bt[(size_t)k * S_tot + a];
        if (b == ~0ull) continue;
        if (b < hi) break;   // (b_k is non-decreasing in a; a window that has no end lies further right)
        far = std::max(far, b - hi + 1);
      }
      for (uint64_t s = lo; s < hi; ++s) {
        const uint64_t a = lt[(size_t)k * S_tot + s];
        if (a == ~0ull) continue;
        if (a >= lo) break;   // (lo_k is non-decreasing in s; a site without one lies further left)
        back = std::max(back, lo - a);
      }
    }
    sh[r].H = far;
    sh[r].HL = back;
    if (far && far > hs[r + 1]->S) {
      set_error("%s: a window that begins in shard %d reaches %llu sites past its end to the right, but shard "
                "%d holds only %llu: a threshold may not reach past the next shard", who, r,
                (unsigned long long)far, r + 1, (unsigned long long)hs[r + 1]->S);
      return NGHMM_ERR_ARG;
    }
    if (back && back > hs[r - 1]->S) {
      set_error("%s: a window that ends in shard %d reaches %llu sites past its first site to the left, but "
                "shard %d holds only %llu: a threshold may not reach past the previous shard", who, r,
                (unsigned long long)back, r - 1, (unsigned long long)hs[r - 1]->S);
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
  std::vector<uint32_t> tab, ltab;
  // scratch, the tables, and the forward half: first shard to last
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t S = h->S, m = x.reg.size();
    const uint64_t J = fast ? h->fast.J : 0, Spad = fast ? J * h->fast.T : S;
    const uint64_t Hout = r > 0 ? sh[r - 1].H : 0, HLout = r + 1 < n ? sh[r + 1].HL : 0;
    const uint64_t n_q = fast ? I * h->fast.C : I;
    Carver cv;
    cv.add(&x.d_reg, m);
    cv.add(&x.d_piece, I * x.n_pieces);
    cv.add(&x.d_rec, I * m * K);
    cv.add(&x.d_site, site_stats ? S * K : 0);
    cv.add(&x.d_ch, fast ? bylength_chunk_bytes(I, J) : 0);
    cv.add(&x.d_lch, fast ? long_chunk_bytes(I, J) : 0);
    cv.add(&x.d_btab, (uint64_t)K * Spad);
    cv.add(&x.d_lotab, (uint64_t)K * Spad);
    cv.add(&x.d_qmax, n_q);
    relay.add(cv, r);
    cv.add(&x.d_hq, I * x.H);
    cv.add(&x.d_hn, I * x.H);
    cv.add(&x.d_oq, I * Hout);
    cv.add(&x.d_orem, I * Hout);
    cv.add(&x.d_on, I * Hout);
    cv.add(&x.d_lpi, I * x.HL);
    cv.add(&x.d_lqc, I * x.HL);
    cv.add(&x.d_lnc, I * x.HL);
    cv.add(&x.d_lsuf, (uint64_t)K * I * x.HL);
    cv.add(&x.d_lall, (uint64_t)K * I);
    cv.add(&x.d_opi, I * HLout);
    cv.add(&x.d_oqc, I * HLout);
    cv.add(&x.d_onc, I * HLout);
    cv.add(&x.d_ot, I * HLout);
    cv.add(&x.d_oall, I);
    if ((rc = cv.reserve(h->d_long))) return rc;
    const uint64_t cells = bylength_cell_count(fast ? &h->fast : nullptr, S, I);
    if ((rc = h->d_byl_cell.reserve(bylength_cell_bytes(cells)))) return rc;
    if ((rc = h->d_long_cell.reserve(align256(long_cell_bytes(cells)) + (post ? I * S * sizeof(double) : 0))))
      return rc;
    if (fast) {
      x.ch = bylength_carve_chunks(x.d_ch, I, J);
      x.lch = long_carve_chunks(x.d_lch, I, J);
    }
    // the shard's tables: handle-local sites (S + h in either halo), tile-major in fast mode
    tab.assign((size_t)K * Spad, kByLenNone);
    ltab.assign((size_t)K * Spad, kByLenNone);
    const uint64_t T = fast ? h->fast.T : 1;
    for (uint64_t s = 0; s < S; ++s) {
      const uint64_t j = s / T, t = s % T;
      const uint64_t o = fast ? ((j >> 6) * T + t) * 64 + (j & 63) : s;
      for (uint32_t k = 0; k < K; ++k) {
        const uint64_t b = bt[(size_t)k * S_tot + x.base + s];
        if (b != ~0ull) tab[(size_t)k * Spad + o] = (uint32_t)(b - x.base);
        const uint64_t a = lt[(size_t)k * S_tot + x.base + s];
        if (a != ~0ull) ltab[(size_t)k * Spad + o] = (uint32_t)(a >= x.base ? a - x.base : S + (x.base - 1 - a));
      }
    }
    HIP_TRY(hipMemcpyAsync(x.d_btab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(x.d_lotab, ltab.data(), ltab.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                           h->stream));
    if (m) HIP_TRY(hipMemcpyAsync(x.d_reg, x.reg.data(), m * sizeof(ExpectRegion), hipMemcpyHostToDevice, h->stream));
    if ((rc = relay.forward(r))) return rc;   // (waits for the stream: tab and ltab are free again)
  }
  // the backward half and the cells: last shard to first
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t cells = bylength_cell_count(fast ? &h->fast : nullptr, h->S, I);
    const ByLenCells cl = bylength_carve(h->d_byl_cell.p, cells);
    const LongPlanes pl = long_carve(h->d_long_cell.p, cells);
    if (fast) {
      if ((rc = relay.backward_begin(r, who))) return rc;
      if (!bylength_fast_cells(h->fast, h->stream, h->d_indF, h->d_alpha, r > 0, false, cl, x.ch, nullptr, nullptr,
                               x.d_qmax, cl.d))
        return fast_layout_error(h, who);
      if ((rc = relay.backward_end(r))) return rc;
      const uint64_t Ho = r > 0 ? sh[r - 1].H : 0;
      if (Ho) {
        Shard& y = sh[r - 1];
        bylength_fast_halo(h->fast, h->stream, false, cl, Ho, x.d_oq, x.d_on, x.d_orem);
        y.hq.resize((size_t)I * Ho);
        y.hn.resize((size_t)I * Ho);
        HIP_TRY(hipMemcpyAsync(y.hq.data(), x.d_oq, I * Ho * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(y.hn.data(), x.d_on, I * Ho * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
      }
    } else {
      launch_bylength_exact(h->stream, h->d_eprob, h->d_pos, h->d_fw, h->S, I, h->d_indF, h->d_alpha, false, 0, cl,
                            nullptr, nullptr, nullptr, 0, nullptr, x.d_qmax, h->d_flags, cl.d);
      HIP_TRY(hipGetLastError());
      if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    }
    long_pack(h->stream, cells, cl, pl.rec);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sync_stream(h));
  }
  // the thresholds: first shard to last
  std::vector<double> l_pi, l_qc, l_t, l_suf, l_all((size_t)K * I), row;
  std::vector<uint32_t> l_nc;
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t S = h->S, m = x.reg.size();
    const uint64_t Spad = fast ? h->fast.J * h->fast.T : S;
    const uint64_t cells = bylength_cell_count(fast ? &h->fast : nullptr, S, I);
    const ByLenCells cl = bylength_carve(h->d_byl_cell.p, cells);
    const LongPlanes pl = long_carve(h->d_long_cell.p, cells);
    double* d_post = reinterpret_cast<double*>(h->d_long_cell.p + align256(long_cell_bytes(cells)));
    const uint64_t HLout = r + 1 < n ? sh[r + 1].HL : 0;
    ByLenHalo right;
    LongLeft left;
    if (x.H) {
      HIP_TRY(hipMemcpyAsync(x.d_hq, x.hq.data(), I * x.H * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(x.d_hn, x.hn.data(), I * x.H * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
      right.H = x.H;
      right.q = x.d_hq;
      right.n = x.d_hn;
    }
    if (r > 0) {
      left.has_left = true;
      left.H = x.HL;
      if (x.HL) {
        HIP_TRY(hipMemcpyAsync(x.d_lpi, l_pi.data(), I * x.HL * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(x.d_lqc, l_qc.data(), I * x.HL * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(x.d_lnc, l_nc.data(), I * x.HL * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(x.d_lsuf, l_suf.data(), (size_t)K * I * x.HL * sizeof(double), hipMemcpyHostToDevice,
                               h->stream));
      }
      HIP_TRY(hipMemcpyAsync(x.d_lall, l_all.data(), (size_t)K * I * sizeof(double), hipMemcpyHostToDevice,
                             h->stream));
      HIP_TRY(sync_stream(h));   // (the vectors are written again below)
      left.pi = x.d_lpi;
      left.qc = x.d_lqc;
      left.nc = x.d_lnc;
    }
    if (r + 1 < n) {
      l_pi.resize((size_t)I * HLout);
      l_qc.resize((size_t)I * HLout);
      l_nc.resize((size_t)I * HLout);
      l_t.resize((size_t)I * HLout);
      l_suf.assign((size_t)K * I * HLout, 0.0);
    }
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t* bk = x.d_btab + (size_t)k * Spad;
      const uint32_t* lk = x.d_lotab + (size_t)k * Spad;
      if (fast) {
        left.suf = x.d_lsuf + (size_t)k * I * x.HL;
        left.all = x.d_lall + (size_t)k * I;
        if (!long_fast_threshold(h->fast, h->stream, cl, x.ch, pl, x.lch, bk, lk, right, left) ||
            !long_fast_regions(h->fast, h->stream, cl, pl, r > 0, x.d_reg, m, x.n_pieces, x.d_piece, K, k, x.d_rec))
          return fast_layout_error(h, who);
        if (site_stats) long_fast_sites(h->fast, h->stream, pl, thr, K, k, x.d_site);
        if (post) long_fast_post(h->fast, h->stream, pl, d_post);
      } else {
        long_exact_threshold(h->stream, S, I, cl, pl, bk, lk);
        long_exact_regions(h->stream, S, I, h->d_pos, cl, pl, x.d_reg, m, K, k, x.d_rec);
        if (site_stats) long_exact_sites(h->stream, S, I, pl, thr, K, k, x.d_site);
        if (post) long_exact_post(h->stream, S, I, pl, d_post);
      }
      HIP_TRY(hipGetLastError());
      if (post)
        HIP_TRY(hipMemcpy2DAsync(post + ((size_t)k * I) * S_tot + x.base, S_tot * sizeof(double), d_post,
                                 S * sizeof(double), S * sizeof(double), I, hipMemcpyDeviceToHost, h->stream));
      if (r + 1 < n) {   // what the shard behind takes: T_k of the last sites, added from the cut outwards
        long_fast_halo_left(h->fast, h->stream, cl, pl, HLout, x.d_opi, x.d_oqc, x.d_onc, x.d_ot, x.d_oall);
        HIP_TRY(hipGetLastError());
        if (HLout) {
          HIP_TRY(hipMemcpyAsync(l_t.data(), x.d_ot, I * HLout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
          if (k == 0) {
            HIP_TRY(hipMemcpyAsync(l_pi.data(), x.d_opi, I * HLout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(l_qc.data(), x.d_oqc, I * HLout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(l_nc.data(), x.d_onc, I * HLout * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   h->stream));
          }
        }
        HIP_TRY(hipMemcpyAsync(l_all.data() + (size_t)k * I, x.d_oall, I * sizeof(double), hipMemcpyDeviceToHost,
                               h->stream));
        HIP_TRY(sync_stream(h));
        for (uint64_t i = 0; i < I; ++i) {
          double acc = 0.0;
          for (uint64_t hh = 0; hh < HLout; ++hh) {
            l_suf[((size_t)k * I + i) * HLout + hh] = acc;
            acc += l_t[i * HLout + hh];
          }
        }
      } else if (post) {
        HIP_TRY(sync_stream(h));   // (d_post is written again by the next threshold)
      }
    }
    if (m)
      HIP_TRY(hipMemcpyAsync(x.rec.data(), x.d_rec, I * m * K * sizeof(LongRec), hipMemcpyDeviceToHost, h->stream));
    if (site_stats)
      HIP_TRY(hipMemcpyAsync(site_stats + x.base * K, x.d_site, S * K * sizeof(LongSite), hipMemcpyDeviceToHost,
                             h->stream));
    HIP_TRY(sync_stream(h));
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
          const LongRec& s = x.rec[(i * m + g) * K + k];
          nghmm_long_region_stat& d = region_stats[(i * R + o) * K + k];
          assign_or_add(!seen[o], [&](auto op) {
            op(d.sites, s.sites);
            op(d.mb, s.mb);
          });
        }
      seen[o] = 1;
    }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_ibd_long(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, double threshold,
                   uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end,
                   nghmm_long_region_stat* region_stats, nghmm_long_site_stat* site_stats, double* post) {
  g_last_error.clear();
  return long_impl(&h, 1, what, n_lengths, min_length, threshold, n_regions, region_begin, region_end, region_stats,
                   site_stats, post, "nghmm_ibd_long");
}

int nghmm_chain_ibd_long(nghmm_t** hs, int n_handles, int what, uint32_t n_lengths, const double* min_length,
                         double threshold, uint64_t n_regions, const uint64_t* region_begin,
                         const uint64_t* region_end, nghmm_long_region_stat* region_stats,
                         nghmm_long_site_stat* site_stats, double* post) {
  g_last_error.clear();
  const char* who = "nghmm_chain_ibd_long";
  const int rc = chain_entry_check(hs, n_handles, who);
  if (rc) return rc;
  return long_impl(hs, n_handles, what, n_lengths, min_length, threshold, n_regions, region_begin, region_end,
                   region_stats, site_stats, post, who);
}
