// capi_longest_host.hpp -- the host pieces that nghmm_ibd_longest (capi_longest.hip) and
// nghmm_ibd_count (capi_count.hip) share: the check of the thresholds, the whole site axis (the
// distances, cum, the chromosomes' edges), the table of window ends b_k(a), the regions' parts per
// chromosome, and the segments of a shard with the entries of every lane's ring.  One order of
// operations for both callers.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "capi_chain.hpp"
#include "kernels_bounds.hpp"
#include "kernels_longest.hpp"

namespace longest_host {

// 1 to kLongestMaxK thresholds, finite, strictly increasing; whole numbers of sites >= 1 or Mb >= 0
inline int check_lengths(bool mb, uint32_t K, const double* min_len, const char* who) {
  if (K < 1 || K > kLongestMaxK || !min_len) {
    set_error("%s: n_lengths = %u with min_length %s: 1 to %u thresholds are needed", who, K,
              min_len ? "given" : "NULL", kLongestMaxK);
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
  return NGHMM_OK;
}

inline int check_site_count(uint64_t S_tot, const char* who) {
  if (S_tot >= 0xfffffff0ull) {
    set_error("%s: %llu sites: the table of window ends holds 32-bit site indices", who,
              (unsigned long long)S_tot);
    return NGHMM_ERR_ARG;
  }
  return NGHMM_OK;
}

// the whole site axis of a chain (or of one handle)
struct Axis {
  std::vector<double> pos, cum;
  std::vector<uint64_t> base;                     // [n] the global index of every handle's site 0
  std::vector<uint64_t> chrom_begin, chrom_end;   // [S_tot]
  std::vector<uint32_t> bt;                       // [K][S_tot] b_k(a), global; kLongestNone: none
  std::vector<LongestPart> parts;                 // the regions' parts per chromosome, in site order
  std::vector<uint64_t> owner;                    // the region of every part
  bool is_start(uint64_t s) const { return s == 0 || bounds_chrom_start(pos[s]); }
};

// the distances of the whole site axis, cum and the chromosomes' edges
inline int read_axis(nghmm_t** hs, int n, uint64_t S_tot, Axis& ax) {
  int rc;
  ax.pos.resize(S_tot);
  ax.cum.resize(S_tot);
  ax.base.resize(n);
  {
    uint64_t base = 0;
    for (int r = 0; r < n; ++r) {
      nghmm_t* h = hs[r];
      if ((rc = use_device(h))) return rc;
      ax.base[r] = base;
      HIP_TRY(hipMemcpyAsync(ax.pos.data() + base, h->d_pos, h->S * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
      HIP_TRY(sync_stream(h));
      base += h->S;
    }
  }
  ax.chrom_begin.resize(S_tot);
  ax.chrom_end.resize(S_tot);
  {
    double c = 0.0;
    uint64_t b = 0;
    for (uint64_t s = 0; s < S_tot; ++s) {
      if (ax.is_start(s)) b = s;
      c = ax.is_start(s) ? 0.0 : c + ax.pos[s];
      ax.cum[s] = c;
      ax.chrom_begin[s] = b;
    }
    uint64_t e = S_tot;
    for (uint64_t s = S_tot; s-- > 0;) {
      ax.chrom_end[s] = e;
      if (ax.is_start(s)) e = s;
    }
  }
  return NGHMM_OK;
}

// b_k(a), global: non-decreasing in a inside a chromosome, so two pointers (capi_bylength.hip)
inline void window_table(Axis& ax, bool mb, uint32_t K, const double* min_len) {
  const uint64_t S_tot = ax.pos.size();
  ax.bt.resize((size_t)K * S_tot);
  for (uint32_t k = 0; k < K; ++k) {
    const double L = min_len[k];
    uint64_t b = 0;
    for (uint64_t a = 0; a < S_tot; ++a) {
      const uint64_t e = ax.chrom_end[a];
      if (b < a) b = a;
      if (mb) {
        while (b < e && !(ax.cum[b] - ax.cum[a] >= L)) ++b;
      } else {
        // (a whole number of sites beyond the data has no window; the cast of one beyond 2^64 is
        // not defined)
        const uint64_t want = a + (L >= (double)S_tot ? S_tot : (uint64_t)L) - 1;
        b = want < e ? want : e;
      }
      ax.bt[(size_t)k * S_tot + a] = b < e ? (uint32_t)b : kLongestNone;
    }
  }
}

// the regions' parts per chromosome, in site order
inline void region_parts(Axis& ax, uint64_t R, const uint64_t* begin, const uint64_t* end) {
  ax.parts.clear();
  ax.owner.clear();
  for (uint64_t g = 0; g < R; ++g)
    for (uint64_t x = begin[g]; x < end[g];) {
      const uint64_t e = std::min(end[g], ax.chrom_end[x]);
      ax.parts.push_back(LongestPart{x, e});
      ax.owner.push_back(g);
      x = e;
    }
}

// The segments of the shard [base, base + S) (its first site and every chromosome start) and, per
// (segment, threshold), the ring: the longest window b_k(a) - a + 1 of the starts of the segment and
// of the windows that begin in a shard before and reach into it.  Returns the entries in all.
inline uint64_t shard_rings(const Axis& ax, uint64_t base, uint64_t S, uint32_t K, std::vector<uint64_t>& seg,
                            std::vector<uint64_t>& roff, std::vector<uint32_t>& rcap) {
  const uint64_t S_tot = ax.pos.size();
  seg.clear();
  for (uint64_t s = 0; s < S; ++s)
    if (s == 0 || ax.is_start(base + s)) seg.push_back(s);
  seg.push_back(S);
  const uint64_t n_seg = seg.size() - 1;
  roff.resize(n_seg * K);
  rcap.resize(n_seg * K);
  uint64_t E = 0;
  for (uint64_t g = 0; g < n_seg; ++g) {
    const uint64_t A = base + seg[g], B = base + seg[g + 1];
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t* t = ax.bt.data() + (size_t)k * S_tot;
      uint64_t cap = 1;
      for (uint64_t a = A; a < B; ++a)
        if (t[a] != kLongestNone) cap = std::max<uint64_t>(cap, t[a] - a + 1);
      // the windows that begin in a shard before and reach into the segment (the starts without
      // a window are the chromosome's last: the ones with a window lie in front of them)
      for (uint64_t a = A; a-- > ax.chrom_begin[A];) {
        if (t[a] == kLongestNone) continue;
        if (t[a] < A) break;
        cap = std::max<uint64_t>(cap, t[a] - a + 1);
      }
      roff[g * K + k] = E;
      rcap[g * K + k] = (uint32_t)cap;
      E += cap;
    }
  }
  return E;
}

}  // namespace longest_host
