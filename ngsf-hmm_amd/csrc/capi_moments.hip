// capi_moments.hip -- nghmm_ibd_moments / nghmm_chain_ibd_moments: exact posterior means and
// covariances of (IBD sites or IBD Mb, number of tracts) per individual and region
// (kernels_moments.hip).  The host checks the regions, partitions the site axis into segments (the
// regions and the gaps between them), cuts the segments at the shard boundaries and at the
// lane-chunk edges into pieces and numbers them; the device walks, multiplies and -- for one
// handle -- closes.  A chain's shards each produce the centred jets of their parts of the segments;
// the host multiplies the parts across the cuts in rank order with the routine the device uses
// (kernels_moments.hpp: cjet_mul), then scans and closes once (moments_scan_close).
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_chain.hpp"
#include "kernels_moments.hpp"

static_assert(sizeof(nghmm_moment_region) == sizeof(MomentRec) &&
                  offsetof(nghmm_moment_region, mean_a) == offsetof(MomentRec, mean_a) &&
                  offsetof(nghmm_moment_region, mean_t) == offsetof(MomentRec, mean_t) &&
                  offsetof(nghmm_moment_region, var_a) == offsetof(MomentRec, var_a) &&
                  offsetof(nghmm_moment_region, cov_at) == offsetof(MomentRec, cov_at) &&
                  offsetof(nghmm_moment_region, var_t) == offsetof(MomentRec, var_t),
              "the device's record is nghmm_moment_region");

namespace {

struct Seg {
  uint64_t begin, end;
  int32_t region;   // or -1: a gap
  int32_t owner;    // a shard's part: the segment of the whole it belongs to (-1: padding)
};

// The tables of one handle (kernels_moments.hpp: MomentsTables) from its segments, which partition
// [0, J T): a wave whose 64 lane-chunks lie in one segment makes one piece, every other lane-chunk
// one piece per segment it touches.
struct Tables {
  std::vector<uint32_t> chunk_piece, seg_piece;
  std::vector<uint64_t> piece_end;
  std::vector<int32_t> seg_region;
};

void build_tables(const std::vector<Seg>& segs, uint64_t J, uint64_t T, Tables& tb) {
  const size_t n_seg = segs.size();
  tb.chunk_piece.assign(J + 1, 0);
  tb.seg_piece.assign(n_seg + 1, 0);
  tb.seg_region.resize(n_seg);
  tb.piece_end.clear();
  std::vector<uint8_t> seen(n_seg, 0);
  for (size_t k = 0; k < n_seg; ++k) tb.seg_region[k] = segs[k].region;
  size_t k = 0;   // the segment that holds the current site
  auto add = [&](uint64_t b, uint64_t e) {
    while (b >= segs[k].end) ++k;
    if (!seen[k]) {
      seen[k] = 1;
      tb.seg_piece[k] = (uint32_t)tb.piece_end.size();
    }
    tb.piece_end.push_back(e);
  };
  for (uint64_t w = 0; w < J / 64; ++w) {
    const uint64_t wb = w * 64 * T, we = wb + 64 * T;
    while (wb >= segs[k].end) ++k;
    if (we <= segs[k].end) {
      for (uint64_t l = 0; l < 64; ++l) tb.chunk_piece[w * 64 + l] = (uint32_t)tb.piece_end.size();
      add(wb, we);
      continue;
    }
    for (uint64_t l = 0; l < 64; ++l) {
      const uint64_t cb = wb + l * T, ce = cb + T;
      tb.chunk_piece[w * 64 + l] = (uint32_t)tb.piece_end.size();
      uint64_t b = cb;
      size_t kk = k;
      while (b < ce) {
        while (b >= segs[kk].end) ++kk;
        const uint64_t e = std::min(ce, segs[kk].end);
        add(b, e);
        b = e;
      }
    }
  }
  tb.chunk_piece[J] = (uint32_t)tb.piece_end.size();
  tb.seg_piece[n_seg] = (uint32_t)tb.piece_end.size();
  tb.piece_end.push_back(~0ull);   // the sentinel the walk reads behind a lane's last piece
}

int moments_impl(nghmm_t** hs, int n, int what, uint64_t n_regions, const uint64_t* begin,
                 const uint64_t* end, nghmm_moment_region* regions, const char* who) {
  uint64_t S_tot = 0;
  int rc;
  if ((rc = chain_check_loaded(hs, n, who, &S_tot))) return rc;
  if (what & ~NGHMM_MOMENTS_MB) {
    set_error("%s: what = %d is not 0 or NGHMM_MOMENTS_MB", who, what);
    return NGHMM_ERR_ARG;
  }
  if (n_regions == 0 || !begin || !end || !regions) {
    set_error("%s: n_regions = %llu, region_begin %s, region_end %s, regions %s: at least one region "
              "and all three arrays are needed", who, (unsigned long long)n_regions, begin ? "given" : "NULL",
              end ? "given" : "NULL", regions ? "given" : "NULL");
    return NGHMM_ERR_ARG;
  }
  const uint64_t I = hs[0]->I, R = n_regions;
  if ((rc = summary_check_regions(S_tot, I, R, begin, end, regions, nullptr, who))) return rc;
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  const bool mb = (what & NGHMM_MOMENTS_MB) != 0;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  if (!fast) {
    nghmm_t* h = hs[0];
    if ((rc = use_device(h))) return rc;
    uint64_t* d_reg;
    double* d_bw;
    MomentRec* d_out;
    Carver cv;
    cv.add(&d_reg, R * 2);
    cv.add(&d_bw, R * 2 * I);
    cv.add(&d_out, I * R);
    if ((rc = cv.reserve(h->d_mom))) return rc;
    std::vector<uint64_t> reg(R * 2);
    for (uint64_t k = 0; k < R; ++k) {
      reg[2 * k] = begin[k];
      reg[2 * k + 1] = end[k];
    }
    HIP_TRY(hipMemcpyAsync(d_reg, reg.data(), R * 2 * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = clear_flags(h))) return rc;
    launch_moments_exact(h->stream, h->d_eprob, h->d_pos, h->S, I, h->d_indF, h->d_alpha, mb, d_reg, R, d_bw,
                         d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(regions, d_out, I * R * sizeof(MomentRec), hipMemcpyDeviceToHost, h->stream));
    return check_flags(h);   // (waits for the stream)
  }
  // the segments of the whole: the regions and the gaps between them
  std::vector<Seg> whole;
  {
    uint64_t at = 0;
    for (uint64_t k = 0; k < R; ++k) {
      if (begin[k] > at) whole.push_back({at, begin[k], -1, 0});
      whole.push_back({begin[k], end[k], (int32_t)k, 0});
      at = end[k];
    }
    if (at < S_tot) whole.push_back({at, S_tot, -1, 0});
  }
  const uint32_t G = (uint32_t)whole.size();
  std::vector<int32_t> whole_region(G);
  for (uint32_t g = 0; g < G; ++g) whole_region[g] = whole[g].region;
  std::vector<double> segH, Fh;     // a chain: [G][27][I], the parts multiplied in rank order
  std::vector<uint8_t> have(n > 1 ? G : 0, 0);
  std::vector<double> part;
  if (n > 1) segH.resize((size_t)G * kCJetDoubles * I);
  uint64_t base = 0;
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    if ((rc = use_device(h))) return rc;
    const FastState& fs = h->fast;
    const uint64_t lo = base, hi = base + h->S, Spad = fs.J * fs.T;
    base = hi;
    if (fs.T == 0 || fs.C == 0 || fs.J != (uint64_t)fs.C * 64 || Spad < h->S) {
      set_error("%s: the fast layout (C = %u waves, T = %llu sites per lane) is not one the kernels walk", who,
                (unsigned)fs.C, (unsigned long long)fs.T);
      return NGHMM_ERR_HIP;
    }
    // this shard's parts of the segments, handle-local, and the padding behind its last site
    std::vector<Seg> segs;
    for (uint32_t g = 0; g < G; ++g) {
      if (whole[g].end <= lo || whole[g].begin >= hi) continue;
      segs.push_back({std::max(whole[g].begin, lo) - lo, std::min(whole[g].end, hi) - lo, whole[g].region,
                      (int32_t)g});
    }
    if (Spad > h->S) segs.push_back({h->S, Spad, -1, -1});
    Tables tb;
    build_tables(segs, fs.J, fs.T, tb);
    const uint32_t n_seg = (uint32_t)segs.size(), P = (uint32_t)(tb.piece_end.size() - 1);
    uint32_t *d_cp, *d_sp;
    uint64_t* d_pe;
    int32_t* d_sr;
    double *d_piece, *d_seg, *d_bw;
    MomentRec* d_out;
    Carver cv;
    cv.add(&d_cp, fs.J + 1);
    cv.add(&d_pe, (uint64_t)P + 1);
    cv.add(&d_sp, (uint64_t)n_seg + 1);
    cv.add(&d_sr, (uint64_t)n_seg);
    cv.add(&d_piece, I * P * kCJetDoubles);
    cv.add(&d_seg, I * n_seg * kCJetDoubles);
    cv.add(&d_bw, ((uint64_t)n_seg + 1) * 2 * I);
    cv.add(&d_out, I * R);
    if ((rc = cv.reserve(h->d_mom))) return rc;
    HIP_TRY(hipMemcpyAsync(d_cp, tb.chunk_piece.data(), (fs.J + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_pe, tb.piece_end.data(), ((uint64_t)P + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_sp, tb.seg_piece.data(), ((uint64_t)n_seg + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_sr, tb.seg_region.data(), (uint64_t)n_seg * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = clear_flags(h))) return rc;
    if ((rc = ensure_emissions(h))) return rc;
    const MomentsTables mt{d_cp, d_pe, d_sp, d_sr, P, n_seg};
    if (!moments_fast_segments(fs, h->stream, h->d_indF, h->d_alpha, mb, r > 0, mt, d_piece, d_seg)) {
      set_error("%s: the fast layout (C = %u waves, T = %llu sites per lane) is not one the kernels walk, or a "
                "kernel launch failed", who, (unsigned)fs.C, (unsigned long long)fs.T);
      return NGHMM_ERR_HIP;
    }
    if (n == 1) {
      launch_moments_close(h->stream, d_seg, d_bw, I, n_seg, d_sr, h->d_indF, R, d_out);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(regions, d_out, I * R * sizeof(MomentRec), hipMemcpyDeviceToHost, h->stream));
      return check_flags(h);   // (waits for the stream)
    }
    part.resize((size_t)n_seg * kCJetDoubles * I);
    HIP_TRY(hipMemcpyAsync(part.data(), d_seg, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (r == 0) {   // the chain's parameters are equal on every handle
      Fh.resize(I);
      HIP_TRY(hipMemcpyAsync(Fh.data(), h->d_indF, I * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    for (uint32_t k = 0; k < n_seg; ++k) {
      const int32_t g = segs[k].owner;
      if (g < 0) continue;
      const double* src = &part[(size_t)k * kCJetDoubles * I];
      double* dst = &segH[(size_t)g * kCJetDoubles * I];
      if (!have[g]) {
        std::memcpy(dst, src, (size_t)kCJetDoubles * I * sizeof(double));
        have[g] = 1;
      } else {
        for (uint64_t i = 0; i < I; ++i)
          cjet_store(dst + i, I, cjet_mul(cjet_load(dst + i, I), cjet_load(src + i, I)));
      }
    }
  }
  std::vector<double> bw(((size_t)G + 1) * 2 * I);
  std::vector<MomentRec> rec(R);
  for (uint64_t i = 0; i < I; ++i) {
    moments_scan_close(segH.data() + i, bw.data() + i, I, G, whole_region.data(), Fh[i], rec.data());
    std::memcpy(&regions[i * R], rec.data(), R * sizeof(MomentRec));
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_ibd_moments(nghmm_t* h, int what, uint64_t n_regions, const uint64_t* region_begin,
                      const uint64_t* region_end, nghmm_moment_region* regions) {
  g_last_error.clear();
  return moments_impl(&h, 1, what, n_regions, region_begin, region_end, regions, "nghmm_ibd_moments");
}

int nghmm_chain_ibd_moments(nghmm_t** hs, int n_handles, int what, uint64_t n_regions,
                            const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_moment_region* regions) {
  g_last_error.clear();
  const char* who = "nghmm_chain_ibd_moments";
  const int rc = chain_entry_check(hs, n_handles, who);
  return rc ? rc : moments_impl(hs, n_handles, what, n_regions, region_begin, region_end, regions, who);
}
