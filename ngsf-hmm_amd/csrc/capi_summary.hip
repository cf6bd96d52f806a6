// capi_summary.hip -- IBD per region and per site of one handle (nghmm_ibd_summary; the chain's
// merge is in capi_multi.hip): the regions cut into pieces at the segment edges on the host, one
// pass over the path and the posteriors and two small finish kernels on the device
// (kernels_summary.hip), the records copied out once.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_internal.hpp"

static_assert(sizeof(nghmm_region_stat) == sizeof(RegionRec) &&
                  offsetof(nghmm_region_stat, vit_sites) == offsetof(RegionRec, vit_sites) &&
                  offsetof(nghmm_region_stat, post_sites) == offsetof(RegionRec, post_sites) &&
                  offsetof(nghmm_region_stat, post_sum) == offsetof(RegionRec, post_sum) &&
                  offsetof(nghmm_region_stat, vit_mb) == offsetof(RegionRec, vit_mb),
              "the device records are nghmm_region_stat");
static_assert(sizeof(nghmm_site_stat) == sizeof(SiteRec) &&
                  offsetof(nghmm_site_stat, vit_count) == offsetof(SiteRec, vit_count) &&
                  offsetof(nghmm_site_stat, post_count) == offsetof(SiteRec, post_count) &&
                  offsetof(nghmm_site_stat, post_sum) == offsetof(SiteRec, post_sum),
              "the device records are nghmm_site_stat");
static_assert(NGHMM_SUMMARY_VITERBI == SUMMARY_VITERBI && NGHMM_SUMMARY_POSTERIOR == SUMMARY_POSTERIOR,
              "summary sources");

namespace capi {

int summary_check_source(nghmm_t* h, int what, double threshold, const char* who) {
  if (!h || !h->loaded) {
    set_error("%s: the handle holds no data", who);
    return NGHMM_ERR_ARG;
  }
  if (what == 0 || (what & ~(NGHMM_SUMMARY_VITERBI | NGHMM_SUMMARY_POSTERIOR))) {
    set_error("%s: what = %d is not a mask of NGHMM_SUMMARY_VITERBI and NGHMM_SUMMARY_POSTERIOR", who,
              what);
    return NGHMM_ERR_ARG;
  }
  if ((what & NGHMM_SUMMARY_VITERBI) && !h->path_decoded) {
    set_error("%s: no Viterbi decode since the data were loaded (run nghmm_viterbi first)", who);
    return NGHMM_ERR_ARG;
  }
  if ((what & NGHMM_SUMMARY_POSTERIOR) && !(threshold > 0.0 && threshold <= 1.0)) {
    set_error("%s: the posterior threshold %g is not in (0, 1]", who, threshold);
    return NGHMM_ERR_ARG;
  }
  return NGHMM_OK;
}

int summary_check_regions(uint64_t S, uint64_t I, uint64_t n_regions, const uint64_t* begin,
                          const uint64_t* end, const void* regions, const void* sites,
                          const char* who) {
  if ((regions == nullptr) != (n_regions == 0) || (n_regions && (!begin || !end))) {
    set_error("%s: regions, region_begin and region_end are NULL iff n_regions == 0", who);
    return NGHMM_ERR_ARG;
  }
  if (!regions && !sites) {
    set_error("%s: neither region nor site records are asked for", who);
    return NGHMM_ERR_ARG;
  }
  if (n_regions > S || n_regions >= (1ull << 31) / 2) {   // (disjoint and not empty: at most S)
    set_error("%s: %llu regions of %llu sites", who, (unsigned long long)n_regions, (unsigned long long)S);
    return NGHMM_ERR_ARG;
  }
  for (uint64_t r = 0; r < n_regions; ++r)
    if (!(begin[r] < end[r]) || end[r] > S || (r > 0 && begin[r] < end[r - 1])) {
      set_error("%s: region %llu = [%llu, %llu) is empty, ends behind the last of the %llu sites, or "
                "begins before region %llu ends (regions are sorted and do not overlap)",
                who, (unsigned long long)r, (unsigned long long)begin[r], (unsigned long long)end[r],
                (unsigned long long)S, (unsigned long long)(r ? r - 1 : 0));
      return NGHMM_ERR_ARG;
    }
  (void)I;
  return NGHMM_OK;
}

namespace {

size_t round_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

}  // namespace

void summary_cut_pieces(const std::vector<SummaryRegion>& regs, uint64_t S, std::vector<SummaryPiece>& pieces,
                        std::vector<uint32_t>& seg_piece, std::vector<uint32_t>& piece_first) {
  const uint64_t nseg = summary_segments(S), R = regs.size();
  pieces.clear();
  seg_piece.assign(nseg + 1, 0);
  piece_first.assign(R + 1, 0);
  for (uint64_t r = 0; r < R; ++r) {
    piece_first[r] = (uint32_t)pieces.size();
    for (uint64_t lo = regs[r].begin; lo < regs[r].end;) {
      const uint64_t edge = (lo / kSummarySeg + 1) * kSummarySeg;
      const uint64_t hi = edge < regs[r].end ? edge : regs[r].end;
      SummaryPiece p;
      p.lo = lo;
      p.hi = hi;
      p.region = (uint32_t)r;
      p.first = lo == regs[r].begin && regs[r].first ? 1u : 0u;
      ++seg_piece[lo / kSummarySeg + 1];
      pieces.push_back(p);
      lo = hi;
    }
  }
  piece_first[R] = (uint32_t)pieces.size();
  for (uint64_t g = 0; g < nseg; ++g) seg_piece[g + 1] += seg_piece[g];
}

int summary_last_state(nghmm_t* h, uint8_t* out) {
  int rc;
  if ((rc = use_device(h))) return rc;
  DevBuf<uint8_t> d;
  if ((rc = d.alloc(h->I))) return rc;
  launch_summary_last_state(h->stream, h->d_path_sites, h->S, h->I, d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d, h->I, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));
  return NGHMM_OK;
}

// Arguments checked by the caller: regs sorted, disjoint, inside [0, S).
int summary_to_host(nghmm_t* h, int what, double thr, const std::vector<SummaryRegion>& regs,
                    const uint8_t* prev_state, nghmm_region_stat* regions, nghmm_site_stat* sites) {
  int rc;
  if ((rc = use_device(h))) return rc;
  // fast mode: the site-major copy of the tile-major posteriors (kept until the next E-step)
  if ((what & NGHMM_SUMMARY_POSTERIOR) && (rc = ensure_marg(h))) return rc;
  const uint64_t S = h->S, I = h->I, nseg = summary_segments(S), nib = (I + 63) / 64, R = regs.size();
  // the pieces: every region cut at the segment edges, in site order
  std::vector<SummaryPiece> pieces;
  std::vector<uint32_t> seg_piece, piece_first;
  summary_cut_pieces(regs, S, pieces, seg_piece, piece_first);
  const uint64_t np = pieces.size();
  // d_summ: piece records [np][I] | region records [I][R] | site partials [nib][S] (nib > 1) |
  // site records [S] | pieces [np] | segment starts [nseg + 1] | region starts [R + 1] | state [I]
  const size_t o_piece = 0;
  const size_t o_reg = o_piece + np * I * sizeof(RegionRec);
  const size_t o_part = o_reg + R * I * sizeof(RegionRec);
  const size_t o_site = o_part + (sites && nib > 1 ? nib * S * sizeof(SiteRec) : 0);
  const size_t o_pc = o_site + (sites ? S * sizeof(SiteRec) : 0);
  const size_t o_segp = round_up(o_pc + np * sizeof(SummaryPiece), 16);
  const size_t o_first = round_up(o_segp + (nseg + 1) * 4, 16);
  const size_t o_prev = round_up(o_first + (R + 1) * 4, 16);
  if ((rc = h->d_summ.reserve(o_prev + I))) return rc;
  uint8_t* base = h->d_summ.p;
  RegionRec* d_piece = reinterpret_cast<RegionRec*>(base + o_piece);
  RegionRec* d_reg = reinterpret_cast<RegionRec*>(base + o_reg);
  SiteRec* d_site = reinterpret_cast<SiteRec*>(base + o_site);
  SiteRec* d_part = !sites ? nullptr : nib > 1 ? reinterpret_cast<SiteRec*>(base + o_part) : d_site;
  SummaryPiece* d_pc = reinterpret_cast<SummaryPiece*>(base + o_pc);
  uint32_t* d_segp = reinterpret_cast<uint32_t*>(base + o_segp);
  uint32_t* d_first = reinterpret_cast<uint32_t*>(base + o_first);
  uint8_t* d_prev = base + o_prev;
  if (np) HIP_TRY(hipMemcpyAsync(d_pc, pieces.data(), np * sizeof(SummaryPiece), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_segp, seg_piece.data(), (nseg + 1) * 4, hipMemcpyHostToDevice, h->stream));
  if (R) HIP_TRY(hipMemcpyAsync(d_first, piece_first.data(), (R + 1) * 4, hipMemcpyHostToDevice, h->stream));
  const bool vit = (what & NGHMM_SUMMARY_VITERBI) != 0;
  if (vit && prev_state) HIP_TRY(hipMemcpyAsync(d_prev, prev_state, I, hipMemcpyHostToDevice, h->stream));
  launch_summary_pass(h->stream, what, vit ? h->d_path_sites.p : nullptr,
                      (what & NGHMM_SUMMARY_POSTERIOR) ? h->d_marg.p : nullptr, h->d_pos,
                      vit && prev_state ? d_prev : nullptr, thr, S, I, d_pc, d_segp, d_piece, d_part);
  if (R) launch_summary_finish_regions(h->stream, d_piece, d_first, R, I, d_reg);
  if (sites && nib > 1) launch_summary_finish_sites(h->stream, d_part, nib, S, d_site);
  HIP_TRY(hipGetLastError());
  if (R) HIP_TRY(hipMemcpyAsync(regions, d_reg, R * I * sizeof(RegionRec), hipMemcpyDeviceToHost, h->stream));
  if (sites) HIP_TRY(hipMemcpyAsync(sites, d_site, S * sizeof(SiteRec), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(sync_stream(h));   // (also: the host vectors above were read)
  return NGHMM_OK;
}

}  // namespace capi

int nghmm_ibd_summary(nghmm_t* h, int what, double threshold, uint64_t n_regions,
                      const uint64_t* region_begin, const uint64_t* region_end,
                      nghmm_region_stat* regions, nghmm_site_stat* sites) {
  g_last_error.clear();
  int rc;
  if ((rc = summary_check_source(h, what, threshold, "nghmm_ibd_summary"))) return rc;
  if ((rc = summary_check_regions(h->S, h->I, n_regions, region_begin, region_end, regions, sites,
                                  "nghmm_ibd_summary")))
    return rc;
  std::vector<SummaryRegion> regs(n_regions);
  for (uint64_t r = 0; r < n_regions; ++r) regs[r] = {region_begin[r], region_end[r], true};
  return summary_to_host(h, what, threshold, regs, nullptr, regions, sites);
}
