// capi_genosmooth.hip -- nghmm_geno_smooth / nghmm_chain_geno_smooth: the genotype posteriors of
// every cell given all data of the individual, the calls, and their sums per site and per
// (individual, region) (kernels_genosmooth.hip).  The cavity weights come from cavity_walks
// (capi_cavity.hip), which nghmm_freq_info drives too; behind a shard's backward walk this file
// queues the cell pass and the two finish kernels and copies the shard's outputs to their place
// in the caller's arrays.  post, call and sites are the concatenation of the shards'; a region's
// parts are added on the host in rank order once every shard has answered.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_chain.hpp"
#include "kernels_genosmooth.hpp"

static_assert(sizeof(nghmm_geno_site_stat) == sizeof(GenoSiteRec) &&
                  offsetof(nghmm_geno_site_stat, n0) == offsetof(GenoSiteRec, n0) &&
                  offsetof(nghmm_geno_site_stat, n1) == offsetof(GenoSiteRec, n1) &&
                  offsetof(nghmm_geno_site_stat, n2) == offsetof(GenoSiteRec, n2) &&
                  offsetof(nghmm_geno_site_stat, het_prior) == offsetof(GenoSiteRec, het_prior) &&
                  offsetof(nghmm_geno_site_stat, ibd) == offsetof(GenoSiteRec, ibd) &&
                  offsetof(nghmm_geno_site_stat, alt_ibd) == offsetof(GenoSiteRec, alt_ibd),
              "the device records are nghmm_geno_site_stat");
static_assert(sizeof(nghmm_geno_region_stat) == sizeof(GenoRegionRec) &&
                  offsetof(nghmm_geno_region_stat, het) == offsetof(GenoRegionRec, het) &&
                  offsetof(nghmm_geno_region_stat, het_prior) == offsetof(GenoRegionRec, het_prior) &&
                  offsetof(nghmm_geno_region_stat, non_ibd) == offsetof(GenoRegionRec, non_ibd) &&
                  offsetof(nghmm_geno_region_stat, dosage) == offsetof(GenoRegionRec, dosage),
              "the device records are nghmm_geno_region_stat");

namespace {

// what one shard does: its regions (handle-local), their pieces, and where its bytes lie
struct Plan {
  uint64_t r0 = 0;                       // the first region of the call that the shard holds a part of
  std::vector<SummaryRegion> regs;       // (first: the region begins in this shard; the pass does not read it)
  std::vector<SummaryPiece> pieces;
  std::vector<uint32_t> seg_piece, piece_first;
  std::vector<nghmm_geno_region_stat> part;   // [I][regs.size()], the shard's answer
  uint64_t o_post, o_call, o_part, o_site, o_piece, o_reg, o_pc, o_segp, o_first, bytes;
};

int genosmooth_impl(nghmm_t** hs, int n, uint64_t R, const uint64_t* begin, const uint64_t* end,
                    nghmm_geno_region_stat* regions, nghmm_geno_site_stat* sites, double* post,
                    uint8_t* call, const char* who) {
  int rc;
  if ((rc = chain_check_loaded(hs, n, who))) return rc;
  if (!regions && !sites && !post && !call) {
    set_error("%s: regions, sites, post and call are all NULL: nothing is asked for", who);
    return NGHMM_ERR_ARG;
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
  // (the last argument: some output other than the regions, if there is one)
  const void* other = sites ? (const void*)sites : post ? (const void*)post : (const void*)call;
  if ((rc = summary_check_regions(S_tot, I, R, begin, end, regions, other, who))) return rc;
  // every shard's regions, cut into pieces at the segment edges of its own sites, in site order
  std::vector<Plan> plan(n);
  uint64_t r0 = 0;
  for (int q = 0; q < n; ++q) {
    Plan& p = plan[q];
    const uint64_t S = hs[q]->S, lo = base[q], hi = lo + S;
    const uint64_t nseg = summary_segments(S), nib = (I + 63) / 64;
    while (r0 < R && end[r0] <= lo) ++r0;
    p.r0 = r0;
    for (uint64_t r = r0; r < R && begin[r] < hi; ++r)
      p.regs.push_back({(begin[r] > lo ? begin[r] : lo) - lo, (end[r] < hi ? end[r] : hi) - lo, begin[r] >= lo});
    const uint64_t Rq = p.regs.size();
    summary_cut_pieces(p.regs, S, p.pieces, p.seg_piece, p.piece_first);
    p.part.resize((size_t)I * Rq);
    const uint64_t np = p.pieces.size();
    // posteriors [S][I][3] | calls [S][I] | site partials [nib][S] (nib > 1) | site records [S] |
    // piece records [np][I] | region records [I][Rq] | pieces [np] | segment starts | region starts
    p.o_post = 0;
    p.o_call = p.o_post + (post ? align256(S * I * 3 * sizeof(double)) : 0);
    p.o_part = p.o_call + (call ? align256(S * I) : 0);
    p.o_site = p.o_part + (sites && nib > 1 ? align256(nib * S * sizeof(GenoSiteRec)) : 0);
    p.o_piece = p.o_site + (sites ? align256(S * sizeof(GenoSiteRec)) : 0);
    p.o_reg = p.o_piece + align256(np * I * sizeof(GenoRegionRec));
    p.o_pc = p.o_reg + align256(Rq * I * sizeof(GenoRegionRec));
    p.o_segp = p.o_pc + align256(np * sizeof(SummaryPiece));
    p.o_first = p.o_segp + align256((nseg + 1) * 4);
    p.bytes = p.o_first + align256((Rq + 1) * 4);
  }
  auto shard_done = [&](int q, const double* d_cav, uint8_t* x) -> int {
    nghmm_t* h = hs[q];
    Plan& p = plan[q];
    const uint64_t S = h->S, nib = (I + 63) / 64, nseg = summary_segments(S);
    const uint64_t np = p.pieces.size(), Rq = p.regs.size();
    int rc;
    double* d_post = post ? reinterpret_cast<double*>(x + p.o_post) : nullptr;
    uint8_t* d_call = call ? x + p.o_call : nullptr;
    GenoSiteRec* d_site = reinterpret_cast<GenoSiteRec*>(x + p.o_site);
    GenoSiteRec* d_part = !sites ? nullptr : nib > 1 ? reinterpret_cast<GenoSiteRec*>(x + p.o_part) : d_site;
    GenoRegionRec* d_piece = reinterpret_cast<GenoRegionRec*>(x + p.o_piece);
    GenoRegionRec* d_reg = reinterpret_cast<GenoRegionRec*>(x + p.o_reg);
    SummaryPiece* d_pc = reinterpret_cast<SummaryPiece*>(x + p.o_pc);
    uint32_t* d_segp = reinterpret_cast<uint32_t*>(x + p.o_segp);
    uint32_t* d_first = reinterpret_cast<uint32_t*>(x + p.o_first);
    // (a shard that holds no piece leaves the three tables unwritten: the cell pass reads them only
    // under a non-null piece_out, which it then does not get, and no region is finished)
    if (np) {
      HIP_TRY(hipMemcpyAsync(d_pc, p.pieces.data(), np * sizeof(SummaryPiece), hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(d_segp, p.seg_piece.data(), (nseg + 1) * 4, hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(d_first, p.piece_first.data(), (Rq + 1) * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (!genosmooth_cells(h->stream, d_cav, fast ? fast_gl_lin(h->fast) : own_gl(h), !fast, h->d_freq, S, I,
                          d_pc, d_segp, d_post, d_call, d_part, np ? d_piece : nullptr) ||
        (Rq && !genosmooth_finish_regions(h->stream, d_piece, d_first, Rq, I, d_reg)) ||
        (sites && nib > 1 && !genosmooth_finish_sites(h->stream, d_part, nib, S, d_site))) {
      set_error("%s: a kernel launch failed", who);
      return NGHMM_ERR_HIP;
    }
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    if (post)
      HIP_TRY(hipMemcpyAsync(post + base[q] * I * 3, d_post, S * I * 3 * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
    if (call) HIP_TRY(hipMemcpyAsync(call + base[q] * I, d_call, S * I, hipMemcpyDeviceToHost, h->stream));
    if (sites)
      HIP_TRY(hipMemcpyAsync(sites + base[q], d_site, S * sizeof(GenoSiteRec), hipMemcpyDeviceToHost, h->stream));
    if (Rq)
      HIP_TRY(hipMemcpyAsync(p.part.data(), d_reg, Rq * I * sizeof(GenoRegionRec), hipMemcpyDeviceToHost,
                             h->stream));
    HIP_TRY(sync_stream(h));
    return NGHMM_OK;
  };
  if ((rc = cavity_walks(hs, n, &nghmm_handle::d_gsm, [&](int q) { return plan[q].bytes; }, shard_done, who)))
    return rc;
  // a region's parts in rank order, the first one's value first
  for (int q = 0; q < n; ++q) {
    const Plan& p = plan[q];
    const uint64_t Rq = p.regs.size();
    for (uint64_t i = 0; i < I; ++i)
      for (uint64_t k = 0; k < Rq; ++k) {
        nghmm_geno_region_stat& t = regions[i * R + p.r0 + k];
        const nghmm_geno_region_stat& a = p.part[i * Rq + k];
        if (p.regs[k].first) {
          t = a;
        } else {
          t.het += a.het;
          t.het_prior += a.het_prior;
          t.non_ibd += a.non_ibd;
          t.dosage += a.dosage;
        }
      }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_geno_smooth(nghmm_t* h, uint64_t n_regions, const uint64_t* region_begin,
                      const uint64_t* region_end, nghmm_geno_region_stat* regions,
                      nghmm_geno_site_stat* sites, double* post, uint8_t* call) {
  g_last_error.clear();
  return genosmooth_impl(&h, 1, n_regions, region_begin, region_end, regions, sites, post, call,
                         "nghmm_geno_smooth");
}

int nghmm_chain_geno_smooth(nghmm_t** hs, int n_handles, uint64_t n_regions,
                            const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_geno_region_stat* regions, nghmm_geno_site_stat* sites,
                            double* post, uint8_t* call) {
  g_last_error.clear();
  const char* who = "nghmm_chain_geno_smooth";
  const int rc = chain_entry_check(hs, n_handles, who);
  return rc ? rc : genosmooth_impl(hs, n_handles, n_regions, region_begin, region_end, regions, sites, post, call, who);
}
