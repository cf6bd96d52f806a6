// capi_expect.hip -- nghmm_ibd_expect / nghmm_chain_ibd_expect: exact expectations over IBD paths
// (kernels_expect.hip).  The host checks the regions, cuts them at the shard boundaries and
// numbers their pieces (one per lane-chunk a region touches); the device does the rest.  A chain is
// walked like nghmm_chain_tract_support: the forward vectors from the first shard to the last, the
// backward vectors from the last to the first, I x 2 doubles per boundary; the decoded state at a
// shard's last site travels to the next shard as in nghmm_chain_ibd_summary; a region that
// crosses a boundary is the sum of its shards' parts in rank order, added here.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <cstddef>

#include "capi_chain.hpp"
#include "kernels_expect.hpp"

static_assert(sizeof(nghmm_expect_region) == sizeof(ExpectRec) &&
                  offsetof(nghmm_expect_region, ibd) == offsetof(ExpectRec, ibd) &&
                  offsetof(nghmm_expect_region, starts) == offsetof(ExpectRec, starts) &&
                  offsetof(nghmm_expect_region, switches) == offsetof(ExpectRec, switches) &&
                  offsetof(nghmm_expect_region, ibd_mb) == offsetof(ExpectRec, ibd_mb) &&
                  offsetof(nghmm_expect_region, entropy) == offsetof(ExpectRec, entropy) &&
                  offsetof(nghmm_expect_region, log_p_path) == offsetof(ExpectRec, log_p_path),
              "the device's record is nghmm_expect_region");
static_assert(sizeof(nghmm_expect_site) == sizeof(ExpectSite) &&
                  offsetof(nghmm_expect_site, on) == offsetof(ExpectSite, on) &&
                  offsetof(nghmm_expect_site, off) == offsetof(ExpectSite, off) &&
                  offsetof(nghmm_expect_site, ibd) == offsetof(ExpectSite, ibd) &&
                  offsetof(nghmm_expect_site, entropy) == offsetof(ExpectSite, entropy),
              "the device's record is nghmm_expect_site");

namespace {

struct Shard {
  uint64_t base = 0;                 // global index of its first site
  std::vector<ExpectRegion> reg;     // its parts of the regions, handle-local
  std::vector<uint64_t> owner;       // the region a part belongs to
  std::vector<ExpectRec> rec;        // [I][reg.size()]
  uint64_t n_pieces = 0;
  // device scratch (h->d_expt)
  ExpectRegion* d_reg = nullptr;
  ExpectRec *d_piece = nullptr, *d_rec = nullptr;
  ExpectSite* d_sites = nullptr;
  uint8_t* d_prev = nullptr;
};

int expect_impl(nghmm_t** hs, int n, int what, uint64_t n_regions, const uint64_t* begin,
                const uint64_t* end, nghmm_expect_region* regions, nghmm_expect_site* sites,
                const char* who) {
  uint64_t S_tot = 0;
  int rc;
  if ((rc = chain_check_loaded(hs, n, who, &S_tot))) return rc;
  if (what & ~NGHMM_EXPECT_VITERBI) {
    set_error("%s: what = %d is not 0 or NGHMM_EXPECT_VITERBI", who, what);
    return NGHMM_ERR_ARG;
  }
  const bool vit = (what & NGHMM_EXPECT_VITERBI) != 0;
  if (vit)
    for (int r = 0; r < n; ++r)
      if (!hs[r]->path_decoded) {
        set_error("%s: no Viterbi decode since the data were loaded (run nghmm_viterbi first)", who);
        return NGHMM_ERR_ARG;
      }
  const uint64_t I = hs[0]->I, R = n_regions;
  if ((rc = summary_check_regions(S_tot, I, R, begin, end, regions, sites, who))) return rc;
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  // cut at the shard boundaries; number the pieces
  std::vector<Shard> sh(n);
  for (int r = 0; r < n; ++r) {
    Shard& x = sh[r];
    x.base = r ? sh[r - 1].base + hs[r - 1]->S : 0;
    x.n_pieces = cut_regions(begin, end, R, x.base, x.base + hs[r]->S, fast ? hs[r]->fast.T : 0, x.reg, x.owner);
    x.rec.resize((size_t)I * x.reg.size());
  }
  ChainRelay relay(hs, n);
  std::vector<uint8_t> state(I);
  // scratch, and the forward half: first shard to last
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t m = x.reg.size();
    Carver cv;
    cv.add(&x.d_reg, m);
    cv.add(&x.d_piece, I * x.n_pieces);
    cv.add(&x.d_rec, I * m);
    cv.add(&x.d_sites, sites ? h->S : 0);
    cv.add(&x.d_prev, I);
    relay.add(cv, r);
    if ((rc = cv.reserve(h->d_expt))) return rc;
    if (sites && (rc = h->d_expt_cell.reserve(expect_cell_doubles(fast ? &h->fast : nullptr, h->S, I))))
      return rc;
    if (m) HIP_TRY(hipMemcpyAsync(x.d_reg, x.reg.data(), m * sizeof(ExpectRegion), hipMemcpyHostToDevice, h->stream));
    if ((rc = relay.forward(r))) return rc;
  }
  // the backward half: last shard to first
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const uint64_t m = x.reg.size();
    // the decoded state at the last site of the shard before (its device, its stream)
    if (vit && r > 0 && (rc = summary_last_state(hs[r - 1], state.data()))) return rc;
    if ((rc = use_device(h))) return rc;
    if (vit && r > 0) HIP_TRY(hipMemcpyAsync(x.d_prev, state.data(), I, hipMemcpyHostToDevice, h->stream));
    double* d_cell = sites ? h->d_expt_cell.p : nullptr;
    const uint8_t* path = vit ? h->d_path_sites.p : nullptr;
    if (fast) {
      if ((rc = relay.backward_begin(r, who))) return rc;
      if (!expect_fast_walk(h->fast, h->stream, h->d_indF, h->d_alpha, r > 0, path,
                            vit && r > 0 ? x.d_prev : nullptr, x.d_reg, m, x.n_pieces, x.d_piece, x.d_rec,
                            d_cell, x.d_sites))
        return fast_layout_error(h, who);
      if ((rc = relay.backward_end(r))) return rc;
    } else {
      launch_expect_exact(h->stream, h->d_eprob, h->d_pos, h->d_fw, h->S, I, h->d_indF, h->d_alpha, path,
                          x.d_reg, m, x.d_rec, d_cell, x.d_sites, h->d_flags);
      HIP_TRY(hipGetLastError());
      if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    }
    HIP_TRY(hipGetLastError());
    if (m)
      HIP_TRY(hipMemcpyAsync(x.rec.data(), x.d_rec, I * m * sizeof(ExpectRec), hipMemcpyDeviceToHost, h->stream));
    if (sites)
      HIP_TRY(hipMemcpyAsync(sites + x.base, x.d_sites, h->S * sizeof(ExpectSite), hipMemcpyDeviceToHost,
                             h->stream));
    HIP_TRY(sync_stream(h));
  }
  // the shards' parts of every region in rank order, the first part's value first
  std::vector<uint8_t> seen(R, 0);
  for (int r = 0; r < n; ++r) {
    const Shard& x = sh[r];
    const uint64_t m = x.reg.size();
    for (uint64_t k = 0; k < m; ++k) {
      const uint64_t g = x.owner[k];
      for (uint64_t i = 0; i < I; ++i) {
        const ExpectRec& s = x.rec[i * m + k];
        nghmm_expect_region& o = regions[i * R + g];
        assign_or_add(!seen[g], [&](auto op) {
          op(o.ibd, s.ibd);
          op(o.starts, s.starts);
          op(o.switches, s.switches);
          op(o.ibd_mb, s.ibd_mb);
          op(o.entropy, s.entropy);
          op(o.log_p_path, s.log_p_path);
        });
      }
      seen[g] = 1;
    }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_ibd_expect(nghmm_t* h, int what, uint64_t n_regions, const uint64_t* region_begin,
                     const uint64_t* region_end, nghmm_expect_region* regions, nghmm_expect_site* sites) {
  g_last_error.clear();
  return expect_impl(&h, 1, what, n_regions, region_begin, region_end, regions, sites, "nghmm_ibd_expect");
}

int nghmm_chain_ibd_expect(nghmm_t** hs, int n_handles, int what, uint64_t n_regions,
                           const uint64_t* region_begin, const uint64_t* region_end,
                           nghmm_expect_region* regions, nghmm_expect_site* sites) {
  g_last_error.clear();
  const char* who = "nghmm_chain_ibd_expect";
  const int rc = chain_entry_check(hs, n_handles, who);
  return rc ? rc : expect_impl(hs, n_handles, what, n_regions, region_begin, region_end, regions, sites, who);
}
