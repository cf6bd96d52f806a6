// capi_support.hip -- nghmm_tract_support / nghmm_chain_tract_support: the joint posterior of
// whole runs of sites (kernels_support.hip).  The host checks the records, which it has to read
// anyway, and while doing so cuts them at the shard boundaries and numbers their pieces (one per
// lane-chunk a range touches: a scan over the records); the device does the rest.  A chain is
// walked like nghmm_chain_sample_paths: the forward vectors from the first shard to the last, the
// backward vectors from the last to the first, I x 2 doubles per boundary; a range that crosses a
// boundary is the sum of its shards' parts in site order, added here.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_chain.hpp"
#include "kernels_support.hpp"

static_assert(sizeof(nghmm_tract_score) == 32, "nghmm_tract_score is 32 bytes");
static_assert(sizeof(SupportScore) == sizeof(nghmm_tract_score), "the device's record is nghmm_tract_score");

namespace {

struct Shard {
  uint64_t base = 0;                  // global index of its first site
  std::vector<SupportRange> rec;      // its parts of the ranges, handle-local
  std::vector<uint64_t> owner, ioff;  // the range a part belongs to; [I + 1] offsets into rec
  std::vector<SupportScore> score;
  uint64_t n_pieces = 0;
  // device scratch (h->d_supp)
  SupportRange* d_rec = nullptr;
  uint64_t* d_ioff = nullptr;
  SupportScore *d_piece = nullptr, *d_score = nullptr;
};

int support_impl(nghmm_t** hs, int n, const nghmm_tract* tracts, uint64_t n_rec, nghmm_tract_score* out,
                 const char* who) {
  int rc;
  if ((rc = chain_check_loaded(hs, n, who))) return rc;
  if (n_rec == 0) return NGHMM_OK;
  if (!tracts || !out) {
    set_error("%s: tracts %s, out %s: both are needed for n = %llu records", who, tracts ? "given" : "NULL",
              out ? "given" : "NULL", (unsigned long long)n_rec);
    return NGHMM_ERR_ARG;
  }
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  const uint64_t I = hs[0]->I;
  std::vector<Shard> sh(n);
  uint64_t S_tot = 0;
  for (int r = 0; r < n; ++r) {
    sh[r].base = S_tot;
    S_tot += hs[r]->S;
    sh[r].ioff.assign(I + 1, 0);
  }
  // the records: inside the data, ordered by (ind, first_site), disjoint within an individual
  if ((rc = check_tract_records(tracts, n_rec, I, S_tot, who))) return rc;
  // cut at the shard boundaries; number the pieces
  for (int r = 0; r < n; ++r) {
    Shard& x = sh[r];
    const uint64_t lo = x.base, hi = x.base + hs[r]->S, T = fast ? hs[r]->fast.T : 1;
    for (uint64_t k = 0; k < n_rec; ++k) {
      const nghmm_tract& t = tracts[k];
      const uint64_t a = t.first_site, b = t.first_site + t.n_sites - 1;
      if (b < lo || a >= hi) continue;
      SupportRange R;
      R.first = std::max(a, lo) - lo;
      R.last = std::min(b, hi - 1) - lo;
      R.piece0 = x.n_pieces;
      R.cont = a < lo ? 1 : 0;
      if (fast) x.n_pieces += support_pieces(R.first, R.last, T);
      x.rec.push_back(R);
      x.owner.push_back(k);
      ++x.ioff[t.ind + 1];
    }
    for (uint64_t i = 0; i < I; ++i) x.ioff[i + 1] += x.ioff[i];
    x.score.resize(x.rec.size());
  }
  ChainRelay relay(hs, n);
  // scratch, and the forward half: first shard to last
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t m = x.rec.size();
    Carver cv;
    cv.add(&x.d_rec, m);
    cv.add(&x.d_ioff, I + 1);
    cv.add(&x.d_piece, x.n_pieces);
    cv.add(&x.d_score, m);
    relay.add(cv, r);
    if ((rc = cv.reserve(h->d_supp))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(x.d_rec, x.rec.data(), m * sizeof(SupportRange), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(x.d_ioff, x.ioff.data(), (I + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = relay.forward(r))) return rc;
  }
  // the backward half: last shard to first
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const uint64_t m = x.rec.size();
    if ((rc = use_device(h))) return rc;
    if (fast) {
      if ((rc = relay.backward_begin(r, who))) return rc;
      if (!support_fast_walk(h->fast, h->stream, h->d_indF, h->d_alpha, x.d_ioff, x.d_rec, m, x.d_piece, x.d_score))
        return fast_layout_error(h, who);
      if ((rc = relay.backward_end(r))) return rc;
    } else {
      launch_support_exact(h->stream, h->d_eprob, h->d_pos, h->d_fw, h->S, I, h->d_indF, h->d_alpha, x.d_ioff,
                           x.d_rec, x.d_score, h->d_flags);
      HIP_TRY(hipGetLastError());
      if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    }
    HIP_TRY(hipGetLastError());
    if (m)
      HIP_TRY(hipMemcpyAsync(x.score.data(), x.d_score, m * sizeof(SupportScore), hipMemcpyDeviceToHost,
                             h->stream));
    HIP_TRY(sync_stream(h));
  }
  // the shards' parts of every range in site order
  std::vector<uint8_t> seen(n_rec, 0);
  for (int r = 0; r < n; ++r) {
    const Shard& x = sh[r];
    for (size_t k = 0; k < x.rec.size(); ++k) {
      const SupportScore& s = x.score[k];
      nghmm_tract_score& o = out[x.owner[k]];
      if (!seen[x.owner[k]]) {
        seen[x.owner[k]] = 1;
        o.log_p_ibd = s.log_ibd;
        o.log_p_non = s.log_non;
        o.post_min = s.post_min;
        o.post_min_site = s.post_min_site + x.base;
      } else {
        o.log_p_ibd += s.log_ibd;
        o.log_p_non += s.log_non;
        if (s.post_min < o.post_min) {   // ascending sites: a tie stays with the lower one
          o.post_min = s.post_min;
          o.post_min_site = s.post_min_site + x.base;
        }
      }
    }
  }
  return NGHMM_OK;
}

}  // namespace

int nghmm_tract_support(nghmm_t* h, const nghmm_tract* tracts, uint64_t n, nghmm_tract_score* out) {
  g_last_error.clear();
  return support_impl(&h, 1, tracts, n, out, "nghmm_tract_support");
}

int nghmm_chain_tract_support(nghmm_t** hs, int n_handles, const nghmm_tract* tracts, uint64_t n,
                              nghmm_tract_score* out) {
  g_last_error.clear();
  const char* who = "nghmm_chain_tract_support";
  const int rc = chain_entry_check(hs, n_handles, who);
  return rc ? rc : support_impl(hs, n_handles, tracts, n, out, who);
}
