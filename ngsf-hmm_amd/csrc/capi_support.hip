// capi_support.hip -- nghmm_tract_support / nghmm_chain_tract_support: the joint posterior of
// whole runs of sites (kernels_support.hip).  The host checks the records, which it has to read
// anyway, and while doing so cuts them at the shard boundaries and numbers their pieces (one per
// lane-chunk a range touches: a scan over the records); the device does the rest.  A chain is
// walked like nghmm_chain_sample_paths: the forward vectors from the first shard to the last, the
// backward vectors from the last to the first, I x 2 doubles per boundary; a range that crosses a
// boundary is the sum of its shards' parts in site order, added here.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_internal.hpp"
#include "kernels_sample.hpp"
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
  double *d_vin = nullptr, *d_vout = nullptr, *d_win = nullptr, *d_wout = nullptr;
};

int support_impl(nghmm_t** hs, int n, const nghmm_tract* tracts, uint64_t n_rec, nghmm_tract_score* out,
                 const char* who) {
  for (int r = 0; r < n; ++r)
    if (!hs[r] || !hs[r]->loaded) {
      set_error("%s: the handle holds no data", who);
      return NGHMM_ERR_ARG;
    }
  if (n_rec == 0) return NGHMM_OK;
  if (!tracts || !out) {
    set_error("%s: tracts %s, out %s: both are needed for n = %llu records", who, tracts ? "given" : "NULL",
              out ? "given" : "NULL", (unsigned long long)n_rec);
    return NGHMM_ERR_ARG;
  }
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if (n > 1 && !fast) {
    set_error("%s: site shards are a fast-mode layout", who);
    return NGHMM_ERR_ARG;
  }
  const uint64_t I = hs[0]->I;
  std::vector<Shard> sh(n);
  uint64_t S_tot = 0;
  for (int r = 0; r < n; ++r) {
    sh[r].base = S_tot;
    S_tot += hs[r]->S;
    sh[r].ioff.assign(I + 1, 0);
  }
  // the records: inside the data, ordered by (ind, first_site), disjoint within an individual
  for (uint64_t k = 0; k < n_rec; ++k) {
    const nghmm_tract& t = tracts[k];
    const unsigned long long kk = k, a = t.first_site, len = t.n_sites;
    if (t.n_sites == 0) {
      set_error("%s: record %llu has n_sites = 0", who, kk);
      return NGHMM_ERR_ARG;
    }
    if (t.ind >= I) {
      set_error("%s: record %llu has ind = %u, of %llu individuals", who, kk, t.ind, (unsigned long long)I);
      return NGHMM_ERR_ARG;
    }
    if (t.first_site >= S_tot || t.n_sites > S_tot - t.first_site) {
      set_error("%s: record %llu, sites [%llu, %llu + %llu), is outside the data's %llu sites", who, kk, a, a,
                len, (unsigned long long)S_tot);
      return NGHMM_ERR_ARG;
    }
    if (k > 0) {
      const nghmm_tract& p = tracts[k - 1];
      if (t.ind < p.ind || (t.ind == p.ind && t.first_site < p.first_site + p.n_sites)) {
        set_error("%s: record %llu (ind %u, first_site %llu) is out of order or overlaps record %llu: the "
                  "records are ordered by (ind, first_site) and disjoint within an individual", who, kk,
                  t.ind, a, kk - 1);
        return NGHMM_ERR_ARG;
      }
    }
  }
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
  int rc;
  std::vector<double> vec((size_t)I * 2);
  // scratch, and the forward half: first shard to last
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    if ((rc = use_device(h))) return rc;
    const uint64_t m = x.rec.size();
    const uint64_t b_rec = align256(m * sizeof(SupportRange)), b_off = align256((I + 1) * sizeof(uint64_t)),
                   b_piece = align256(x.n_pieces * sizeof(SupportScore)),
                   b_score = align256(m * sizeof(SupportScore)), b_vec = align256(I * 2 * sizeof(double));
    if ((rc = h->d_supp.reserve(b_rec + b_off + b_piece + b_score + 4 * b_vec))) return rc;
    uint8_t* p = h->d_supp.p;
    x.d_rec = reinterpret_cast<SupportRange*>(p);
    p += b_rec;
    x.d_ioff = reinterpret_cast<uint64_t*>(p);
    p += b_off;
    x.d_piece = reinterpret_cast<SupportScore*>(p);
    p += b_piece;
    x.d_score = reinterpret_cast<SupportScore*>(p);
    p += b_score;
    double** const vecs[4] = {&x.d_vin, &x.d_vout, &x.d_win, &x.d_wout};
    for (double** v : vecs) {
      *v = reinterpret_cast<double*>(p);
      p += b_vec;
    }
    if (m) HIP_TRY(hipMemcpyAsync(x.d_rec, x.rec.data(), m * sizeof(SupportRange), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(x.d_ioff, x.ioff.data(), (I + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = clear_flags(h))) return rc;
    if (fast) {
      if ((rc = ensure_emissions(h))) return rc;
      if (r > 0)
        HIP_TRY(hipMemcpyAsync(x.d_vin, vec.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (!sample_fast_forward(h->fast, h->stream, h->d_indF, h->d_alpha, r ? x.d_vin : nullptr, x.d_vout))
        return NGHMM_ERR_HIP;
      if (r + 1 < n)
        HIP_TRY(hipMemcpyAsync(vec.data(), x.d_vout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipGetLastError());
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
  }
  // the backward half: last shard to first
  for (int r = n - 1; r >= 0; --r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const bool last = r == n - 1;
    const uint64_t m = x.rec.size();
    if ((rc = use_device(h))) return rc;
    if (fast) {
      if (!last)
        HIP_TRY(hipMemcpyAsync(x.d_win, vec.data(), I * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (!support_fast_bounds(h->fast, h->stream, last ? nullptr : x.d_win, r > 0 ? x.d_wout : nullptr) ||
          !support_fast_walk(h->fast, h->stream, h->d_indF, h->d_alpha, x.d_ioff, x.d_rec, m, x.d_piece,
                             x.d_score)) {
        set_error("%s: the fast layout (T = %llu sites per lane) is not one the walk knows, or a kernel "
                  "launch failed", who, (unsigned long long)h->fast.T);
        return NGHMM_ERR_HIP;
      }
      if (r > 0)
        HIP_TRY(hipMemcpyAsync(vec.data(), x.d_wout, I * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
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
  if (!hs || n_handles < 1) {
    set_error("nghmm_chain_tract_support: no handles");
    return NGHMM_ERR_ARG;
  }
  if (n_handles > 1) {
    struct ChainCtx* cx = hs[0] ? hs[0]->chain : nullptr;
    bool ok = cx != nullptr;
    for (int r = 0; ok && r < n_handles; ++r)
      ok = hs[r] && hs[r]->chain == cx && hs[r]->fast.shard.rank == (uint32_t)r &&
           hs[r]->fast.shard.world == (uint32_t)n_handles;
    if (!ok) {
      set_error("nghmm_chain_tract_support: call nghmm_chain_setup on these handles first");
      return NGHMM_ERR_ARG;
    }
  }
  return support_impl(hs, n_handles, tracts, n, out, "nghmm_chain_tract_support");
}
