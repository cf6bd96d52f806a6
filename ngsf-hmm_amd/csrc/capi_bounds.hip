// capi_bounds.hip -- nghmm_tract_bounds / nghmm_chain_tract_bounds: credible bounds of the two ends
// of an IBD tract (kernels_bounds.hip).  The host checks the records as capi_support.hip does,
// cuts the ranges of every pass at the shard boundaries and numbers their pieces (one per
// lane-chunk a range touches).  Three passes over the shards:
//   anchor  the cores (or the given anchors, as one-site cores): the pieces' minima in site order
//           give every record's anchor and P(z_c = 1 | y);
//   sum     the stretches between two limits (an anchor, or a chromosome's edge): ln prod g per
//           piece; the host adds them in site order -- within a shard and, in rank order, over
//           the shards -- into the two reaches and into the value at every piece's edge;
//   locate  the stretches again, every piece with its edge values: per level the first failing
//           site of every shard's part, of which the one nearest the anchor counts.
// A chain is prepared like nghmm_chain_tract_support: the forward vectors travel from the first
// shard to the last and the backward vectors from the last to the first, I x 2 doubles per
// boundary; after that every shard's boundary vectors (fast.bound) serve all three passes.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include <algorithm>
#include <limits>

#include "capi_chain.hpp"
#include "kernels_bounds.hpp"

static_assert(sizeof(nghmm_tract_bound) == 48, "nghmm_tract_bound is 48 bytes");

namespace {

constexpr double kNegInf = -std::numeric_limits<double>::infinity();

// a range of a pass in global sites
struct Range {
  uint32_t ind;
  uint64_t first, last;
  uint32_t nofact, search;
};

struct Shard {
  uint64_t base = 0;              // global index of its first site
  std::vector<BoundRange> rec;    // its parts of the ranges, handle-local
  std::vector<uint64_t> ioff;     // [I + 1] offsets into rec
  std::vector<int64_t> part;      // [ranges]: the range's part here, or -1
  uint64_t n_pieces = 0;
  std::vector<BoundOff> off;      // [n_pieces] locate pass, in
  std::vector<uint8_t> out;       // [n_pieces] records of the pass
};

// cut at the shard boundaries; number the pieces
void cut(nghmm_t** hs, int n, bool fast, uint64_t I, const std::vector<Range>& rg, std::vector<Shard>& sh) {
  for (int r = 0; r < n; ++r) {
    Shard& x = sh[r];
    const uint64_t lo = x.base, hi = x.base + hs[r]->S, T = fast ? hs[r]->fast.T : ~0ull;
    x.rec.clear();
    x.ioff.assign(I + 1, 0);
    x.part.assign(rg.size(), -1);
    x.n_pieces = 0;
    for (size_t k = 0; k < rg.size(); ++k) {
      const Range& g = rg[k];
      if (g.last < lo || g.first >= hi) continue;
      BoundRange R;
      R.first = std::max(g.first, lo) - lo;
      R.last = std::min(g.last, hi - 1) - lo;
      R.piece0 = x.n_pieces;
      R.nofact = (g.nofact && g.first >= lo) ? 1 : 0;
      R.search = g.search;
      x.n_pieces += support_pieces(R.first, R.last, T);
      x.part[k] = (int64_t)x.rec.size();
      x.rec.push_back(R);
      ++x.ioff[g.ind + 1];
    }
    for (uint64_t i = 0; i < I; ++i) x.ioff[i + 1] += x.ioff[i];
  }
}

// one pass over every shard that holds a range: x.out = its pieces; locate: one record per range
int run_pass(nghmm_t** hs, int n, bool fast, uint64_t I, std::vector<Shard>& sh, int pass,
             const BoundLevels& lv, const char* who) {
  const size_t rec_size = pass == 0 ? sizeof(BoundAnchor) : pass == 1 ? sizeof(BoundSum) : sizeof(BoundFail);
  int rc;
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    Shard& x = sh[r];
    const uint64_t m = x.rec.size();
    const uint64_t n_out = pass == 2 ? m : x.n_pieces;
    x.out.assign(n_out * rec_size, 0);
    if (m == 0) continue;
    if ((rc = use_device(h))) return rc;
    BoundRange* d_rec;
    uint64_t* d_ioff;
    BoundOff* d_off;
    uint8_t *d_pieces, *d_ranges;   // the pass's records per piece; locate: per range
    Carver cv;
    cv.add(&d_rec, m);
    cv.add(&d_ioff, I + 1);
    cv.add(&d_off, x.n_pieces);
    cv.add(&d_pieces, x.n_pieces * rec_size);
    cv.add(&d_ranges, pass == 2 ? m * rec_size : 0);
    if ((rc = cv.reserve(h->d_bnd))) return rc;
    void* d_out = d_pieces;
    void* d_fin = (pass == 2 && fast) ? d_ranges : d_out;   // (exact mode: a range is its one piece)
    HIP_TRY(hipMemcpyAsync(d_rec, x.rec.data(), m * sizeof(BoundRange), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_ioff, x.ioff.data(), (I + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if (pass == 2)
      HIP_TRY(hipMemcpyAsync(d_off, x.off.data(), x.n_pieces * sizeof(BoundOff), hipMemcpyHostToDevice, h->stream));
    if (fast) {
      const bool ok =
          pass == 0 ? bounds_fast_anchor(h->fast, h->stream, h->d_indF, h->d_alpha, d_ioff, d_rec,
                                         static_cast<BoundAnchor*>(d_out))
          : pass == 1 ? bounds_fast_sum(h->fast, h->stream, h->d_indF, h->d_alpha, d_ioff, d_rec,
                                        static_cast<BoundSum*>(d_out))
                      : bounds_fast_locate(h->fast, h->stream, h->d_indF, h->d_alpha, d_ioff, d_rec, d_off, lv,
                                           static_cast<BoundFail*>(d_out), m, static_cast<BoundFail*>(d_fin));
      if (!ok) return fast_layout_error(h, who);
    } else {
      if ((rc = clear_flags(h))) return rc;
      launch_bounds_exact(pass, h->stream, h->d_eprob, h->d_pos, h->d_fw, h->S, I, h->d_indF, h->d_alpha, d_ioff,
                          d_rec, d_off, lv, d_out, h->d_flags);
      HIP_TRY(hipGetLastError());
      if ((rc = check_flags(h))) return rc;   // (waits for the stream)
    }
    HIP_TRY(hipMemcpyAsync(x.out.data(), d_fin, n_out * rec_size, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(sync_stream(h));
  }
  return NGHMM_OK;
}

// the pieces of range k in site order: f(shard, slot)
template <typename F>
void for_pieces(nghmm_t** hs, int n, bool fast, const std::vector<Shard>& sh, size_t k, F f) {
  for (int r = 0; r < n; ++r) {
    const int64_t q = sh[r].part[k];
    if (q < 0) continue;
    const BoundRange& R = sh[r].rec[q];
    const uint64_t np = support_pieces(R.first, R.last, fast ? hs[r]->fast.T : ~0ull);
    for (uint64_t pc = 0; pc < np; ++pc) f(r, R.piece0 + pc);
  }
}

int bounds_impl(nghmm_t** hs, int n, const nghmm_tract* tracts, uint64_t n_rec, const uint64_t* anchor,
                const double* levels, uint32_t n_levels, nghmm_tract_bound* out, uint64_t* start,
                uint64_t* end, const char* who) {
  int rc;
  if ((rc = chain_check_loaded(hs, n, who))) return rc;
  if (n_rec == 0) return NGHMM_OK;
  if (n_levels < 1 || n_levels > BOUNDS_MAX_LEVELS) {
    set_error("%s: n_levels = %u: between 1 and %u levels", who, n_levels, BOUNDS_MAX_LEVELS);
    return NGHMM_ERR_ARG;
  }
  if (!tracts || !levels || !out || !start || !end) {
    set_error("%s: tracts %s, levels %s, out %s, start %s, end %s: all are needed for n = %llu records", who,
              tracts ? "given" : "NULL", levels ? "given" : "NULL", out ? "given" : "NULL",
              start ? "given" : "NULL", end ? "given" : "NULL", (unsigned long long)n_rec);
    return NGHMM_ERR_ARG;
  }
  BoundLevels lv{};
  lv.n = n_levels;
  for (uint32_t m = 0; m < n_levels; ++m) {
    if (!(levels[m] > 0.0 && levels[m] < 1.0)) {
      set_error("%s: levels[%u] = %g is outside the open range (0, 1)", who, m, levels[m]);
      return NGHMM_ERR_ARG;
    }
    if (m > 0 && !(levels[m] < levels[m - 1])) {
      set_error("%s: levels[%u] = %g after %g: the levels are strictly descending", who, m, levels[m],
                levels[m - 1]);
      return NGHMM_ERR_ARG;
    }
    lv.ln[m] = std::log(levels[m]);
  }
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  const uint64_t I = hs[0]->I;
  std::vector<Shard> sh(n);
  uint64_t S_tot = 0;
  for (int r = 0; r < n; ++r) {
    sh[r].base = S_tot;
    S_tot += hs[r]->S;
  }
  // the records, one by one: nghmm_tract_support's checks, then the anchor inside its core
  for (uint64_t k = 0; k < n_rec; ++k) {
    if ((rc = check_tract_record(tracts, k, I, S_tot, who))) return rc;
    const nghmm_tract& t = tracts[k];
    if (anchor && anchor[k] != UINT64_MAX && (anchor[k] < t.first_site || anchor[k] - t.first_site >= t.n_sites)) {
      const unsigned long long a = t.first_site, len = t.n_sites;
      set_error("%s: record %llu: the anchor %llu is outside its core, sites [%llu, %llu + %llu)", who,
                (unsigned long long)k, (unsigned long long)anchor[k], a, a, len);
      return NGHMM_ERR_ARG;
    }
  }
  // the boundary vectors of every shard: the forward half first shard to last, the backward half
  // last shard to first.  (The two vectors lie at the front of d_bnd, which run_pass carves anew:
  // by then fast.bound holds what they carried.  A backward half that cannot launch returns its
  // code without a message of this call's.)
  if (fast) {
    ChainRelay relay(hs, n, true);
    for (int r = 0; r < n; ++r) {
      nghmm_t* h = hs[r];
      if ((rc = use_device(h))) return rc;
      Carver cv;
      relay.add(cv, r);
      if ((rc = cv.reserve(h->d_bnd))) return rc;
      if ((rc = relay.forward(r))) return rc;
    }
    for (int r = n - 1; r >= 0; --r) {
      nghmm_t* h = hs[r];
      if ((rc = use_device(h))) return rc;
      if ((rc = relay.backward_begin(r, nullptr)) || (rc = relay.backward_end(r))) return rc;
      HIP_TRY(sync_stream(h));
    }
  } else {
    if ((rc = use_device(hs[0]))) return rc;
    if ((rc = ensure_emissions(hs[0]))) return rc;
  }
  // the chromosome starts, ascending, in global sites
  std::vector<uint64_t> chrom;
  {
    std::vector<double> pos;
    for (int r = 0; r < n; ++r) {
      nghmm_t* h = hs[r];
      if ((rc = use_device(h))) return rc;
      pos.resize(h->S);
      HIP_TRY(hipMemcpyAsync(pos.data(), h->d_pos, h->S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(sync_stream(h));
      for (uint64_t s = 0; s < h->S; ++s)
        if ((r == 0 && s == 0) || bounds_chrom_start(pos[s])) chrom.push_back(sh[r].base + s);
    }
  }
  // anchors
  std::vector<Range> rg(n_rec);
  for (uint64_t k = 0; k < n_rec; ++k) {
    const nghmm_tract& t = tracts[k];
    const bool given = anchor && anchor[k] != UINT64_MAX;
    rg[k] = Range{t.ind, given ? anchor[k] : t.first_site, given ? anchor[k] : t.first_site + t.n_sites - 1, 0, 0};
  }
  cut(hs, n, fast, I, rg, sh);
  if ((rc = run_pass(hs, n, fast, I, sh, 0, lv, who))) return rc;
  std::vector<double> lp1c(n_rec);
  for (uint64_t k = 0; k < n_rec; ++k) {
    double best = std::numeric_limits<double>::infinity(), p1 = 0.0;
    uint64_t site = rg[k].first;
    for_pieces(hs, n, fast, sh, k, [&](int r, uint64_t slot) {
      const BoundAnchor& a = reinterpret_cast<const BoundAnchor*>(sh[r].out.data())[slot];
      if (a.p0 < best) {   // ascending sites: a tie stays with the lower one
        best = a.p0;
        p1 = a.p1;
        site = a.site + sh[r].base;
      }
    });
    nghmm_tract_bound& o = out[k];
    o.anchor = site;
    o.post_anchor = p1;
    lp1c[k] = std::log(p1);
    // limits
    const size_t ci = std::upper_bound(chrom.begin(), chrom.end(), site) - chrom.begin();   // >= 1: site 0 starts one
    o.left_limit = chrom[ci - 1];
    o.right_limit = (ci < chrom.size() ? chrom[ci] : S_tot) - 1;
    o.log_reach_left = o.log_reach_right = 0.0;
  }
  for (uint64_t k = 0; k + 1 < n_rec; ++k)
    if (tracts[k].ind == tracts[k + 1].ind) {
      out[k].right_limit = std::min(out[k].right_limit, out[k + 1].anchor);
      out[k + 1].left_limit = std::max(out[k + 1].left_limit, out[k].anchor);
    }
  // the stretches: left of k (G), right of k (H); kl / kr: the records a stretch serves, or none
  rg.clear();
  std::vector<uint64_t> kl, kr;
  constexpr uint64_t none = ~0ull;
  for (uint64_t k = 0; k < n_rec; ++k) {
    const nghmm_tract_bound& o = out[k];
    const bool left_shared = k > 0 && tracts[k - 1].ind == tracts[k].ind && o.left_limit == out[k - 1].anchor;
    if (!left_shared && o.left_limit < o.anchor) {
      rg.push_back(Range{tracts[k].ind, o.left_limit, o.anchor, 1, 2});
      kl.push_back(none);
      kr.push_back(k);
    }
    const bool right_shared =
        k + 1 < n_rec && tracts[k + 1].ind == tracts[k].ind && o.right_limit == out[k + 1].anchor;
    if (right_shared || o.right_limit > o.anchor) {
      rg.push_back(Range{tracts[k].ind, o.anchor + 1, o.right_limit, 0, right_shared ? 3u : 1u});
      kl.push_back(k);
      kr.push_back(right_shared ? k + 1 : none);
    }
  }
  for (uint64_t k = 0; k < n_rec; ++k)
    for (uint32_t m = 0; m < n_levels; ++m) {
      start[k * n_levels + m] = out[k].anchor;
      end[k * n_levels + m] = out[k].anchor;
    }
  cut(hs, n, fast, I, rg, sh);
  if ((rc = run_pass(hs, n, fast, I, sh, 1, lv, who))) return rc;
  // the pieces in site order: H's running value through every piece's zero-free front, G's from
  // the far end; the two reaches
  for (int r = 0; r < n; ++r) sh[r].off.assign(sh[r].n_pieces, BoundOff{0.0, 0.0});
  std::vector<std::pair<int, uint64_t>> pcs;
  for (size_t g = 0; g < rg.size(); ++g) {
    pcs.clear();
    for_pieces(hs, n, fast, sh, g, [&](int r, uint64_t slot) { pcs.emplace_back(r, slot); });
    auto sum_of = [&](const std::pair<int, uint64_t>& pc) -> const BoundSum& {
      return reinterpret_cast<const BoundSum*>(sh[pc.first].out.data())[pc.second];
    };
    double pre = 0.0;
    bool dead = false;
    for (const auto& pc : pcs) {
      const BoundSum& s = sum_of(pc);
      sh[pc.first].off[pc.second].off_h = dead ? kNegInf : pre + s.leftrun;
      if (!dead) pre += s.leftrun;
      if (s.has_zero) dead = true;
    }
    if (kl[g] != none) out[kl[g]].log_reach_right = dead ? kNegInf : pre;
    if (kr[g] != none) {
      double suf = -lp1c[kr[g]];
      for (size_t q = pcs.size(); q-- > 0;) {
        sh[pcs[q].first].off[pcs[q].second].off_g = suf;
        suf += sum_of(pcs[q]).total;
      }
      // ln G(lo): lo is the neighbour's anchor, or the stretch's first site (which has no factor)
      const double lp1_lo = kl[g] != none ? lp1c[kl[g]] : sum_of(pcs[0]).lp1_first;
      const double reach = lp1_lo + suf;
      out[kr[g]].log_reach_left = reach == reach ? reach : kNegInf;
    }
  }
  if ((rc = run_pass(hs, n, fast, I, sh, 2, lv, who))) return rc;
  for (size_t g = 0; g < rg.size(); ++g) {
    auto fail_of = [&](int r) -> const BoundFail* {   // the stretch's part in shard r
      const int64_t q = sh[r].part[g];
      return q < 0 ? nullptr : reinterpret_cast<const BoundFail*>(sh[r].out.data()) + q;
    };
    if (kl[g] != none)   // H: the lowest failing site
      for (uint32_t m = 0; m < n_levels; ++m) {
        uint64_t e = out[kl[g]].right_limit;
        for (int r = 0; r < n; ++r) {
          const BoundFail* f = fail_of(r);
          if (f && f->h[m] != BOUNDS_NONE) {
            e = f->h[m] + sh[r].base - 1;
            break;
          }
        }
        end[kl[g] * n_levels + m] = e;
      }
    if (kr[g] != none)   // G: the highest failing site; the limit itself is the host's to judge
      for (uint32_t m = 0; m < n_levels; ++m) {
        const nghmm_tract_bound& o = out[kr[g]];
        uint64_t b = o.log_reach_left >= lv.ln[m] ? o.left_limit : o.left_limit + 1;
        for (int r = n - 1; r >= 0; --r) {
          const BoundFail* f = fail_of(r);
          if (f && f->g[m] != BOUNDS_NONE) {
            b = f->g[m] + sh[r].base + 1;
            break;
          }
        }
        start[kr[g] * n_levels + m] = b;
      }
  }
  // an anchor that cannot be IBD
  for (uint64_t k = 0; k < n_rec; ++k)
    if (!(out[k].post_anchor > 0.0)) {
      out[k].post_anchor = 0.0;
      out[k].log_reach_left = out[k].log_reach_right = kNegInf;
      for (uint32_t m = 0; m < n_levels; ++m) start[k * n_levels + m] = end[k * n_levels + m] = out[k].anchor;
    }
  return NGHMM_OK;
}

}  // namespace

int nghmm_tract_bounds(nghmm_t* h, const nghmm_tract* tracts, uint64_t n, const uint64_t* anchor,
                       const double* levels, uint32_t n_levels, nghmm_tract_bound* out, uint64_t* start,
                       uint64_t* end) {
  g_last_error.clear();
  return bounds_impl(&h, 1, tracts, n, anchor, levels, n_levels, out, start, end, "nghmm_tract_bounds");
}

int nghmm_chain_tract_bounds(nghmm_t** hs, int n_handles, const nghmm_tract* tracts, uint64_t n,
                             const uint64_t* anchor, const double* levels, uint32_t n_levels,
                             nghmm_tract_bound* out, uint64_t* start, uint64_t* end) {
  g_last_error.clear();
  const char* who = "nghmm_chain_tract_bounds";
  const int rc = chain_entry_check(hs, n_handles, who);
  return rc ? rc : bounds_impl(hs, n_handles, tracts, n, anchor, levels, n_levels, out, start, end, who);
}
