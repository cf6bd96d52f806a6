// capi_chain_host.hpp -- the host logic that the IBD entry points of the C ABI share and that needs
// no device: carving a scratch buffer into parts, the checks of tract records, cutting regions at a
// shard's boundaries, and the merge of the shards' parts.  No HIP header, so that
// tests/stub/chain_host_main.cpp checks it on the CPU; capi_chain.hpp has what queues work.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/nghmm.h"
#include "expect_region.hpp"

namespace capi {

void set_error(const char* fmt, ...);

// a carved scratch keeps every part 256-byte aligned
inline uint64_t align256(uint64_t n) { return (n + 255) & ~255ull; }

// One scratch buffer carved into parts.  Every part is registered once, with the pointer that is
// to receive it: add(&p, n) is n elements of p's type, rounded up by align256.  reserve(owner)
// reserves the sum on the owner (a DevScratch<uint8_t>, or anything with reserve(bytes) and p) and
// hands out the parts in the order they were registered; an empty part gets the address of the one
// behind it.
class Carver {
 public:
  template <typename T>
  void add(T** slot, uint64_t n) {
    parts_.push_back({slot, align256(n * sizeof(T)), [](void* s, uint8_t* p) {
                        *static_cast<T**>(s) = reinterpret_cast<T*>(p);
                      }});
    total_ += parts_.back().bytes;
  }
  uint64_t bytes() const { return total_; }
  template <typename Owner>
  int reserve(Owner& owner) {
    int rc;
    if ((rc = owner.reserve(total_))) return rc;
    uint8_t* p = owner.p;
    for (const Part& q : parts_) {
      q.set(q.slot, p);
      p += q.bytes;
    }
    return NGHMM_OK;
  }

 private:
  struct Part {
    void* slot;
    uint64_t bytes;
    void (*set)(void*, uint8_t*);
  };
  std::vector<Part> parts_;
  uint64_t total_ = 0;
};

// Record k of nghmm_tract_support's and nghmm_tract_bounds' input: inside the data's I individuals
// and S_tot sites, and behind record k - 1 in the order (ind, first_site) without overlapping it
inline int check_tract_record(const nghmm_tract* tracts, uint64_t k, uint64_t I, uint64_t S_tot, const char* who) {
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
  return NGHMM_OK;
}

// every record, in order: the first one that fails gives the message
inline int check_tract_records(const nghmm_tract* tracts, uint64_t n_rec, uint64_t I, uint64_t S_tot,
                               const char* who) {
  int rc;
  for (uint64_t k = 0; k < n_rec; ++k)
    if ((rc = check_tract_record(tracts, k, I, S_tot, who))) return rc;
  return NGHMM_OK;
}

// The parts that the shard of global sites [lo, hi) holds of the R regions [begin[k], end[k])
// (sorted, disjoint, global), in handle-local sites, and the region each part belongs to.  Returns
// the shard's pieces per individual, one per lane-chunk of T sites that a part touches (piece0
// numbers them); T = 0 (exact mode: no lanes) counts none.
inline uint64_t cut_regions(const uint64_t* begin, const uint64_t* end, uint64_t R, uint64_t lo, uint64_t hi,
                            uint64_t T, std::vector<nghmm::ExpectRegion>& parts, std::vector<uint64_t>& owner) {
  uint64_t n_pieces = 0;
  for (uint64_t k = 0; k < R; ++k) {
    if (end[k] <= lo || begin[k] >= hi) continue;
    nghmm::ExpectRegion g;
    g.begin = std::max(begin[k], lo) - lo;
    g.end = std::min(end[k], hi) - lo;
    g.piece0 = n_pieces;
    g.pad = 0;
    if (T) n_pieces += nghmm::expect_pieces(g.begin, g.end, T);
    parts.push_back(g);
    owner.push_back(k);
  }
  return n_pieces;
}

// A value that several shards hold parts of, the parts visited in rank order: the first part's
// fields are assigned, the later ones' added.  fields(op) calls op(dst, src) for every field.
template <typename Fields>
void assign_or_add(bool first, Fields fields) {
  if (first)
    fields([](double& d, double s) { d = s; });
  else
    fields([](double& d, double s) { d += s; });
}

}  // namespace capi
