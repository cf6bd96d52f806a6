// nghmm_summary_stub.cpp -- the region and site summary entries of include/nghmm.h for the CPU
// stand-in tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_summary_cpu.py).  The records are those of the stand-in's filler path
// (nghmm_chain_viterbi: path[k] = k & 1 over [I][all sites]) and filler posteriors
// (nghmm_format_posteriors: 0.5 everywhere) with the distances the host loaded, so that the host's
// writers can be checked against the definitions applied to the .ibd file the same run writes.
// Nothing here is a fallback.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nghmm.h"

// the stand-in's handle, token for token as tests/stub/nghmm_stub.cpp defines it
struct nghmm_handle {
  uint64_t I, S;
  int mode;
  bool packed, loading = false, loaded = false;
  std::vector<double> indF, alpha, freq, pos;
  std::vector<uint8_t> seen;  // per site: loaded exactly once
  nghmm_handle* parent = nullptr;
  int replicas = 0, g_n = 0;
  uint64_t checksum = 0;
};

extern "C" {

int nghmm_chain_ibd_summary(nghmm_t** hs, int n, int what, double threshold, uint64_t n_regions,
                            const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_region_stat* regions, nghmm_site_stat* sites) {
  if (!hs || n < 1 || !hs[0] || (n > 1 && hs[0]->g_n != n)) return NGHMM_ERR_ARG;
  if (what == 0 || (what & ~(NGHMM_SUMMARY_VITERBI | NGHMM_SUMMARY_POSTERIOR))) return NGHMM_ERR_ARG;
  if ((what & NGHMM_SUMMARY_POSTERIOR) && !(threshold > 0.0 && threshold <= 1.0)) return NGHMM_ERR_ARG;
  if ((regions == nullptr) != (n_regions == 0) || (!regions && !sites)) return NGHMM_ERR_ARG;
  if (n_regions && (!region_begin || !region_end)) return NGHMM_ERR_ARG;
  const uint64_t I = hs[0]->I;
  std::vector<double> d;
  for (int r = 0; r < n; ++r) {
    if (!hs[r] || !hs[r]->loaded || hs[r]->I != I) return NGHMM_ERR_ARG;
    d.insert(d.end(), hs[r]->pos.begin(), hs[r]->pos.end());
  }
  const uint64_t S = d.size();
  for (uint64_t r = 0; r < n_regions; ++r)
    if (!(region_begin[r] < region_end[r]) || region_end[r] > S ||
        (r > 0 && region_begin[r] < region_end[r - 1]))
      return NGHMM_ERR_ARG;
  const bool vit = what & NGHMM_SUMMARY_VITERBI, post = what & NGHMM_SUMMARY_POSTERIOR;
  auto in = [&](uint64_t i, uint64_t s) { return vit && ((i * S + s) & 1) != 0; };
  const double p = post ? 0.5 : 0.0;
  for (uint64_t i = 0; i < I; ++i)
    for (uint64_t r = 0; r < n_regions; ++r) {
      nghmm_region_stat t;
      std::memset(&t, 0, sizeof t);
      for (uint64_t s = region_begin[r]; s < region_end[r]; ++s) {
        t.vit_sites += in(i, s) ? 1 : 0;
        t.post_sites += post && p >= threshold ? 1 : 0;
        t.post_sum += p;
        if (s > region_begin[r] && in(i, s - 1) && in(i, s) && std::isfinite(d[s])) t.vit_mb += d[s];
      }
      regions[i * n_regions + r] = t;   // (writes every record the caller made room for)
    }
  if (sites)
    for (uint64_t s = 0; s < S; ++s) {
      nghmm_site_stat t;
      std::memset(&t, 0, sizeof t);
      for (uint64_t i = 0; i < I; ++i) {
        t.vit_count += in(i, s) ? 1 : 0;
        t.post_count += post && p >= threshold ? 1 : 0;
        t.post_sum += p;
      }
      sites[s] = t;
    }
  return NGHMM_OK;
}

int nghmm_ibd_summary(nghmm_t* h, int what, double threshold, uint64_t n_regions,
                      const uint64_t* region_begin, const uint64_t* region_end,
                      nghmm_region_stat* regions, nghmm_site_stat* sites) {
  return nghmm_chain_ibd_summary(&h, 1, what, threshold, n_regions, region_begin, region_end, regions,
                                 sites);
}

}  // extern "C"
