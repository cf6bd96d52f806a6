// nghmm_tracts_stub.cpp -- the IBD tract entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_tracts_cpu.py).  The records are those of the stand-in's filler path
// (nghmm_chain_viterbi: path[k] = k & 1 over [I][all sites]) with chromosome starts taken from
// the distances the host loaded, so that the host's BED writer can be checked against
// convert_ibd.pl's rule on the .ibd file the same run writes.  Nothing here is a fallback.
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

int nghmm_chain_ibd_tracts(nghmm_t** hs, int n, int source, double threshold, uint64_t min_sites,
                           nghmm_tract* out, uint64_t cap, uint64_t* n_total) {
  (void)threshold;
  if (!hs || n < 1 || hs[0]->g_n != n || !n_total || (cap && !out) ||
      source != NGHMM_TRACTS_VITERBI)
    return NGHMM_ERR_ARG;
  const uint64_t I = hs[0]->I;
  std::vector<char> cs;
  for (int r = 0; r < n; ++r) {
    if (!hs[r]->loaded) return NGHMM_ERR_ARG;
    for (uint64_t s = 0; s < hs[r]->S; ++s) cs.push_back(std::isinf(hs[r]->pos[s]) ? 1 : 0);
  }
  const uint64_t S = cs.size();
  cs[0] = 1;
  std::vector<nghmm_tract> all;
  for (uint64_t i = 0; i < I; ++i) {
    auto in = [&](uint64_t s) { return ((i * S + s) & 1) != 0; };
    for (uint64_t s = 0; s < S; ++s) {
      if (!in(s) || (s > 0 && in(s - 1) && !cs[s])) continue;
      uint64_t e = s;
      while (e + 1 < S && in(e + 1) && !cs[e + 1]) ++e;
      nghmm_tract t;
      std::memset(&t, 0, sizeof t);
      t.first_site = s;
      t.n_sites = e - s + 1;
      t.ind = (uint32_t)i;
      t.post_sum = 0.5 * (double)t.n_sites;
      if (t.n_sites >= min_sites) all.push_back(t);
    }
  }
  for (uint64_t k = 0; k < cap && k < all.size(); ++k) out[k] = all[k];
  *n_total = all.size();
  return NGHMM_OK;
}

int nghmm_ibd_tracts(nghmm_t* h, int source, double threshold, uint64_t min_sites,
                     nghmm_tract* out, uint64_t cap, uint64_t* n_total) {
  return nghmm_chain_ibd_tracts(&h, 1, source, threshold, min_sites, out, cap, n_total);
}

}  // extern "C"
