// nghmm_expect_stub.cpp -- the path-expectation entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_expect_cpu.py).  The records are formulas of (individual, region) and of the site,
// restated in that test, so that the host's --ibd_expect writers can be checked byte for byte;
// log_p_path is -inf for every region that begins at a multiple of 7.  Nothing here is a fallback.
#include <cmath>
#include <cstdint>
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

int nghmm_chain_ibd_expect(nghmm_t** hs, int n, int what, uint64_t n_regions, const uint64_t* region_begin,
                           const uint64_t* region_end, nghmm_expect_region* regions,
                           nghmm_expect_site* sites) {
  if (!hs || n < 1 || !hs[0] || (n > 1 && hs[0]->g_n != n)) return NGHMM_ERR_ARG;
  if (what & ~NGHMM_EXPECT_VITERBI) return NGHMM_ERR_ARG;
  if ((regions == nullptr) != (n_regions == 0) || (!regions && !sites)) return NGHMM_ERR_ARG;
  if (n_regions && (!region_begin || !region_end)) return NGHMM_ERR_ARG;
  const uint64_t I = hs[0]->I;
  uint64_t S = 0;
  for (int r = 0; r < n; ++r) {
    if (!hs[r] || !hs[r]->loaded || hs[r]->I != I) return NGHMM_ERR_ARG;
    S += hs[r]->S;
  }
  for (uint64_t r = 0; r < n_regions; ++r)
    if (!(region_begin[r] < region_end[r]) || region_end[r] > S ||
        (r > 0 && region_begin[r] < region_end[r - 1]))
      return NGHMM_ERR_ARG;
  for (uint64_t i = 0; i < I; ++i)
    for (uint64_t r = 0; r < n_regions; ++r) {
      const double a = (double)region_begin[r], len = (double)(region_end[r] - region_begin[r]);
      nghmm_expect_region t;
      t.ibd = 0.25 * len + (double)i;
      t.starts = 1.0 / (1.0 + a);
      t.switches = 2.0 / (1.0 + a);
      t.ibd_mb = 0.001 * len;
      t.entropy = 1e-12 * (double)(i + 1) * len;
      t.log_p_path = !(what & NGHMM_EXPECT_VITERBI) ? 0.0
                     : region_begin[r] % 7 == 0     ? -HUGE_VAL
                                                    : -len / 8.0 - (double)i;
      regions[i * n_regions + r] = t;   // (writes every record the caller made room for)
    }
  if (sites)
    for (uint64_t s = 0; s < S; ++s)
      sites[s] = nghmm_expect_site{1.0 / (double)(s + 2), 1.0 / (double)(s + 3), 0.5 * (double)I,
                                   1e-3 * (double)s};
  return NGHMM_OK;
}

int nghmm_ibd_expect(nghmm_t* h, int what, uint64_t n_regions, const uint64_t* region_begin,
                     const uint64_t* region_end, nghmm_expect_region* regions, nghmm_expect_site* sites) {
  return nghmm_chain_ibd_expect(&h, 1, what, n_regions, region_begin, region_end, regions, sites);
}

}  // extern "C"
