// nghmm_moments_stub.cpp -- the posterior-moment entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_moments_cpu.py).  The records are formulas of (individual, region, length), restated
// in that test, so that the host's --ibd_moments writer can be checked byte for byte; var_t is 0
// for every region that begins at a multiple of 5 and the Mb variance is 0 for individual 0, which
// the writer turns into NA correlations.  Nothing here is a fallback.
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

int nghmm_chain_ibd_moments(nghmm_t** hs, int n, int what, uint64_t n_regions, const uint64_t* region_begin,
                            const uint64_t* region_end, nghmm_moment_region* regions) {
  if (!hs || n < 1 || !hs[0] || (n > 1 && hs[0]->g_n != n)) return NGHMM_ERR_ARG;
  if (what & ~NGHMM_MOMENTS_MB) return NGHMM_ERR_ARG;
  if (n_regions == 0 || !regions || !region_begin || !region_end) return NGHMM_ERR_ARG;
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
  const bool mb = (what & NGHMM_MOMENTS_MB) != 0;
  for (uint64_t i = 0; i < I; ++i)
    for (uint64_t r = 0; r < n_regions; ++r) {
      const double a = (double)region_begin[r], len = (double)(region_end[r] - region_begin[r]);
      nghmm_moment_region t;
      t.mean_a = mb ? 0.001 * len + 1e-4 * (double)i : 0.25 * len + (double)i;
      t.mean_t = 1.0 / (1.0 + a) + (double)i;
      t.var_a = mb ? 1e-6 * len * (double)i : 0.5 * len + (double)i;
      t.var_t = region_begin[r] % 5 == 0 ? 0.0 : 0.125 * (double)(i + 1);
      t.cov_at = (mb ? -1e-4 : 0.01) * std::sqrt(len);
      regions[i * n_regions + r] = t;   // (writes every record the caller made room for)
    }
  return NGHMM_OK;
}

int nghmm_ibd_moments(nghmm_t* h, int what, uint64_t n_regions, const uint64_t* region_begin,
                      const uint64_t* region_end, nghmm_moment_region* regions) {
  return nghmm_chain_ibd_moments(&h, 1, what, n_regions, region_begin, region_end, regions);
}

}  // extern "C"
