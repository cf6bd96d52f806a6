// nghmm_long_moments_stub.cpp -- nghmm_ibd_long_moments of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_long_moments_cpu.py).  The records are formulas of (individual, region, threshold,
// unit), restated in that test, so that the host's --ibd_long_moments writer can be checked byte for
// byte; some variances are 0, so that the writer's NA is reached.  Nothing here is a fallback.
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

int nghmm_ibd_long_moments(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, uint64_t n_regions,
                           const uint64_t* region_begin, const uint64_t* region_end, nghmm_long_moment_stat* stats) {
  if (!h || !h->loaded) return NGHMM_ERR_ARG;
  if (what & ~NGHMM_LONG_MOMENTS_MB) return NGHMM_ERR_ARG;
  if (n_lengths < 1 || n_lengths > 8 || !min_length) return NGHMM_ERR_ARG;
  if (n_regions == 0 || !stats || !region_begin || !region_end) return NGHMM_ERR_ARG;
  const bool mb = (what & NGHMM_LONG_MOMENTS_MB) != 0;
  for (uint32_t k = 0; k < n_lengths; ++k) {
    const double L = min_length[k];
    if (!std::isfinite(L) || (mb ? L < 0 : (L < 1 || L != std::floor(L))) || (k > 0 && !(L > min_length[k - 1])))
      return NGHMM_ERR_ARG;
  }
  for (uint64_t r = 0; r < n_regions; ++r)
    if (!(region_begin[r] < region_end[r]) || region_end[r] > h->S ||
        (r > 0 && region_begin[r] < region_end[r - 1]))
      return NGHMM_ERR_ARG;
  for (uint64_t i = 0; i < h->I; ++i)
    for (uint64_t r = 0; r < n_regions; ++r)
      for (uint32_t k = 0; k < n_lengths; ++k) {
        const double a = (double)region_begin[r], len = (double)(region_end[r] - region_begin[r]);
        nghmm_long_moment_stat& t = stats[(i * n_regions + r) * n_lengths + k];
        t.mean_a = (1.0 + (double)i) * len / (3.0 + min_length[k]) + (mb ? 0.5 : 0.25) * (double)(k + 1);
        t.mean_t = (1.0 + (double)i) / (2.0 + (double)i + a) + 1e-3 * (double)k;
        t.var_a = r % 3 == 2 ? 0.0 : 4.0 + (double)k + 0.5 * (double)i;
        t.cov_at = (k % 2 ? -0.5 : 0.75) / (1.0 + (double)i);
        t.var_t = (i % 2 == 1 && k == 0) ? 0.0 : 0.25 * (double)(k + 1) + 1e-2 * len;
      }
  return NGHMM_OK;
}

}  // extern "C"
