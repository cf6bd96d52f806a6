// nghmm_count_stub.cpp -- nghmm_ibd_count of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_count_cpu.py).  The records are formulas of (individual, region, threshold, level,
// unit), restated in that test, so that the host's --ibd_count writer can be checked byte for byte.
// Nothing here is a fallback.
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

int nghmm_ibd_count(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, uint32_t n_counts,
                    uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end, double* prob) {
  if (!h || !h->loaded) return NGHMM_ERR_ARG;
  if (what & ~NGHMM_COUNT_MB) return NGHMM_ERR_ARG;
  if (n_lengths < 1 || n_lengths > 8 || !min_length) return NGHMM_ERR_ARG;
  if (n_counts < 1 || n_counts > 16) return NGHMM_ERR_ARG;
  if (n_regions == 0 || !prob || !region_begin || !region_end) return NGHMM_ERR_ARG;
  const bool mb = (what & NGHMM_COUNT_MB) != 0;
  for (uint32_t k = 0; k < n_lengths; ++k) {
    const double L = min_length[k];
    if (!std::isfinite(L) || (mb ? L < 0 : (L < 1 || L != std::floor(L))) || (k > 0 && !(L > min_length[k - 1])))
      return NGHMM_ERR_ARG;
  }
  for (uint64_t r = 0; r < n_regions; ++r)
    if (!(region_begin[r] < region_end[r]) || region_end[r] > h->S ||
        (r > 0 && region_begin[r] < region_end[r - 1]))
      return NGHMM_ERR_ARG;
  const uint64_t W = n_counts + 1;
  for (uint64_t i = 0; i < h->I; ++i)
    for (uint64_t r = 0; r < n_regions; ++r)
      for (uint32_t k = 0; k < n_lengths; ++k)
        for (uint64_t c = 0; c < W; ++c) {
          const double a = (double)region_begin[r], len = (double)(region_end[r] - region_begin[r]);
          // (writes every double the caller made room for)
          prob[((i * n_regions + r) * n_lengths + k) * W + c] =
              (1.0 + (double)i) / ((2.0 + (double)i + a) * (1.0 + min_length[k]) * (1.0 + (double)c)) +
              (mb ? 0.5 : 0.25) * 1e-3 * (double)(k + 1) + 1e-7 * len;
        }
  return NGHMM_OK;
}

}  // extern "C"
