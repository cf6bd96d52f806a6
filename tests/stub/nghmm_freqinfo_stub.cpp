// nghmm_freqinfo_stub.cpp -- the frequency-information entries of include/nghmm.h for the CPU
// stand-in tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_freqinfo_cpu.py).  A fixed formula per global site s, so that the host's --freq_info
// writer can be checked line by line:
//   freq = 0 where s % 13 == 0, else 0.1 + (s % 50) / 100
//   ll = -inf where s % 11 == 0 (score, info and the curve NaN there), else -(s + 1) / 4
//   score = 3 - s / 8,   info = -1 where s % 3 == 0, else 4 + s
//   curve[s][k] = -inf where s % 7 == 0 and k == 0, else -(s + k) / 8 - levels[k]
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

int nghmm_chain_freq_info(nghmm_t** hs, int n_handles, uint32_t n_levels, const double* levels,
                          nghmm_freq_stat* stats, double* curve, double* cavity) {
  if (!hs || n_handles < 1 || hs[0]->g_n != n_handles) return NGHMM_ERR_ARG;
  uint64_t S = 0;
  for (int r = 0; r < n_handles; ++r) {
    if (!hs[r]->loaded) return NGHMM_ERR_ARG;
    S += hs[r]->S;
  }
  if (n_levels > 8 || (n_levels > 0) != (curve != nullptr) || (n_levels > 0 && !levels)) return NGHMM_ERR_ARG;
  if (!stats && !curve && !cavity) return NGHMM_ERR_ARG;
  for (uint32_t k = 0; k < n_levels; ++k)
    if (!(levels[k] >= 0.0 && levels[k] <= 1.0)) return NGHMM_ERR_ARG;
  for (uint64_t s = 0; s < S; ++s) {
    const bool dead = s % 11 == 0;
    if (stats) {
      stats[s].freq = s % 13 == 0 ? 0.0 : 0.1 + (double)(s % 50) / 100.0;
      stats[s].ll = dead ? -INFINITY : -(double)(s + 1) / 4.0;
      stats[s].score = dead ? NAN : 3.0 - (double)s / 8.0;
      stats[s].info = dead ? NAN : (s % 3 == 0 ? -1.0 : 4.0 + (double)s);
    }
    for (uint32_t k = 0; k < n_levels; ++k)
      curve[s * n_levels + k] = dead ? NAN
                                : (s % 7 == 0 && k == 0) ? -INFINITY
                                                         : -(double)(s + k) / 8.0 - levels[k];
  }
  if (cavity)
    for (uint64_t x = 0; x < hs[0]->I * S; ++x) cavity[x] = 0.5;
  return NGHMM_OK;
}

int nghmm_freq_info(nghmm_t* h, uint32_t n_levels, const double* levels, nghmm_freq_stat* stats,
                    double* curve, double* cavity) {
  return nghmm_chain_freq_info(&h, 1, n_levels, levels, stats, curve, cavity);
}

}  // extern "C"
