// nghmm_info_stub.cpp -- the observed-information entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_info_cpu.py).  Individual i gets a deterministic record from its index and the
// stand-in's current parameters: lkl = -1000 - 3 i - F_i, g = (0.001 (i + 1), -0.002 (i + 1)),
// h_FF = -(40 + 10 i), h_AA = -(2 + i), h_FA = 1.5 + 0.5 i -- negative definite, except that
// individual 1's h_FF is positive (not definite: NA for its block) and individual 3's h_FA is 50
// (negative diagonal, negative determinant).  The bound cases come from the stand-in's
// parameters: next to tests/stub/nghmm_bounds_stub.cpp individual 2's alpha is 10 and individual
// 4's indF is 1e-6 after every iteration.  Nothing here is a fallback.
#include <cstdint>
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

int nghmm_chain_obs_info(nghmm_t** hs, int n, const double* F, const double* alpha, nghmm_info* out) {
  if (!hs || n < 1 || !hs[0] || (n > 1 && hs[0]->g_n != n) || !out || (F == nullptr) != (alpha == nullptr))
    return NGHMM_ERR_ARG;
  for (int r = 0; r < n; ++r)
    if (!hs[r] || !hs[r]->loaded) return NGHMM_ERR_ARG;
  for (uint64_t i = 0; i < hs[0]->I; ++i) {
    const double f = F ? F[i] : hs[0]->indF[i];
    nghmm_info r;
    r.lkl = -1000.0 - 3.0 * (double)i - f;
    r.g_F = 0.001 * (double)(i + 1);
    r.g_A = -0.002 * (double)(i + 1);
    r.h_FF = i == 1 ? 7.0 : -(40.0 + 10.0 * (double)i);
    r.h_AA = -(2.0 + (double)i);
    r.h_FA = i == 3 ? 50.0 : 1.5 + 0.5 * (double)i;
    out[i] = r;
  }
  return NGHMM_OK;
}

int nghmm_obs_info(nghmm_t* h, const double* F, const double* alpha, nghmm_info* out) {
  return nghmm_chain_obs_info(&h, 1, F, alpha, out);
}

}  // extern "C"
