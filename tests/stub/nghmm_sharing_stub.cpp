// nghmm_sharing_stub.cpp -- the pairwise sharing entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_sharing_cpu.py).  The matrices are those of the stand-in's filler path
// (nghmm_chain_viterbi: path[k] = k & 1 over [I][all sites]) and filler posteriors
// (nghmm_format_posteriors: 0.5 everywhere), so that the host's writer can be checked against the
// definitions applied to the .ibd file the same run writes.  Nothing here is a fallback.
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

int nghmm_chain_ibd_sharing(nghmm_t** hs, int n, int what, double threshold, uint64_t site_begin,
                            uint64_t site_end, uint64_t* vit_both, uint64_t* post_both,
                            double* post_prod) {
  if (!hs || n < 1 || !hs[0] || (n > 1 && hs[0]->g_n != n)) return NGHMM_ERR_ARG;
  if (what == 0 || (what & ~(NGHMM_SHARING_VITERBI | NGHMM_SHARING_POSTERIOR))) return NGHMM_ERR_ARG;
  const bool vit = what & NGHMM_SHARING_VITERBI, post = what & NGHMM_SHARING_POSTERIOR;
  if (vit != (vit_both != nullptr) || post != (post_both || post_prod)) return NGHMM_ERR_ARG;
  if (post_both && !(threshold > 0.0 && threshold <= 1.0)) return NGHMM_ERR_ARG;
  const uint64_t I = hs[0]->I;
  uint64_t S = 0;
  for (int r = 0; r < n; ++r) {
    if (!hs[r] || !hs[r]->loaded || hs[r]->I != I) return NGHMM_ERR_ARG;
    S += hs[r]->S;
  }
  if (!(site_begin < site_end) || site_end > S) return NGHMM_ERR_ARG;
  auto in = [&](uint64_t i, uint64_t s) { return ((i * S + s) & 1) != 0; };
  const double p = 0.5;
  for (uint64_t i = 0; i < I; ++i)
    for (uint64_t j = 0; j < I; ++j) {
      uint64_t v = 0, b = 0;
      double x = 0.0;
      for (uint64_t s = site_begin; s < site_end; ++s) {
        v += in(i, s) && in(j, s) ? 1 : 0;
        b += p >= threshold ? 1 : 0;
        x += p * p;
      }
      if (vit_both) vit_both[i * I + j] = v;
      if (post_both) post_both[i * I + j] = b;
      if (post_prod) post_prod[i * I + j] = x;
    }
  return NGHMM_OK;
}

int nghmm_ibd_sharing(nghmm_t* h, int what, double threshold, uint64_t site_begin, uint64_t site_end,
                      uint64_t* vit_both, uint64_t* post_both, double* post_prod) {
  return nghmm_chain_ibd_sharing(&h, 1, what, threshold, site_begin, site_end, vit_both, post_both,
                                 post_prod);
}

}  // extern "C"
