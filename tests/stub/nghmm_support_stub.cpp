// nghmm_support_stub.cpp -- the tract-support entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it and
// tests/stub/nghmm_tracts_stub.cpp by tests/test_support_cpu.py).  A fixed formula per record, so
// that the host's --ibd_support writer can be checked line by line:
//   log_p_ibd = -inf where first_site % 7 == 0, else -(first_site + 1) / 8 - ind,
//   log_p_non = -3 n_sites - ind / 4,   post_min = 1 / (2 + first_site),
//   post_min_site = the range's last site
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

int nghmm_chain_tract_support(nghmm_t** hs, int n_handles, const nghmm_tract* tracts, uint64_t n,
                              nghmm_tract_score* out) {
  if (!hs || n_handles < 1 || hs[0]->g_n != n_handles) return NGHMM_ERR_ARG;
  uint64_t S = 0;
  for (int r = 0; r < n_handles; ++r) {
    if (!hs[r]->loaded) return NGHMM_ERR_ARG;
    S += hs[r]->S;
  }
  if (n == 0) return NGHMM_OK;
  if (!tracts || !out) return NGHMM_ERR_ARG;
  for (uint64_t k = 0; k < n; ++k) {
    const nghmm_tract& t = tracts[k];
    if (t.n_sites == 0 || t.ind >= hs[0]->I || t.first_site >= S || t.n_sites > S - t.first_site)
      return NGHMM_ERR_ARG;
    if (k > 0) {
      const nghmm_tract& p = tracts[k - 1];
      if (t.ind < p.ind || (t.ind == p.ind && t.first_site < p.first_site + p.n_sites)) return NGHMM_ERR_ARG;
    }
    out[k].log_p_ibd = t.first_site % 7 == 0 ? -INFINITY : -(double)(t.first_site + 1) / 8.0 - (double)t.ind;
    out[k].log_p_non = -3.0 * (double)t.n_sites - (double)t.ind / 4.0;
    out[k].post_min = 1.0 / (2.0 + (double)t.first_site);
    out[k].post_min_site = t.first_site + t.n_sites - 1;
  }
  return NGHMM_OK;
}

int nghmm_tract_support(nghmm_t* h, const nghmm_tract* tracts, uint64_t n, nghmm_tract_score* out) {
  return nghmm_chain_tract_support(&h, 1, tracts, n, out);
}

}  // extern "C"
