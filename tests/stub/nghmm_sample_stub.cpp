// nghmm_sample_stub.cpp -- the sampled-path entries of include/nghmm.h for the CPU stand-in
// tests/stub/nghmm_stub.cpp, TEST INFRASTRUCTURE ONLY (linked next to it by
// tests/test_sample_cpu.py).  Draw d fills a deterministic path -- path[d][i][s] = ((i + 1) * (s +
// 3 * d) / 3) & 1, runs of one to three sites -- and reports its statistics with chromosome starts
// taken from the distances the host loaded, so that the host's writers can be checked against the
// files they write.  Nothing here is a fallback.
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

int nghmm_chain_sample_paths(nghmm_t** hs, int n, uint64_t seed, uint32_t n_draws,
                             nghmm_path_stats* stats, uint32_t n_keep, uint8_t* paths) {
  (void)seed;
  if (!hs || n < 1 || (n > 1 && hs[0]->g_n != n) || n_draws == 0 || n_keep > n_draws ||
      (n_keep > 0) != (paths != nullptr))
    return NGHMM_ERR_ARG;
  const uint64_t I = hs[0]->I;
  std::vector<double> pos;
  for (int r = 0; r < n; ++r) {
    if (!hs[r]->loaded) return NGHMM_ERR_ARG;
    pos.insert(pos.end(), hs[r]->pos.begin(), hs[r]->pos.begin() + hs[r]->S);
  }
  const uint64_t S = pos.size();
  for (uint32_t d = 0; d < n_draws; ++d)
    for (uint64_t i = 0; i < I; ++i) {
      nghmm_path_stats st;
      std::memset(&st, 0, sizeof st);
      uint64_t run = 0;
      for (uint64_t s = 0; s < S; ++s) {
        const uint8_t z = (uint8_t)((((i + 1) * (s + 3 * d)) / 3) & 1);
        if (d < n_keep) paths[((uint64_t)d * I + i) * S + s] = z;
        const bool cont = z && run > 0 && !std::isinf(pos[s]);
        if (cont) st.ibd_mb += pos[s];
        run = z ? (cont ? run + 1 : 1) : 0;
        if (z && run == 1) ++st.n_tracts;
        if (run > st.longest_sites) st.longest_sites = run;
        st.ibd_sites += z;
      }
      if (stats) stats[(uint64_t)d * I + i] = st;
    }
  return NGHMM_OK;
}

int nghmm_sample_paths(nghmm_t* h, uint64_t seed, uint32_t n_draws, nghmm_path_stats* stats,
                       uint32_t n_keep, uint8_t* paths) {
  return nghmm_chain_sample_paths(&h, 1, seed, n_draws, stats, n_keep, paths);
}

}  // extern "C"
