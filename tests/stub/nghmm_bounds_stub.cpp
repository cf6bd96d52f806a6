// nghmm_bounds_stub.cpp -- the CPU stand-in tests/stub/nghmm_stub.cpp with an EM iteration that
// runs two individuals into the bounds of their parameters, TEST INFRASTRUCTURE ONLY (linked IN
// PLACE of nghmm_stub.cpp by tests/test_info_cpu.py, which needs rows of PREFIX.indF.se whose
// parameters are on a bound; the host's own readers clamp what they are given to
// [1e-6, 1 - 1e-6], so only the library can put them there).  After every iteration individual
// 2's alpha is 10 (the box's upper end: its se_alpha and corr are NA, its se_indF is not) and
// individual 4's indF is 1e-6 (below the .indF file's NA limit of 1e-5: all three are NA).
// Everything else is nghmm_stub.cpp's, included here under another name for the one entry.
#define nghmm_chain_iter_em nghmm_chain_iter_em_plain
#include "nghmm_stub.cpp"
#undef nghmm_chain_iter_em

extern "C" int nghmm_chain_iter_em(nghmm_t** hs, int n, int freq_step, int indF_fixed, int alpha_fixed,
                                   double* ind_lkl, nghmm_mstep_stats* st) {
  const int rc = nghmm_chain_iter_em_plain(hs, n, freq_step, indF_fixed, alpha_fixed, ind_lkl, st);
  if (rc != NGHMM_OK) return rc;
  for (int r = 0; r < n; ++r) {
    if (hs[r]->I > 2) hs[r]->alpha[2] = 10.0;
    if (hs[r]->I > 4) hs[r]->indF[4] = 1e-6;
  }
  return NGHMM_OK;
}
