// kernels_longest.hpp -- the distribution of the longest IBD tract (kernels_longest.hip): host
// interface.  include/nghmm.h (nghmm_ibd_longest) has the definition of a record.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "glview.hpp"

namespace nghmm {

constexpr uint32_t kLongestMaxK = 8;
constexpr uint32_t kLongestNone = 0xffffffffu;   // in the table of window ends: no end in the chromosome

// laid out as nghmm_longest_stat (include/nghmm.h)
struct LongestRec {
  double p_any, p_none;
};
static_assert(sizeof(LongestRec) == 16, "nghmm_longest_stat is 16 bytes");

// a region's part inside one chromosome, GLOBAL sites (of the whole chain)
struct LongestPart {
  uint64_t begin, end;
};

// the per-cell planes the backward walk leaves, [S][I] each (40 bytes per cell): the four
// conditional steps r(k, l) and ln rho, 1.0 where the step is blocked (ln rho <= 0 is never 1.0)
struct LongestPlanes {
  double *r00, *r01, *r10, *r11, *lnrho;
};
inline uint64_t longest_plane_bytes(uint64_t S, uint64_t I) { return S * I * 5 * sizeof(double); }
inline LongestPlanes longest_carve(uint8_t* p, uint64_t S, uint64_t I) {
  double* d = reinterpret_cast<double*>(p);
  const uint64_t n = S * I;
  return LongestPlanes{d, d + n, d + 2 * n, d + 3 * n, d + 4 * n};
}

// what a forward lane hands across a cut, per individual: pi and Q at the handle's last site and
// per threshold the three masses, the oldest unresolved start (a GLOBAL site), the ring's live
// entries (cnt of them from slot hd of the last segment's ring)
struct LongestCarry {
  double pi0, pi1, q;
  double n[kLongestMaxK], v[kLongestMaxK], hit[kLongestMaxK];
  uint32_t ap[kLongestMaxK], cnt[kLongestMaxK], hd[kLongestMaxK];
};

// the rings of one handle: segment g, threshold k owns cap[g * K + k] entries (tau_a, Q_a) from
// entry off[g * K + k]; entry e of individual i lies at ring[e * I + i]
struct LongestRings {
  double2* ring;
  const uint64_t* off;
  const uint32_t* cap;
};

// the rings the shard before left (its last segment's): threshold k has cap[k] entries from off[k]
struct LongestRingIn {
  const double2* ring;
  uint64_t off[kLongestMaxK];
  uint32_t cap[kLongestMaxK];
};

// Fast mode, the backward walk: one lane per (individual, segment) right to left over the LINEAR
// likelihoods gl_lin [S][I] and the current frequencies, as freqinfo_fast_walks.  d_seg [n_seg + 1].
// Leaves the planes and, for every segment whose first site starts a chromosome (or is the data's
// first site: first_is_start), pi of that site in d_piseg [n_seg][I][2].  d_win [I][2]: beta at the
// handle's last site (null: (1, 1)); d_wout (may be null): the one at the last site of the shard
// before.  A NaN raises d_flags[FLAG_INVALID_LKL].
bool longest_fast_bwd(hipStream_t st, const GlView& gl_lin, const double* d_freq, const double* d_pos,
                      const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I, const double* d_indF,
                      const double* d_alpha, bool first_is_start, const double* d_win, double* d_wout,
                      const LongestPlanes& pl, double* d_piseg, int* d_flags);

// Exact mode: one lane per individual in log space through detmath.h over the LOG likelihoods; the
// same planes and d_piseg (site 0 is the data's first site)
void launch_longest_bwd_exact(hipStream_t st, const GlView& gl_log, const double* d_freq, const double* pos,
                              uint64_t S, uint64_t I, uint64_t n_seg, const double* d_indF, const double* d_alpha,
                              const LongestPlanes& pl, double* d_piseg, int* d_flags);

// The forward walk, one lane per (individual, segment) left to right: pi, and per part and
// threshold (N, V, Hit, ring).  base: the global index of the handle's site 0; d_btab [K][S_tot]
// GLOBAL window ends; d_part [n_part] sorted; d_rec [I][n_part][K] (a part's record is written by the
// handle that holds its last site).  d_cin (null: none, or the handle's first site starts a
// chromosome) / d_cout [I] (may be null): the lane state across the cuts.  exact: W through det_exp.
// split: a lane per (individual, segment, threshold) instead of the K thresholds as a loop inside
// a lane; the same bits either way.  *d_overflow is raised if a ring is ever full at a push (the
// host's sizing would be wrong): the records are then not to be used.
bool longest_fwd(hipStream_t st, bool exact, bool split, const uint64_t* d_seg, uint64_t n_seg,
                 uint64_t S, uint64_t I, uint64_t base, uint64_t S_tot, uint32_t K, const uint32_t* d_btab,
                 const LongestPart* d_part, uint64_t n_part, const LongestPlanes& pl, const double* d_piseg,
                 const LongestRings& rings, const LongestCarry* d_cin, const LongestRingIn& rin,
                 LongestCarry* d_cout, LongestRec* d_rec, int* d_overflow);

// Whether the thresholds get lanes of their own.  The walks are serial over a segment's sites and
// bound by latency, not by bytes: measured at 1000 x 1 M with five thresholds, lanes of their own
// take 215 ms against 333 ms on 20 chromosomes (1600 waves against 320) and 2.09 s against 4.39 s
// on one (80 against 16), although they read the planes K times.  So they are used as long as all
// their waves are resident at once -- 256 compute units x 4 SIMDs x 2 waves at k_longest_fwd's
// registers; beyond that nothing is measured and the loop, which reads the planes once, stays
// (DESIGN.md section 4).
constexpr uint64_t kLongestSplitWaves = 2048;
bool longest_split_lanes(uint64_t n_seg, uint64_t I, uint32_t K);

}  // namespace nghmm
