// kernels_freqinfo.hpp -- per-site likelihood in the allele frequency (kernels_freqinfo.hip): host
// interface.  include/nghmm.h (nghmm_freq_info) has the definition of a record.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "glview.hpp"
#include "kernels_fast.hpp"

namespace nghmm {

constexpr uint32_t FREQINFO_MAX_LEVELS = 8;

// laid out as nghmm_freq_stat (include/nghmm.h)
struct FreqStat {
  double freq, ll, score, info;
};
static_assert(sizeof(FreqStat) == 32, "nghmm_freq_stat is 32 bytes");

struct FreqLevels {
  uint32_t n;
  uint32_t pad;
  double f[FREQINFO_MAX_LEVELS];
};

// a chromosome start in the distances (+inf; as kernels_bounds.hpp)
inline bool freqinfo_chrom_start(double d) { return !(d < 1e22); }

// fast mode: the two walks of one handle, plain vector recursions over the site-major LINEAR
// likelihoods gl_lin [S][I], the frequencies d_freq [S] and the distances d_pos [S]; one lane per
// (individual, segment).  d_seg [n_seg + 1]: the first site of every segment -- site 0 and every
// chromosome start --, then S.  d_cav [S][I][2]: the forward walk leaves every site's prediction
// there, the backward walk (which follows it) the two weights (1 - c, c) in its place.
//   forward  d_vin [I][2]: the forward vector after the last site of the shard before (null: the
//            handle holds the data's first site); d_vout [I][2] (may be null): the one after this
//            handle's last site
//   backward d_win [I][2]: the backward vector at the handle's last site (null: (1, 1)); d_wout
//            [I][2] (may be null): the one at the last site of the shard before
// A weight that is NaN raises d_flags[FLAG_INVALID_LKL].
bool freqinfo_fast_walks(hipStream_t st, const GlView& gl_lin, const double* d_freq, const double* d_pos,
                         const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I,
                         const double* d_indF, const double* d_alpha, const double* d_vin,
                         double* d_vout, const double* d_win, double* d_wout, double* d_cav,
                         int* d_flags, bool backward);

// exact mode: one lane per individual in log space over the LOG likelihoods gl_log [S][I] cells and
// the frequencies (the two log emissions of a cell are formed on the way); fw [S + 1][I][2] is
// scratch for the normalised forward values, as in launch_support_exact; d_cav [S][I][2]
void launch_freqinfo_exact(hipStream_t st, const GlView& gl_log, const double* d_freq, const double* pos,
                           double* fw, uint64_t S, uint64_t I, const double* d_indF,
                           const double* d_alpha, double* d_cav, int* d_flags);

// the site pass: d_stats [S], d_curve [S][lv.n] from the weights d_cav [S][I][2] and the
// likelihoods gl, site-major [S][I] cells (log_gl: their logarithms)
bool freqinfo_sites(hipStream_t st, const double* d_cav, const GlView& gl, bool log_gl,
                    const double* d_freq, uint64_t S, uint64_t I, const FreqLevels& lv,
                    FreqStat* d_stats, double* d_curve);

// d_out [I][S] = c of every cell (the second weight)
bool freqinfo_cavity_out(hipStream_t st, const double* d_cav, uint64_t S, uint64_t I, double* d_out);

}  // namespace nghmm
