// kernels_expect.hpp -- exact expectations over IBD paths (kernels_expect.hip): host interface.
// include/nghmm.h (nghmm_ibd_expect) has the definition of every term.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "expect_region.hpp"   // ExpectRegion, expect_pieces
#include "kernels_fast.hpp"

namespace nghmm {

// What a piece of a region contributes, and what a region ends up with: laid out as
// nghmm_expect_region (include/nghmm.h)
struct ExpectRec {
  double ibd, starts, switches, ibd_mb, entropy, log_p_path;
};
static_assert(sizeof(ExpectRec) == 48, "nghmm_expect_region is 48 bytes");

// laid out as nghmm_expect_site
struct ExpectSite {
  double on, off, ibd, entropy;
};
static_assert(sizeof(ExpectSite) == 32, "nghmm_expect_site is 32 bytes");

// doubles of per-cell scratch that the site records need (fast mode: [C T][I][4][64]; exact mode:
// [S][I][4]): on, off, ibd, h of every cell
uint64_t expect_cell_doubles(const FastState* fs, uint64_t S, uint64_t I);

// fast mode, behind sample_fast_forward and support_fast_bounds (fs.bound holds both boundary
// vectors of every lane-chunk): the walk over every cell, then every region's pieces added in site
// order, then (d_cell != null) the site records.
//   has_vin      the handle continues a site shard: its first site is an ordinary site
//   path16       the decoded path (null: no log_p_path), prev_state [I] the decoded state at the
//                site before the handle's first (null: there is none)
//   d_reg [n_reg], d_piece [I][n_pieces], d_out [I][n_reg], d_cell (see above), d_sites [S]
bool expect_fast_walk(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                      bool has_vin, const uint8_t* path16, const uint8_t* prev_state,
                      const ExpectRegion* d_reg, uint64_t n_reg, uint64_t n_pieces,
                      ExpectRec* d_piece, ExpectRec* d_out, double* d_cell, ExpectSite* d_sites);

// exact mode: one lane per individual over the log emissions eprob [S][I][2], with the forward
// array fw [S + 1][I][2] filled and normalised as launch_support_exact does it.  A NaN in the
// forward values raises d_flags[FLAG_INVALID_LKL].
void launch_expect_exact(hipStream_t st, const double* eprob, const double* pos, double* fw,
                         uint64_t S, uint64_t I, const double* d_indF, const double* d_alpha,
                         const uint8_t* path16, const ExpectRegion* d_reg, uint64_t n_reg,
                         ExpectRec* d_out, double* d_cell, ExpectSite* d_sites, int* d_flags);

}  // namespace nghmm
