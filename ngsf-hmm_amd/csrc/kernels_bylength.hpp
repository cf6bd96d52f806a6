// kernels_bylength.hpp -- expected IBD above a minimum tract length (kernels_bylength.hip): host
// interface.  include/nghmm.h (nghmm_ibd_by_length) has the definition of every term.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_expect.hpp"
#include "kernels_fast.hpp"

namespace nghmm {

// laid out as nghmm_bylength_stat
struct ByLenRec {
  double tracts, length;
};
static_assert(sizeof(ByLenRec) == 16, "nghmm_bylength_stat is 16 bytes");

constexpr uint32_t kByLenMaxK = 8;             // thresholds per call
constexpr uint32_t kByLenNone = 0xffffffffu;   // b_k(a): no site of a's chromosome reaches L_k

// Per-cell scratch of one handle, 36 bytes per cell.  Fast mode: five planes tile-major
// [c T + t][i][64] (site (c 64 + lane) T + t), padding included; exact mode [S][I].
//   sigma  start_s
//   q      ln rho_s, a blocked step as the flag 1.0 (k_bylength_walk); then the prefix Q_s
//          (k_bylength_fill)
//   m      rho_s (walk); then M_s (fill)
//   d      D_s (fill, Mb only)
//   n      the blocked steps at or in front of s (fill)
struct ByLenCells {
  double *sigma, *q, *m, *d;
  uint32_t* n;
};
uint64_t bylength_cell_count(const FastState* fs, uint64_t S, uint64_t I);
inline uint64_t bylength_cell_bytes(uint64_t cells) { return cells * 36; }
inline ByLenCells bylength_carve(uint8_t* p, uint64_t cells) {
  double* x = reinterpret_cast<double*>(p);
  return ByLenCells{x, x + cells, x + 2 * cells, x + 3 * cells, reinterpret_cast<uint32_t*>(x + 4 * cells)};
}

// Per lane-chunk scratch of one handle in fast mode, [I][J] each (J = 64 C): 64 bytes
struct ByLenChunks {
  double* map;    // [3]: A, B_M, B_D of x -> A x + B, from M (D) at the chunk's last site to M (D) at
                  // the site in front of its first
  double* qtail;  // sum of ln rho behind the chunk's last blocked step (of all of it if none)
  double *endM, *endD;   // M, D at the chunk's last site (k_bylength_scan)
  double* q0;            // Q at the site in front of the chunk's first
  uint32_t *nblk, *n0;   // blocked steps in the chunk; n at the site in front of its first
};
inline uint64_t bylength_chunk_bytes(uint64_t I, uint64_t J) { return I * J * 64; }
inline ByLenChunks bylength_carve_chunks(uint8_t* p, uint64_t I, uint64_t J) {
  double* x = reinterpret_cast<double*>(p);
  const uint64_t n = I * J;
  return ByLenChunks{x, x + 3 * n, x + 4 * n, x + 5 * n, x + 6 * n, reinterpret_cast<uint32_t*>(x + 7 * n),
                     reinterpret_cast<uint32_t*>(x + 7 * n) + n};
}

// What a site shard takes from its right neighbour: Q, n and rem (M or D) of the neighbour's first
// H sites, [I][H] each
struct ByLenHalo {
  uint64_t H = 0;
  const double *q = nullptr, *rem = nullptr;
  const uint32_t* n = nullptr;
};

// fast mode, behind sample_fast_forward and support_fast_bounds: walk, scan, fill.
//   has_vin    the handle continues a site shard: its first site is an ordinary site
//   carry_in   [I][2]: M, D at the handle's last site (null: 0, nothing follows)
//   carry_out  [I][2]: M, D at the site in front of the handle's first (null: not wanted)
//   qmax       [I C]: the largest |Q| of every wave
//   pi         a plane like sigma for the posterior of the IBD state (null: not wanted; it may be
//              cells.d when mb is false, which then stays untouched)
bool bylength_fast_cells(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                         bool has_vin, bool mb, const ByLenCells& cells, const ByLenChunks& ch,
                         const double* carry_in, double* carry_out, double* qmax, double* pi = nullptr);
// Q, n, rem of the handle's first H sites, [I][H] each
void bylength_fast_halo(FastState& fs, hipStream_t st, bool mb, const ByLenCells& cells, uint64_t H,
                        double* q, uint32_t* n, double* rem);
// the terms of every start site and threshold, added per region piece and then per region.
//   btab [K][C T][64]  b_k(a) as a handle-local site, S + h for the neighbour's site h, or kByLenNone
//   cum  [C T][64] and cum_halo [H]  (Mb only) cum_s, running on across the cut
//   d_reg [n_reg], d_piece [I][n_pieces][K], d_out [I][n_reg][K]
bool bylength_fast_terms(FastState& fs, hipStream_t st, bool mb, uint32_t K, const ByLenCells& cells,
                         const uint32_t* btab, const double* cum, const double* cum_halo,
                         const ByLenHalo& halo, const ExpectRegion* d_reg, uint64_t n_reg,
                         uint64_t n_pieces, ByLenRec* d_piece, ByLenRec* d_out);

// exact mode: one lane per individual in log space, serial over the sites.  btab [K][S] and cum [S]
// site-major; cells [S][I]; fw [S + 1][I][2] as launch_expect_exact; qmax [I]; pi [S][I] the
// posterior of the IBD state (null: not wanted).  n_reg = 0 fills the cells alone.
void launch_bylength_exact(hipStream_t st, const double* eprob, const double* pos, double* fw, uint64_t S,
                           uint64_t I, const double* d_indF, const double* d_alpha, bool mb, uint32_t K,
                           const ByLenCells& cells, const uint32_t* btab, const double* cum,
                           const ExpectRegion* d_reg, uint64_t n_reg, ByLenRec* d_out, double* qmax,
                           int* d_flags, double* pi = nullptr);

}  // namespace nghmm
