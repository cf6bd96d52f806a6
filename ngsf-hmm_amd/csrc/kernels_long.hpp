// kernels_long.hpp -- per-site posterior of lying in an IBD tract of at least L_k
// (kernels_long.hip): host interface.  include/nghmm.h (nghmm_ibd_long) has the definition of every
// term; the cells (sigma, Q, n and the posterior pi) are kernels_bylength.hip's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_bylength.hpp"

namespace nghmm {

// laid out as nghmm_long_region_stat and nghmm_long_site_stat
struct LongRec {
  double sites, mb;
};
struct LongSite {
  double sum;
  uint64_t count;
};
static_assert(sizeof(LongRec) == 16 && sizeof(LongSite) == 16, "the records are 16 bytes");

// What the gather at lo_k(s) reads, one 32-byte record per cell (a lane touches one cache line, not
// one per plane): pi, Q and n of the cell, and the current threshold's prefix U.
struct alignas(32) LongCell {
  double pi, q, u;
  uint32_t n, pad;
};
static_assert(sizeof(LongCell) == 32, "LongCell");

// Per-cell scratch of one handle besides ByLenCells (36 bytes; its d plane holds pi, its m plane the
// current threshold's T_k): the packed records and the plane P of the current threshold, 40 bytes
// per cell whatever K is.  Fast mode tile-major as ByLenCells, exact mode [S][I].
struct LongPlanes {
  LongCell* rec;
  double* p;
};
inline uint64_t long_cell_bytes(uint64_t cells) { return cells * 40; }
inline LongPlanes long_carve(uint8_t* x, uint64_t cells) {
  return LongPlanes{reinterpret_cast<LongCell*>(x), reinterpret_cast<double*>(x + cells * 32)};
}

// Per lane-chunk scratch in fast mode, [I][J] each: 20 bytes
struct LongChunks {
  double* utail;    // the sum of T_k behind the chunk's last blocked step (of all of it if none)
  double* u0;       // U at the site in front of the chunk's first
  uint32_t* ublk;   // whether the chunk holds a blocked step
};
inline uint64_t long_chunk_bytes(uint64_t I, uint64_t J) { return I * J * 20; }
inline LongChunks long_carve_chunks(uint8_t* p, uint64_t I, uint64_t J) {
  double* x = reinterpret_cast<double*>(p);
  return LongChunks{x, x + I * J, reinterpret_cast<uint32_t*>(x + 2 * I * J)};
}

// What a site shard takes from its left neighbour, h = 0 at the neighbour's last site and counting
// back from there, [I][H] each: pi, the sum of ln rho and the blocked steps from the site to the
// cut, and suf, the current threshold's sum of T_k over the sites behind it; all [I]: the
// neighbour's U at its last site.
struct LongLeft {
  bool has_left = false;
  uint64_t H = 0;
  const double *pi = nullptr, *qc = nullptr, *suf = nullptr, *all = nullptr;
  const uint32_t* nc = nullptr;
};

// (pi, Q, n) of every cell into the packed records; either layout
void long_pack(hipStream_t st, uint64_t cells, const ByLenCells& cl, LongCell* rec);

// fast mode, behind bylength_fast_cells (with pi in cl.d): one threshold.  btab, lotab [C T][64]:
// b_k(a) as a handle-local site, S + h for the right neighbour's site h, or kByLenNone; lo_k(s) as a
// handle-local site, S + h for the left neighbour's site h from its end, or kByLenNone.  Leaves
// T_k in cl.m, U in the records and P_k in pl.p.
bool long_fast_threshold(FastState& fs, hipStream_t st, const ByLenCells& cl, const ByLenChunks& ch,
                         const LongPlanes& pl, const LongChunks& lc, const uint32_t* btab,
                         const uint32_t* lotab, const ByLenHalo& right, const LongLeft& left);
// ... what the shard behind takes from it: pi, qc, nc and T_k of its last H sites [I][H], U at its
// last site [I]
void long_fast_halo_left(FastState& fs, hipStream_t st, const ByLenCells& cl, const LongPlanes& pl, uint64_t H,
                         double* hpi, double* hqc, uint32_t* hnc, double* ht, double* hall);
// ... its region records: d_piece [I][n_pieces], d_out [I][n_reg][K] at threshold k
bool long_fast_regions(FastState& fs, hipStream_t st, const ByLenCells& cl, const LongPlanes& pl,
                       bool has_vin, const ExpectRegion* d_reg, uint64_t n_reg, uint64_t n_pieces,
                       LongRec* d_piece, uint32_t K, uint32_t k, LongRec* d_out);
// ... its site records, d_site [S][K] at threshold k
void long_fast_sites(FastState& fs, hipStream_t st, const LongPlanes& pl, double thr, uint32_t K, uint32_t k,
                     LongSite* d_site);
// ... P_k as d_post [I][S]
void long_fast_post(FastState& fs, hipStream_t st, const LongPlanes& pl, double* d_post);

// exact mode, behind launch_bylength_exact (n_reg = 0, pi in cl.d): the same, planes [S][I], btab
// and lotab [S], pos [S] the site distances
void long_exact_threshold(hipStream_t st, uint64_t S, uint64_t I, const ByLenCells& cl, const LongPlanes& pl,
                          const uint32_t* btab, const uint32_t* lotab);
void long_exact_regions(hipStream_t st, uint64_t S, uint64_t I, const double* pos, const ByLenCells& cl,
                        const LongPlanes& pl, const ExpectRegion* d_reg, uint64_t n_reg, uint32_t K, uint32_t k,
                        LongRec* d_out);
void long_exact_sites(hipStream_t st, uint64_t S, uint64_t I, const LongPlanes& pl, double thr, uint32_t K,
                      uint32_t k, LongSite* d_site);
void long_exact_post(hipStream_t st, uint64_t S, uint64_t I, const LongPlanes& pl, double* d_post);

}  // namespace nghmm
