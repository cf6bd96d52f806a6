// kernels_info.hpp -- log-likelihood, gradient and Hessian in (F, alpha) per individual
// (kernels_info.hip): the second-order jet of 2x2 operators and the host interface.
// include/nghmm.h (nghmm_obs_info) has the definition.
//
// A run of sites is the product of its operators M_s(F, alpha) (fast_dev.hpp: Op); the product rule
// carries the derivatives along: a JET (M, M_F, M_A, M_FF, M_FA, M_AA) of six 2x2 matrices with
// ONE binary exponent, that of the value component -- the derivative components are signed and
// share it.  Jets compose associatively (jet_mul: 15 2x2 products), so lane-chunks, waves and site
// shards multiply theirs exactly as they multiply operators.  Everything that forms a product or
// closes it is __host__ __device__: a chain's host multiplies its shards' jets with the routine
// the device uses.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels_fast.hpp"

namespace nghmm {

enum { JET_V = 0, JET_F = 1, JET_A = 2, JET_FF = 3, JET_FA = 4, JET_AA = 5 };

struct Jet {
  double m[6][4];   // [component][a00, a01, a10, a11], row-vector convention v' = v M
  int ex;
};
// a jet in memory: the 24 entries, the exponent; site shards add their sum of log e0
constexpr int kJetDoubles = 25;
constexpr int kJetShardDoubles = 26;

// the six doubles of nghmm_info
struct InfoRec {
  double lkl, g_F, g_A, h_FF, h_FA, h_AA;
};

__host__ __device__ inline Jet jet_identity() {
  Jet j;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) j.m[k][e] = 0.0;
  j.m[0][0] = j.m[0][3] = 1.0;
  j.ex = 0;
  return j;
}

// exponent e with mx = m * 2^e, m in [0.5, 1); 0 for mx == 0 or non-finite (fast_dev.hpp: exp_of)
__host__ __device__ inline int jet_exp_of(double mx) {
  if (!(mx > 0.0 && mx < __builtin_huge_val())) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_frexp_exp(mx);
#else
  int e;
  (void)std::frexp(mx, &e);
  return e;
#endif
}

// by the exponent of the VALUE component (non-negative entries)
__host__ __device__ inline void jet_renorm(Jet& j) {
  const double mx = fmax(fmax(j.m[0][0], j.m[0][1]), fmax(j.m[0][2], j.m[0][3]));
  const int e = jet_exp_of(mx);
  const double sc = __builtin_ldexp(1.0, -e);
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) j.m[k][q] *= sc;
  j.ex += e;
}

// o = L R
__host__ __device__ inline void jet_mm(double* o, const double* L, const double* R) {
  o[0] = fma(L[0], R[0], L[1] * R[2]);
  o[1] = fma(L[0], R[1], L[1] * R[3]);
  o[2] = fma(L[2], R[0], L[3] * R[2]);
  o[3] = fma(L[2], R[1], L[3] * R[3]);
}
// o += w L R
__host__ __device__ inline void jet_mma(double* o, const double* L, const double* R, double w) {
  o[0] = fma(w, fma(L[0], R[0], L[1] * R[2]), o[0]);
  o[1] = fma(w, fma(L[0], R[1], L[1] * R[3]), o[1]);
  o[2] = fma(w, fma(L[2], R[0], L[3] * R[2]), o[2]);
  o[3] = fma(w, fma(L[2], R[1], L[3] * R[3]), o[3]);
}

// L applied first, then R: the product rule to second order, 15 2x2 products
__host__ __device__ inline Jet jet_mul(const Jet& L, const Jet& R) {
  Jet o;
  jet_mm(o.m[JET_V], L.m[JET_V], R.m[JET_V]);
  jet_mm(o.m[JET_F], L.m[JET_F], R.m[JET_V]);
  jet_mma(o.m[JET_F], L.m[JET_V], R.m[JET_F], 1.0);
  jet_mm(o.m[JET_A], L.m[JET_A], R.m[JET_V]);
  jet_mma(o.m[JET_A], L.m[JET_V], R.m[JET_A], 1.0);
  jet_mm(o.m[JET_FF], L.m[JET_FF], R.m[JET_V]);
  jet_mma(o.m[JET_FF], L.m[JET_F], R.m[JET_F], 2.0);
  jet_mma(o.m[JET_FF], L.m[JET_V], R.m[JET_FF], 1.0);
  jet_mm(o.m[JET_FA], L.m[JET_FA], R.m[JET_V]);
  jet_mma(o.m[JET_FA], L.m[JET_F], R.m[JET_A], 1.0);
  jet_mma(o.m[JET_FA], L.m[JET_A], R.m[JET_F], 1.0);
  jet_mma(o.m[JET_FA], L.m[JET_V], R.m[JET_FA], 1.0);
  jet_mm(o.m[JET_AA], L.m[JET_AA], R.m[JET_V]);
  jet_mma(o.m[JET_AA], L.m[JET_A], R.m[JET_A], 2.0);
  jet_mma(o.m[JET_AA], L.m[JET_V], R.m[JET_AA], 1.0);
  o.ex = L.ex + R.ex;
  jet_renorm(o);
  return o;
}

__host__ __device__ inline Jet jet_load(const double* p) {
  Jet j;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) j.m[k][q] = p[k * 4 + q];
  j.ex = (int)p[24];
  return j;
}
__host__ __device__ inline void jet_store(double* p, const Jet& j) {
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) p[k * 4 + q] = j.m[k][q];
  p[24] = (double)j.ex;
}

// The record of the whole product P: Z = q P 1 with q = (1 - F, F), dq/dF = (-1, +1) -- three
// more terms --, lkl = base + log Z + ex ln 2, g = Z_x / Z, h_xy = Z_xy / Z - g_x g_y.
__host__ __device__ inline InfoRec jet_close(const Jet& P, double F, double base) {
  const double q0 = 1 - F, q1 = F;
  double rs[6][2];   // row sums P_k 1
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    rs[k][0] = P.m[k][0] + P.m[k][1];
    rs[k][1] = P.m[k][2] + P.m[k][3];
  }
  const double Z = fma(q0, rs[JET_V][0], q1 * rs[JET_V][1]);
  const double dV = rs[JET_V][1] - rs[JET_V][0];   // (dq/dF) P 1
  const double dF = rs[JET_F][1] - rs[JET_F][0];
  const double dA = rs[JET_A][1] - rs[JET_A][0];
  const double ZF = fma(q0, rs[JET_F][0], q1 * rs[JET_F][1]) + dV;
  const double ZA = fma(q0, rs[JET_A][0], q1 * rs[JET_A][1]);
  const double ZFF = fma(2.0, dF, fma(q0, rs[JET_FF][0], q1 * rs[JET_FF][1]));
  const double ZFA = fma(q0, rs[JET_FA][0], q1 * rs[JET_FA][1]) + dA;
  const double ZAA = fma(q0, rs[JET_AA][0], q1 * rs[JET_AA][1]);
  const double iz = 1.0 / Z;
  InfoRec r;
  r.lkl = base + (log(Z) + (double)P.ex * 0.6931471805599453094);
  r.g_F = ZF * iz;
  r.g_A = ZA * iz;
  r.h_FF = fma(-r.g_F, r.g_F, ZFF * iz);
  r.h_FA = fma(-r.g_F, r.g_A, ZFA * iz);
  r.h_AA = fma(-r.g_A, r.g_A, ZAA * iz);
  return r;
}

// ---- host interface ----
// doubles of scratch behind the points: the waves' jets [I][C][25] (fast mode), then the result
// [I][26] (a record, or a shard's jet and its sum of log e0)
inline uint64_t info_scratch_doubles(uint64_t I, uint32_t C) {
  return I * (uint64_t)(C ? C : 1) * kJetDoubles + I * kJetShardDoubles;
}
// fast mode: one walk over e_il / pos_il at the points (d_F, d_A) [I]; d_part = the waves' jets.
// as_shard: d_out [I][26] = the jet of the handle's site range and its sum of log e0, without
// the closing q; else d_out [I][6] = the records
bool info_fast(const FastState& fs, hipStream_t st, const double* d_F, const double* d_A,
               double* d_part, double* d_out, bool as_shard);
// exact mode: one lane per individual over the materialised log emissions eprob [S][I][2];
// d_out [I][6]
void launch_info_exact(hipStream_t st, const double* eprob, const double* pos, uint64_t S, uint64_t I,
                       const double* d_F, const double* d_A, double* d_out);

}  // namespace nghmm
