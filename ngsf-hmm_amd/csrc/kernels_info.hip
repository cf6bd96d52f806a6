// kernels_info.hip -- log-likelihood, gradient and Hessian in (F, alpha) of every individual at one
// point, from exact derivatives carried through one forward pass (include/nghmm.h: nghmm_obs_info
// has the definition; kernels_info.hpp the jet algebra).
//
// A site is M_s = (c I + a 1 q^T) diag(1, rho), a = 1 - c, c = exp(-alpha d), q = (1 - F, F).  With
// c' = dc/dalpha = -d c and c'' = d^2 c (both 0 at a chromosome start, where c = 0) its derivatives
// all have the shape (gamma I + 1 beta^T) diag(1, rho):
//   M     gamma = c     beta = a q           M_F   gamma = 0   beta = a (-1, +1)      M_FF = 0
//   M_A   gamma = c'    beta = -c' q         M_FA  gamma = 0   beta = c' (+1, -1)
//   M_AA  gamma = c''   beta = -c'' q
// (x (I - 1 q^T) is formed as (x_1 q_0 - x_0 q_1) (-1, +1): jet_site)
// so a row x of every jet component advances by the product rule in op_step's algebra (the
// general c form: no kappa form, no small-alpha tricks -- one point needs none):
//   k_info_walk    a wave per (individual, chunk): every lane walks its T sites of e_il / pos_il
//                  once -- the one read of 8 B per cell -- carrying the jet of its lane-chunk,
//                  rescaled every RENORM sites by the exponent of the value component; then the
//                  ordered shuffle tree of the 64 lanes' jets; lane 0 stores the wave's jet;
//   k_info_finish  a wave per individual: lane l multiplies the jets of chunks l K .. l K + K - 1,
//                  the shuffle tree the lanes' (the order of lkl_point_product), and lane 0 closes
//                  with q on the left and 1 on the right -- or, for a site shard, stores the jet
//                  of the whole range and its sum of log e0 for the chain's host to multiply.
// No atomics: one order of operations, the same bits on every call.
// Exact mode: k_info_exact, one lane per individual over the materialised log emissions, the
// same jet arithmetic (ratios and c through detmath.h's exp).
#include "fast_dev.hpp"
#include "kernels_info.hpp"

namespace nghmm {

namespace {

// one site applied to both rows of every component
// a = 1 - c: for x = alpha d <= 2^-6 as expm1(x) c, since 1 - c carries the rounding of c to the 2^-53
// grid below 1 -- a relative error 1e-16 / x of the switching probability, and of every derivative
// that is proportional to it; above, 1 - c is good to 64 ulp
__device__ __forceinline__ void jet_site(Jet& J, double x, double c, double c1, double c2, double q0,
                                         double q1, double rho) {
  const double a = x <= 0.015625 ? expm1_over_x_tiny(x) * x * c : 1 - c;
  const double ce0 = c, ce1 = c * rho;
  const double g0 = a * q0, g1 = a * q1 * rho;
  const double f0 = -a, f1 = a * rho;
  // x (I - 1 q^T) = w(x) (-1, +1), w(x) = x_1 q_0 - x_0 q_1 (q_0 + q_1 = 1): formed from the
  // small terms themselves -- x_0 - (x_0 + x_1) q_0 would cancel to nothing at F = 1e-15
  const double wa0 = -c1, wa1 = c1 * rho;
  const double waa0 = -c2, waa1 = c2 * rho;
  const double h0 = c1, h1 = -c1 * rho;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i0 = 2 * r, i1 = 2 * r + 1;
    const double v0 = J.m[JET_V][i0], v1 = J.m[JET_V][i1], sv = v0 + v1;
    const double F0 = J.m[JET_F][i0], F1 = J.m[JET_F][i1], sF = F0 + F1;
    const double A0 = J.m[JET_A][i0], A1 = J.m[JET_A][i1], sA = A0 + A1;
    const double FF0 = J.m[JET_FF][i0], FF1 = J.m[JET_FF][i1], sFF = FF0 + FF1;
    const double FA0 = J.m[JET_FA][i0], FA1 = J.m[JET_FA][i1], sFA = FA0 + FA1;
    const double AA0 = J.m[JET_AA][i0], AA1 = J.m[JET_AA][i1], sAA = AA0 + AA1;
    const double wv = fma(v1, q0, -(v0 * q1));
    const double wF = fma(F1, q0, -(F0 * q1));
    const double wA = fma(A1, q0, -(A0 * q1));
    // x M
    J.m[JET_V][i0] = fma(g0, sv, ce0 * v0);
    J.m[JET_V][i1] = fma(g1, sv, ce1 * v1);
    // x_F M + x M_F
    J.m[JET_F][i0] = fma(f0, sv, fma(g0, sF, ce0 * F0));
    J.m[JET_F][i1] = fma(f1, sv, fma(g1, sF, ce1 * F1));
    // x_A M + x M_A
    J.m[JET_A][i0] = fma(wa0, wv, fma(g0, sA, ce0 * A0));
    J.m[JET_A][i1] = fma(wa1, wv, fma(g1, sA, ce1 * A1));
    // x_FF M + 2 x_F M_F
    J.m[JET_FF][i0] = fma(2 * f0, sF, fma(g0, sFF, ce0 * FF0));
    J.m[JET_FF][i1] = fma(2 * f1, sF, fma(g1, sFF, ce1 * FF1));
    // x_FA M + x_F M_A + x_A M_F + x M_FA
    J.m[JET_FA][i0] = fma(h0, sv, fma(f0, sA, fma(wa0, wF, fma(g0, sFA, ce0 * FA0))));
    J.m[JET_FA][i1] = fma(h1, sv, fma(f1, sA, fma(wa1, wF, fma(g1, sFA, ce1 * FA1))));
    // x_AA M + 2 x_A M_A + x M_AA
    J.m[JET_AA][i0] = fma(waa0, wv, fma(2 * wa0, wA, fma(g0, sAA, ce0 * AA0)));
    J.m[JET_AA][i1] = fma(waa1, wv, fma(2 * wa1, wA, fma(g1, sAA, ce1 * AA1)));
  }
}

__device__ __forceinline__ Jet jet_shfl_down(const Jet& j, int off) {
  Jet o;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) o.m[k][q] = __shfl_down(j.m[k][q], off);
  o.ex = __shfl_down(j.ex, off);
  return o;
}

// ordered product of the 64 lanes' jets; lane 0 holds it
__device__ __forceinline__ Jet jet_wave_product(Jet m, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const Jet o = jet_shfl_down(m, off);
    if ((lane & (2 * off - 1)) == 0) m = jet_mul(m, o);
  }
  return m;
}

__global__ void __launch_bounds__(64)
k_info_walk(const double* __restrict__ e_il, const double* __restrict__ pos_il, uint64_t T, uint32_t C,
            const double* __restrict__ F, const double* __restrict__ A, double* __restrict__ part) {
  // chunk-major, as the objective kernels: the resident waves share slices of the distance table
  const uint32_t n_i = gridDim.x / C;
  const uint64_t i = blockIdx.x % n_i;
  const uint32_t c = blockIdx.x / n_i;
  const int lane = threadIdx.x;
  const double f = F[i], al = A[i];
  const double q0 = 1 - f, q1 = f;
  const double* ep = e_il + ((i * C + c) * T) * 64 + lane;
  const double* dp = pos_il + ((uint64_t)c * T) * 64 + lane;
  Jet J = jet_identity();
  double rc[RENORM], dc[RENORM], rn[RENORM], dn[RENORM];
#pragma unroll
  for (int u = 0; u < RENORM; ++u) {
    rc[u] = ep[(uint64_t)u * 64];
    dc[u] = dp[(uint64_t)u * 64];
  }
  for (uint64_t t0 = 0; t0 < T; t0 += RENORM) {   // T is a multiple of RENORM
    const bool more = t0 + RENORM < T;
#pragma unroll
    for (int u = 0; u < RENORM; ++u) {
      rn[u] = more ? ep[(t0 + RENORM + u) * 64] : 1.0;
      dn[u] = more ? dp[(t0 + RENORM + u) * 64] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < RENORM; ++u) {
      const double d = dc[u];
      const bool start = !(d < kDStart);
      const double cc = coanc(al, d);
      const double c1 = start ? 0.0 : -d * cc;
      const double c2 = start ? 0.0 : -d * c1;
      jet_site(J, al * d, cc, c1, c2, q0, q1, rc[u]);
    }
    jet_renorm(J);
#pragma unroll
    for (int u = 0; u < RENORM; ++u) {
      rc[u] = rn[u];
      dc[u] = dn[u];
    }
  }
  J = jet_wave_product(J, lane);
  if (lane == 0) jet_store(part + (i * C + c) * kJetDoubles, J);
}

template <bool SHARD>
__global__ void __launch_bounds__(64)
k_info_finish(const double* __restrict__ part, uint32_t C, const double* __restrict__ base_c,
              const double* __restrict__ F, double* __restrict__ out) {
  const uint64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t K = (C + 63) / 64;
  const double base = base_sum(base_c + i * C, C, lane);
  const double* pj = part + i * C * kJetDoubles;
  Jet m = jet_identity();
  if ((uint32_t)lane * K < C) m = jet_load(pj + ((uint64_t)(uint32_t)lane * K) * kJetDoubles);
  for (uint32_t u = 1; u < K; ++u) {
    const uint32_t k = (uint32_t)lane * K + u;
    if (k < C) m = jet_mul(m, jet_load(pj + (uint64_t)k * kJetDoubles));
  }
  m = jet_wave_product(m, lane);
  if (lane == 0) {
    if constexpr (SHARD) {
      jet_store(out + i * kJetShardDoubles, m);
      out[i * kJetShardDoubles + 25] = base;
    } else {
      const InfoRec r = jet_close(m, F[i], base);
      double* o = out + i * 6;
      o[0] = r.lkl;
      o[1] = r.g_F;
      o[2] = r.g_A;
      o[3] = r.h_FF;
      o[4] = r.h_FA;
      o[5] = r.h_AA;
    }
  }
}

// exact mode: eprob [S][I][2] log emissions, pos [S] (+inf at a chromosome start)
__global__ void __launch_bounds__(64)
k_info_exact(const double* __restrict__ eprob, const double* __restrict__ pos, uint64_t S, uint64_t I,
             const double* __restrict__ F, const double* __restrict__ A, double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const double f = F[i], al = A[i];
  const double q0 = 1 - f, q1 = f;
  const double2* e2 = reinterpret_cast<const double2*>(eprob);
  Jet J = jet_identity();
  double base = 0.0;
  for (uint64_t s = 0; s < S; ++s) {
    const double2 le = e2[s * I + i];
    const double d = pos[s];
    const bool start = !(d < kDStart);
    const double cc = start ? 0.0 : det_exp(-al * d);
    const double c1 = start ? 0.0 : -d * cc;
    const double c2 = start ? 0.0 : -d * c1;
    base += le.x;
    jet_site(J, start ? 1.0 : al * d, cc, c1, c2, q0, q1, det_exp(le.y - le.x));
    if ((s & (RENORM - 1)) == RENORM - 1) jet_renorm(J);
  }
  jet_renorm(J);
  const InfoRec r = jet_close(J, f, base);
  double* o = out + i * 6;
  o[0] = r.lkl;
  o[1] = r.g_F;
  o[2] = r.g_A;
  o[3] = r.h_FF;
  o[4] = r.h_FA;
  o[5] = r.h_AA;
}

}  // namespace

bool info_fast(const FastState& fs, hipStream_t st, const double* d_F, const double* d_A,
               double* d_part, double* d_out, bool as_shard) {
  if (fs.T % RENORM != 0 || fs.C == 0) return false;
  hipLaunchKernelGGL(k_info_walk, dim3((unsigned)(fs.I * fs.C)), dim3(64), 0, st, fs.e_il, fs.pos_il,
                     fs.T, fs.C, d_F, d_A, d_part);
  if (as_shard)
    hipLaunchKernelGGL(k_info_finish<true>, dim3((unsigned)fs.I), dim3(64), 0, st, d_part, fs.C,
                       fs.base_c, d_F, d_out);
  else
    hipLaunchKernelGGL(k_info_finish<false>, dim3((unsigned)fs.I), dim3(64), 0, st, d_part, fs.C,
                       fs.base_c, d_F, d_out);
  return hipGetLastError() == hipSuccess;
}

void launch_info_exact(hipStream_t st, const double* eprob, const double* pos, uint64_t S, uint64_t I,
                       const double* d_F, const double* d_A, double* d_out) {
  hipLaunchKernelGGL(k_info_exact, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, eprob, pos, S, I,
                     d_F, d_A, d_out);
}

}  // namespace nghmm
