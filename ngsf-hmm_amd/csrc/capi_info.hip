// capi_info.hip -- nghmm_obs_info / nghmm_chain_obs_info: per individual the log-likelihood, its
// gradient and its Hessian in (F, alpha) at one point (kernels_info.hip).  A chain's shards each
// produce the jet of their site range; the host multiplies them in rank order with the routine
// the device uses (kernels_info.hpp: jet_mul) and closes once.
// (implementation of include/nghmm.h; capi_internal.hpp has the handle and the shared helpers.)
#include "capi_chain.hpp"
#include "kernels_info.hpp"

static_assert(sizeof(nghmm_info) == 48, "nghmm_info is 48 bytes");
static_assert(sizeof(InfoRec) == sizeof(nghmm_info), "the device's record is nghmm_info");

namespace {

int info_impl(nghmm_t** hs, int n, const double* F, const double* alpha, nghmm_info* out,
              const char* who) {
  int rc;
  if ((rc = chain_check_loaded(hs, n, who))) return rc;
  if (!out || (F == nullptr) != (alpha == nullptr)) {
    set_error("%s: out %s, F %s, alpha %s: out is needed, and F and alpha both or neither", who,
              out ? "given" : "NULL", F ? "given" : "NULL", alpha ? "given" : "NULL");
    return NGHMM_ERR_ARG;
  }
  const bool fast = hs[0]->mode == NGHMM_MODE_FAST;
  if ((rc = chain_check_fast(hs, n, who))) return rc;
  const uint64_t I = hs[0]->I;
  if (F)
    for (uint64_t i = 0; i < I; ++i)   // the box of EM.cpp:424-438; NaN fails every comparison
      if (!(F[i] >= 1e-15 && F[i] <= 1 - 1e-15 && alpha[i] >= 1e-15 && alpha[i] <= 10.0)) {
        set_error("%s: point of individual %llu, (F, alpha) = (%g, %g), is outside [1e-15, 1 - 1e-15] "
                  "x [1e-15, 10]", who, (unsigned long long)i, F[i], alpha[i]);
        return NGHMM_ERR_ARG;
      }
  std::vector<double> jets(n > 1 ? (size_t)n * I * kJetShardDoubles : 0), Fh;
  for (int r = 0; r < n; ++r) {
    nghmm_t* h = hs[r];
    if ((rc = use_device(h))) return rc;
    const uint32_t C = fast ? h->fast.C : 0;
    if ((rc = h->d_info.reserve((2 * I + info_scratch_doubles(I, C)) * sizeof(double))))
      return rc;
    double* d_F = reinterpret_cast<double*>(h->d_info.p);
    double* d_A = d_F + I;
    double* d_part = d_A + I;
    double* d_out = d_part + I * (uint64_t)(C ? C : 1) * kJetDoubles;
    if (F) {
      HIP_TRY(hipMemcpyAsync(d_F, F, I * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(d_A, alpha, I * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    const double* pF = F ? d_F : h->d_indF;
    const double* pA = F ? d_A : h->d_alpha;
    if ((rc = clear_flags(h))) return rc;
    if (fast) {
      if ((rc = ensure_emissions(h))) return rc;
      if (!info_fast(h->fast, h->stream, pF, pA, d_part, d_out, n > 1)) {
        set_error("%s: the fast layout (C = %u waves, T = %u sites per lane) is not one the kernels walk, "
                  "or a kernel launch failed", who, (unsigned)h->fast.C, (unsigned)h->fast.T);
        return NGHMM_ERR_HIP;
      }
    } else {
      launch_info_exact(h->stream, h->d_eprob, h->d_pos, h->S, I, pF, pA, d_out);
    }
    HIP_TRY(hipGetLastError());
    if (n > 1) {
      HIP_TRY(hipMemcpyAsync(&jets[(size_t)r * I * kJetShardDoubles], d_out,
                             I * kJetShardDoubles * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      if (r == 0 && !F) {   // the chain's parameters are equal on every handle
        Fh.resize(I);
        HIP_TRY(hipMemcpyAsync(Fh.data(), h->d_indF, I * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      }
    } else {
      HIP_TRY(hipMemcpyAsync(out, d_out, I * sizeof(nghmm_info), hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = check_flags(h))) return rc;   // (waits for the stream)
  }
  if (n > 1)
    for (uint64_t i = 0; i < I; ++i) {
      const double* p = &jets[i * kJetShardDoubles];
      Jet m = jet_load(p);
      double base = p[25];
      for (int r = 1; r < n; ++r) {
        p = &jets[((size_t)r * I + i) * kJetShardDoubles];
        m = jet_mul(m, jet_load(p));
        base += p[25];
      }
      const InfoRec rec = jet_close(m, F ? F[i] : Fh[i], base);
      std::memcpy(&out[i], &rec, sizeof rec);
    }
  return NGHMM_OK;
}

}  // namespace

int nghmm_obs_info(nghmm_t* h, const double* F, const double* alpha, nghmm_info* out) {
  g_last_error.clear();
  return info_impl(&h, 1, F, alpha, out, "nghmm_obs_info");
}

int nghmm_chain_obs_info(nghmm_t** hs, int n, const double* F, const double* alpha, nghmm_info* out) {
  g_last_error.clear();
  const char* who = "nghmm_chain_obs_info";
  const int rc = chain_entry_check(hs, n, who);
  return rc ? rc : info_impl(hs, n, F, alpha, out, who);
}
