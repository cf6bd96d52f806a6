// capi_chain.hpp -- what the IBD entry points that walk a chain of site shards themselves share
// (capi_chain.hip): the checks every one of them opens with, and the relay of the boundary vectors
// from shard to shard.  capi_chain_host.hpp has the part that needs no device.
#pragma once

#include "capi_chain_host.hpp"
#include "capi_internal.hpp"

namespace capi {

// hs[0 .. n) is what nghmm_chain_setup made a chain of, in rank order; one handle needs no chain
// (and may be NULL: chain_check_loaded answers that).  (capi_multi.hip: is_chain asks the chain's
// own list instead, which a later nghmm_site_shard_setup on a member does not change.)
int chain_entry_check(nghmm_t** hs, int n, const char* who);
// every handle holds data; *S_tot (may be NULL) = the sites of all of them
int chain_check_loaded(nghmm_t** hs, int n, const char* who, uint64_t* S_tot = nullptr);
// more than one handle: fast mode
int chain_check_fast(nghmm_t** hs, int n, const char* who);
// sets "<who>: the fast layout ... is not one the walk knows, or a kernel launch failed"
int fast_layout_error(const nghmm_t* h, const char* who);

// The boundary vectors of a chain, I x 2 doubles per cut, through one host vector: the forward
// vectors from the first shard to the last (sample_fast_forward), then the backward vectors from
// the last to the first (support_fast_bounds), after which fast.bound of every shard holds both.
// The caller makes shard r's device current, registers the relay's vectors with the carver of r's
// scratch (add), and puts its own work around the steps; every step queues on hs[r]->stream.
class ChainRelay {
 public:
  // two_vectors: the backward pair lies where the forward pair lay (nghmm_tract_bounds)
  ChainRelay(nghmm_t** hs, int n, bool two_vectors = false);
  void add(Carver& cv, int r);
  // clears the flags; fast mode: the emissions, the vector of shard r - 1 in, the forward half,
  // the vector for shard r + 1 out; checks the flags, which waits for the stream
  int forward(int r);
  // the vector of shard r + 1 in; the backward half (who: the message if it fails, or NULL for none)
  int backward_upload(int r);
  int backward_bounds(int r, const char* who);
  int backward_begin(int r, const char* who) {
    const int rc = backward_upload(r);
    return rc ? rc : backward_bounds(r, who);
  }
  // the vector for shard r - 1 out: the caller waits for the stream before the next step
  int backward_end(int r);

 private:
  struct Vecs {
    double *vin = nullptr, *vout = nullptr, *win = nullptr, *wout = nullptr;
  };
  double* win(int r) const { return two_ ? v_[r].vin : v_[r].win; }
  double* wout(int r) const { return two_ ? v_[r].vout : v_[r].wout; }
  nghmm_t** hs_;
  int n_;
  bool fast_, two_;
  uint64_t I_;
  std::vector<Vecs> v_;
  std::vector<double> vec_;
};

}  // namespace capi
