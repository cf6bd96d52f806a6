// capi_internal.hpp -- what the translation units of the C ABI share: the handle, error plumbing,
// and the helpers every entry point uses.  nghmm_capi.hip and the capi_*.hip files, each of which
// says in its first lines which calls it holds, implement include/nghmm.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <functional>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nghmm.h"
#include "../../include/nghmm_debug.h"
#include "bfgs_batch.hpp"
#include "capi_chain_host.hpp"   // align256
#include "capi_owners.hpp"
#include "kernels.hpp"
#include "kernels_fast.hpp"
#include "kernels_sharing.hpp"
#include "kernels_summary.hpp"

using namespace nghmm;

namespace capi {

// the message of the last failing call on this thread (include/nghmm.h, nghmm_last_error)
extern thread_local std::string g_last_error;

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess) {                                                       \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__,  \
                __LINE__);                                                         \
      return NGHMM_ERR_HIP;                                                        \
    }                                                                              \
  } while (0)

enum Slot { SLOT_EMISSION = 0, SLOT_FORWARD = 1, SLOT_BACKWARD = 2, SLOT_LKL = 3, SLOT_ESTMAF = 4,
            SLOT_VITERBI = 5, SLOT_LKL_FIRST = 6, SLOT_BFGS = 7, NSLOTS = 8 };

}  // namespace capi

using namespace capi;

struct ChainCtx;   // nghmm_chain_setup
// Everything the handle takes from the runtime is a member that releases itself
// (capi_owners.hpp).  Members go in reverse order of declaration, after the destructor has
// drained the streams: so the streams and the handle's events come first here -- they go last,
// after every buffer -- and the lanes hold their events before their buffers.
struct nghmm_handle {
  ~nghmm_handle();   // nghmm_capi.hip
  uint64_t I = 0, S = 0;
  int device = 0, mode = NGHMM_MODE_EXACT;
  Stream stream;
  Event ev0, ev1, ev_sync;
  // exact mode, fused iteration: est_maf on a second stream underneath the objective rounds
  Stream aux_stream;
  Stream g_xstream;   // member of a group (below): the peer copies' stream
  Event aux_ev0, aux_ev1, aux_go, aux_done;
  static constexpr uint32_t kAuxPieces = 16;   // exact mode: est_maf underneath the rounds, in pieces
  Event aux_piece_ev[kAuxPieces];
  Event aux_estep_ev[3];                       // ... the E-step next to the first rounds: its timing
  DevBuf<double> d_aux_params;                 // ... and its own copies of indF / alpha [2][I]
  // pinned landing places of what every call reads back -- the error flags, and a fused iteration's
  // log-likelihoods: a copy to pageable memory is staged and waited for by the runtime, one each
  PinBuf<int> h_flags_pin;         // [NFLAGS]
  PinBuf<double> h_lkl_pin;        // [I]
  hipEvent_t param_snapshot_ev = nullptr;      // (borrowed) those copies are made: an M-step's new parameters wait for it
  bool blocking_sync = false;
  bool loaded = false;
  bool warmed = false;   // nghmm_emission has set up what the first EM iteration needs

  DevBuf<double> d_gl, d_pos;   // (a replica borrows its parent's: nghmm_create_replica)
  DevBuf<double> d_freq, d_eprob, d_fw, d_marg, d_indF, d_alpha, d_ind_lkl;
  DevBuf<int> d_flags;

  // the objective points of one round: the four grow together (ensure_points)
  DevScratch<uint32_t> d_pt_ind;
  DevScratch<double> d_pt_F, d_pt_A, d_pt_lkl;

  DevBuf<uint8_t> d_bp, d_path_sites, d_path;
  DevBuf<double> d_vit;  // Viterbi scratch: transition logs of one site chunk + carry state
  DevBuf<double> d_tmp;  // S*I*2 doubles, transposes for host read-back
  DevScratch<double> d_geno;  // .geno posteriors of one site chunk
  DevScratch<char> d_text;    // formatted posterior lines of one batch of individuals
  bool tmp_is_posteriors = false;  // d_tmp holds the [I][S] posteriors of the last E-step
  // d_path_sites holds a decoded path of the loaded data (nghmm_geno_posteriors allocates and
  // zeroes it before any decode)
  bool path_decoded = false;
  // IBD tracts (capi_tracts.hip): per (individual, segment) counts / offsets, carried sums, the
  // chromosome-start mask and scan scratch; the records (raw, then compacted) and their offsets
  DevScratch<uint8_t> d_tseg, d_trec;
  // sampled paths (capi_sample.hip): maps, lane-chunk statistics, kept paths of one batch of draws
  DevScratch<uint8_t> d_samp;
  // observed information (capi_info.hip): the points, the waves' jets, the records
  DevScratch<uint8_t> d_info;
  // region and site summaries (capi_summary.hip): piece, region and site records, the pieces
  DevScratch<uint8_t> d_summ;
  // pairwise sharing (capi_sharing.hip): the K-splits' partial matrices, the result, the
  // thresholded bytes
  DevScratch<uint8_t> d_share;
  // tract support (capi_support.hip): the ranges, their pieces and scores, the boundary vectors
  DevScratch<uint8_t> d_supp;
  // tract bounds (capi_bounds.hip): the boundary vectors, then each pass's ranges, offsets and pieces
  DevScratch<uint8_t> d_bnd;
  // per-site likelihood in the frequency (capi_freqinfo.hip): the boundary vectors, the cavity
  // weights of every cell, the site records and the curve
  DevScratch<uint8_t> d_finfo;
  // genotype posteriors under the HMM (capi_genosmooth.hip): the boundary vectors, the cavity
  // weights of every cell, the posteriors, the calls, the records and the pieces
  DevScratch<uint8_t> d_gsm;
  // expectations over IBD paths (capi_expect.hip): the regions, their pieces and records, the
  // boundary vectors, the site records; and, only when site records are asked for, the per-cell
  // terms (32 bytes per cell) in an owner of their own
  DevScratch<uint8_t> d_expt;
  DevScratch<double> d_expt_cell;
  // posterior moments of IBD share and tract count (capi_moments.hip): the piece and segment
  // tables, the centred jets of the pieces and of the segments, the backward vectors, the records
  DevScratch<uint8_t> d_mom;
  // expected IBD above a minimum tract length (capi_bylength.hip): the regions, their pieces and
  // records, the lane-chunk maps and scans, the b_k and cum tables, the boundary vectors and the
  // halo; and the per-cell planes (36 bytes per cell) in an owner of their own
  DevScratch<uint8_t> d_byl;
  DevScratch<uint8_t> d_byl_cell;
  double byl_qmax = 0;   // the largest |Q| of the last call (nghmm_debug_bylength_qmax)
  // the longest IBD tract (capi_longest.hip): the segments, tables, parts, boundary vectors, lane
  // states and records; the per-cell planes (40 bytes per cell); the lanes' rings
  DevScratch<uint8_t> d_lng;
  DevScratch<uint8_t> d_lng_cell;
  DevScratch<uint8_t> d_lng_ring;
  // per-site posterior of lying in a long IBD tract (capi_long.hip): the regions, pieces and
  // records, the lane-chunk scans, the b_k and lo_k tables, the boundary vectors and the halos; the
  // packed records and P (40 bytes per cell, and 8 more when post is asked for); the cells
  // themselves are d_byl_cell's
  DevScratch<uint8_t> d_long;
  DevScratch<uint8_t> d_long_cell;
  DevBuf<double> d_freq_new, d_hap;  // --freq_est 2 as intended: [S], [S][4]

  // multi-GPU shard
  uint64_t I_tot = 0, ind_begin = 0, site_begin = 0, S_own = 0;
  DevBuf<double> d_gl_shard;

  // packed handle (NGHMM_GENO_PACKED): called genotypes as 2-bit codes (glview.hpp); d_gl
  // does not exist
  bool packed = false;
  DevBuf<uint32_t> d_codes;           // [S][I] cells, 16 per word (a replica borrows its parent's)
  DevBuf<uint32_t> d_codes_shard;     // [S_own][I_tot] cells of the frequency step's site range
  DevBuf<double> d_cls_log;           // [4][3] prepared log likelihoods of the four classes (borrowed likewise)
  double h_cls_proto[12] = {0};       // ... as nghmm_create prepared them (row 3: the reader's
                                      // missing genotype); a load starts from these
  DevBuf<unsigned long long> d_uniform;     // the one value every uniform cell carries (~0: none yet)
  // chunked loading (nghmm_load_begin .. nghmm_load_end)
  uint64_t lkl_redone = 0;            // objective points re-evaluated by the general kernel
  // fast-mode M-step after its first round: the individuals in two halves, each with its own
  // buffers and events, so that the host advances one half's optimizers while the GPU
  // evaluates the other half's points (mstep_indf_impl)
  struct LklAsync {
    Event ev0, ev1, ev_done;
    DevScratch<double> d_lkl;   // device results
    PinScratch<double> h_lkl;   // pinned host results
    DevBuf<int> d_flags;
    PinBuf<int> h_flags;
    std::vector<uint32_t> ind;
    std::vector<double> F, A;
    uint64_t lo = 0, hi = 0;
    bool pending = false;
  } lane[2];
  // Background work of a fused EM iteration (mstep_indf_impl): the E-step's backward sweep and
  // the allele-frequency step do not depend on the objective rounds after the first, so they
  // go onto the stream in pieces right behind each round's kernels and run while the host
  // digests that round's values.  Error flags of their own (the rounds clear theirs), a pool
  // of timing events (one pair per piece, read when the iteration ends).
  struct BgSpan {
    Event ev0, ev1;
    int slot = 0;
  };
  DevBuf<int> d_flags_bg;
  bool flags_bg_clear = false;   // the last iteration's epilogue kernel left d_flags_bg zeroed
  std::vector<BgSpan> bg_spans;
  size_t bg_used = 0;
  // replicas (nghmm_create_replica): share the parent's data arrays (d_gl / d_codes /
  // d_cls_log / d_pos and the fast-mode layouts of the likelihoods)
  nghmm_handle* parent = nullptr;
  std::atomic<int> n_replicas{0};
  // member of a group (nghmm_group_setup): exchange buffers on this handle's device and a
  // second stream for the peer copies, which run under the remaining objective rounds
  int g_n = 0, g_rank = 0;
  DevBuf<double> g_send, g_recv, g_freq_own, g_freq_all;
  // member of an in-process chain of site shards (nghmm_chain_setup): the exchange buffers of
  // fast.shard on this handle's device and the chain's shared state
  struct ChainCtx* chain = nullptr;
  DevBuf<double> c_send, c_recv;   // (chain_release gives them back when the chain dissolves)
  bool loading = false;
  // sites that have arrived since nghmm_load_begin, as disjoint [begin, end) runs: every site
  // must arrive exactly once (a repeated site would OR two codes into a packed cell)
  std::map<uint64_t, uint64_t> load_cover;
  DevScratch<double> d_stage;         // staging buffer of one chunk of raw likelihoods
  DevScratch<int8_t> d_stage8;        // ... of one chunk of reader genotypes

  FastState fast;  // fast-mode layouts (kernels_fast.hip)
  BfgsBatch batch;  // one L-BFGS-B state machine per individual, storage reused across M-steps
  // fast mode keeps the posteriors tile-major (fast.post); the site-major copy d_marg is
  // made on demand (host read-back, multi-GPU packing, est_maf beyond 4096 individuals)
  bool marg_valid = false;

  std::vector<double> h_indF, h_alpha;
  double ms[NSLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t launches[NSLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace capi {

hipError_t sync_stream(nghmm_t* h);
int use_device(nghmm_t* h);
void tic(nghmm_t* h);
int toc(nghmm_t* h, int slot, bool accumulate);
int clear_flags(nghmm_t* h);
int check_flags(nghmm_t* h, const int* d_flags = nullptr);
int ensure_points(nghmm_t* h, size_t n);
GlView own_gl(const nghmm_t* h);
int ensure_tmp(nghmm_t* h);
int ensure_marg(nghmm_t* h);
// Scratch of the Viterbi forward sweep (d_vit), allocated once for the default chunk; *chunk = the
// sites per chunk of this decode (switch viterbi_chunk: never more than the default), *state = the
// carried scores [I][2], which sit behind THAT chunk's transition logs (where
// launch_viterbi_fwd_exact, given *chunk, reads and leaves them)
int viterbi_scratch(nghmm_t* h, uint64_t* chunk, double** state = nullptr);
int fast_estep_impl(nghmm_t* h, double* ind_lkl, bool have_walk);
int redo_nonfinite(nghmm_t* h, uint32_t n_pts, const uint32_t* ind, const double* F,
                   const double* alpha, double* lkl);
int lkl_batch_impl(nghmm_t* h, uint32_t n_pts, const uint32_t* ind, const double* F,
                   const double* alpha, double* lkl, bool accumulate, bool* emit_estep = nullptr);
int lane_setup(nghmm_t* h, int k, size_t n);
int lkl_submit(nghmm_t* h, int k);
int lkl_wait(nghmm_t* h, int k);
int emission_impl(nghmm_t* h);
int bg_begin(nghmm_t* h);
int bg_open(nghmm_t* h, int slot, hipStream_t st = nullptr);   // (st: where the piece runs; default the handle's stream)
int bg_close(nghmm_t* h, hipStream_t st = nullptr);
int bg_finish(nghmm_t* h);
int ensure_emissions(nghmm_t* h);

// est_maf on the handle's own sites and individuals or on its frequency-step site range
int estmaf_and_refresh(nghmm_t* h, bool shard, const double* d_marg_blocks, uint64_t S_own,
                       uint64_t I_tot, uint64_t I_blk, double* d_freq_out);
// leaves its chain, which dissolves (capi_multi.hip)
void chain_release(nghmm_t* h);
// the IBD tracts of one handle (handle-local sites), all of them, to the host (capi_tracts.hip)
int tracts_to_host(nghmm_t* h, int source, double threshold, uint64_t min_sites,
                   std::vector<nghmm_tract>& out);
// source / threshold of nghmm_ibd_tracts; sets the error message
int tracts_check_args(nghmm_t* h, int source, double threshold, const char* who);
// nghmm_ibd_summary's argument checks (capi_summary.hip); they set the error message
int summary_check_source(nghmm_t* h, int what, double threshold, const char* who);
int summary_check_regions(uint64_t S, uint64_t I, uint64_t n_regions, const uint64_t* begin,
                          const uint64_t* end, const void* regions, const void* sites,
                          const char* who);
// a region in handle-local sites; first: begin is the region's own first site (false: the region
// goes on from the site shard before, whose last decoded state is summary_to_host's prev_state)
struct SummaryRegion {
  uint64_t begin, end;
  bool first;
};
// The regions of one handle (sorted, disjoint, inside [0, S)) cut into pieces at the segment
// edges (the multiples of kSummarySeg), in site order: pieces, seg_piece [summary_segments(S) + 1]
// (the first piece of every segment) and piece_first [regs.size() + 1] (the first piece of every
// region), as launch_summary_pass and the finish kernels take them
void summary_cut_pieces(const std::vector<SummaryRegion>& regs, uint64_t S, std::vector<SummaryPiece>& pieces,
                        std::vector<uint32_t>& seg_piece, std::vector<uint32_t>& piece_first);
// the summary of one handle to the host: regions [I][regs.size()] (NULL iff there are none),
// sites [S] (may be NULL); prev_state [I] (host, may be NULL = all 0)
int summary_to_host(nghmm_t* h, int what, double thr, const std::vector<SummaryRegion>& regs,
                    const uint8_t* prev_state, nghmm_region_stat* regions, nghmm_site_stat* sites);
// out[I] (host) = the decoded state at the handle's last site
int summary_last_state(nghmm_t* h, uint8_t* out);
// nghmm_ibd_sharing's argument checks (capi_sharing.hip); they set the error message
int sharing_check_args(nghmm_t* h, int what, double threshold, const void* vit_both,
                       const void* post_both, const void* post_prod, const char* who);
int sharing_check_range(uint64_t S, uint64_t site_begin, uint64_t site_end, const char* who);
// the sharing matrices [I][I] of one handle over its sites [begin, end) to the host; a NULL
// output is not computed
int sharing_to_host(nghmm_t* h, double thr, uint64_t begin, uint64_t end, uint64_t* vit_both,
                    uint64_t* post_both, double* post_prod);
// The cavity weights (1 - c, c) of every cell of a handle or a chain of site shards, at the
// CURRENT indF, alpha and freq (capi_cavity.hip; kernels_freqinfo.hpp has the walks): the
// segments, the forward walks from the first shard to the last, the backward walks from the last
// to the first, the boundary vectors through the host.  The scratch of shard r lives in
// hs[r]->*owner: the walks' own, then extra_bytes(r) bytes for the caller (256-byte aligned).
// Behind shard r's backward walk, on its stream and with its device current, shard_done(r, d_cav
// [S][I][2], the caller's bytes) queues what the caller makes of the weights, checks the handle's
// flags (check_flags: a NaN weight raises FLAG_INVALID_LKL) and copies its results out.
// The callers check their arguments first: every handle holds data, a chain of more than one is
// fast mode.
int cavity_walks(nghmm_t** hs, int n, DevScratch<uint8_t> nghmm_handle::*owner,
                 const std::function<uint64_t(int)>& extra_bytes,
                 const std::function<int(int, const double*, uint8_t*)>& shard_done, const char* who);

}  // namespace capi
