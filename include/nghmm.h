/*
 * nghmm.h -- C ABI of the MI355X-native ngsF-HMM EM hot path.
 *
 * The reference (fgvieira/ngsF-HMM v1.1.0) has no plugin/FFI interface: its EM
 * engine (EM.cpp) calls its numerical routines (shared/HMM.hpp:8-15,
 * shared/gen_func.hpp:94-103, shared/bfgs.h:54-57) directly through pthread-pool
 * tasks (EM.cpp:385-445).  This header is the seam a maintainer would bind
 * instead: each entry point names the reference call sites it replaces.  All
 * per-site-per-individual arithmetic runs in HIP kernels on one GPU per handle;
 * large state stays device-resident between calls.
 *
 * Conventions
 *   - plain pointers and sizes only; `double` is IEEE binary64;
 *   - sites are 0-based here: site s is the reference's site s+1; the
 *     reference's virtual site 0 is implicit;
 *   - every function returns 0 (NGHMM_OK) or a negative code; the codes -1..-5
 *     correspond to the reference's fatal error() messages, which a host maps
 *     back to the same text (nghmm_strerror); nghmm_last_error() gives detail;
 *   - host buffers are owned by the caller, device buffers by the handle;
 *   - a handle is bound to one HIP device and one stream; calls on different
 *     handles may be made from different threads.
 */
#ifndef NGHMM_H
#define NGHMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nghmm_handle nghmm_t;

enum {
  NGHMM_OK = 0,
  NGHMM_ERR_INVALID_LKL = -1, /* "invalid Lkl found!"          shared/HMM.cpp:18-21,45-48 */
  NGHMM_ERR_FW_BW = -2,       /* "Fw and Bw lkl do not match!" EM.cpp:166-170 */
  NGHMM_ERR_INVALID_MAF = -3, /* "invalid MAF!"                shared/HMM.cpp:145-146 */
  NGHMM_ERR_NAN = -4,         /* "value is NaN!"               shared/gen_func.cpp:56-57 */
  NGHMM_ERR_FREQ_EST2 = -5,   /* "invalid allele frequencies": --freq_est 2 aborts in the
                                 reference at the first site (EM.cpp:235-238,
                                 shared/gen_func.cpp:1030-1031) */
  NGHMM_ERR_ARG = -10,        /* bad argument / call order */
  NGHMM_ERR_HIP = -11,        /* HIP runtime error */
  NGHMM_ERR_NOMEM = -12,
  NGHMM_ERR_NOT_PACKABLE = -13 /* a packed handle met a cell that is not a called genotype */
};

/* Arithmetic mode of a handle. */
enum {
  /* Log-space recursions in the reference's operation order, exp/log from
   * csrc/detmath.h: results are bit-identical to the oracle's `det` build. */
  NGHMM_MODE_EXACT = 0,
  /* Linear-space, chunk-parallel scan over sites with rescaling (the
   * throughput path); per-call results within 1e-9 relative of exact mode. */
  NGHMM_MODE_FAST = 1,
  /* OR-ed into the mode: the genotype likelihoods are CALLED GENOTYPES (--call_geno, or a
   * called-genotype input file; ngsF-HMM.cpp:101-117, shared/read_data.cpp:88-98,
   * shared/gen_func.cpp:886-914), of which every cell is one of four -- genotype 0, 1, 2
   * or missing -- and is kept as a 2-bit code (0.25 B instead of 24 B per site and
   * individual).  Results equal those of an unpacked handle given the same cells: bit for bit
   * in exact mode.  A loader that meets a cell which is not a called genotype (one-hot or
   * uniform likelihoods) returns NGHMM_ERR_NOT_PACKABLE -- the host then falls back to an
   * unpacked handle; NGHMM_ERR_ARG is for input that is wrong either way: a reader genotype
   * > 2, or uniform cells carrying different values within one data set. */
  NGHMM_GENO_PACKED = 0x10
};

/* Statistics of one indF/alpha M-step (shared/bfgs.cpp rounds). */
typedef struct {
  uint32_t rounds;          /* objective rounds: the longest sequence of evaluations any
                               individual needed (= lock-step launches when every round
                               covers all individuals; the two-lane M-step launches more) */
  uint64_t points;          /* objective evaluations sent to the GPU                */
  uint64_t ref_forward_calls; /* forward passes the reference would have spent      */
  uint64_t ind_rounds;      /* sum over rounds of the individuals still being optimised:
                               each costs one pass over that individual's emissions */
} nghmm_mstep_stats;

/* The message of the last failing call ON THE CALLING THREAD (thread-local storage: handles may
 * be driven from several host threads -- replicas, the members of a group or chain -- and each
 * thread sees its own calls' messages; a failure inside a library-owned worker thread of
 * nghmm_group_* / nghmm_chain_* is carried back to the thread that made the call).  Valid until
 * that thread's next library call; "" when that call succeeded. */
const char* nghmm_last_error(void);
const char* nghmm_strerror(int code);
/* 1 if the library was built with its HIP kernels (always, for the shipped .so). */
int nghmm_has_hip(void);

/* Create the state for n_ind individuals x n_sites sites on HIP device `device`
 * (replaces the allocations of read_geno/init_output, shared/read_data.cpp:21,
 * parse_args.cpp:245-412, and iter_EM's per-iteration Fw/Bw, EM.cpp:140-143). */
int nghmm_create(nghmm_t** out, uint64_t n_ind, uint64_t n_sites, int device, int mode);
int nghmm_destroy(nghmm_t* h);

/* Multi-start (ngsF-HMM.sh:77-101 runs 20 replicates from different random starts and keeps
 * the one with the best likelihood): a REPLICA shares its parent's genotype likelihoods and
 * distances on the device (read-only, loaded once) and owns everything an EM run writes --
 * parameters, emissions, posteriors, optimizer state -- and its own HIP stream, so R replicas
 * driven from R host threads run R independent EM analyses concurrently on one GPU.  Every
 * call behaves exactly as on an independent handle loaded with the same data.  The parent must
 * be loaded, must not be reloaded while replicas exist and must be destroyed last. */
int nghmm_create_replica(nghmm_t** out, nghmm_t* parent);

/* Upload genotype likelihoods: natural-log, normalised, site-major [S][I][3]
 * (= the reference's binary --geno file order, shared/read_data.cpp:28-31, after
 * its normalisation) and per-site distances in Mb, +inf at chromosome starts
 * (ngsF-HMM.cpp:75-86).  Host pointers. */
int nghmm_load_gl(nghmm_t* h, const double* gl_site_major, const double* pos_dist_mb);
/* Same from RAW genotype likelihoods as they come out of the input file, prepared on the
 * device in the reference's operation order: conversion to log space, normalisation
 * (shared/read_data.cpp:36-40,89-98), optional genotype calling and second normalisation
 * (ngsF-HMM.cpp:101-117; call_geno, shared/gen_func.cpp:886-914, with its defaults).
 * space: how the values are encoded, see below.  check_nan != 0: a NaN cell after the first
 * normalisation returns NGHMM_ERR_NAN ("NaN found! Is the file format correct?",
 * read_data.cpp:42-45: the reference checks binary input only). */
enum {
  NGHMM_GL_LOG = 0,          /* natural-log likelihoods (--loglkl, or called genotypes) */
  NGHMM_GL_NORMAL_BINARY = 1, /* normal space, binary file: log 0 becomes -1e15 (conv_space) */
  NGHMM_GL_NORMAL_TEXT = 2    /* normal space, text file: plain log (log 0 = -inf)         */
};
/* A cell the reader never filled (the reference lets an empty text line consume a site,
 * read_data.cpp:60-61: its cells keep the initial -1e15 and see only the second
 * normalisation): its FIRST value carries this quiet-NaN bit pattern. */
#define NGHMM_GL_UNREAD_BITS 0x7ff8dead00000001ull
int nghmm_load_gl_raw(nghmm_t* h, const double* gl_raw_site_major, int space, int call_geno,
                      int check_nan, const double* pos_dist_mb);

/* Same, from buffers already resident on the handle's device. */
int nghmm_load_gl_device(nghmm_t* h, const double* d_gl_site_major, const double* d_pos_dist_mb);

/* Chunked loading, for inputs that should never exist in one piece on the host (the file
 * goes to the device a block of sites at a time; read_geno, shared/read_data.cpp:13-116,
 * holds the whole matrix): nghmm_load_begin with the distances, then every site exactly once
 * in chunks [site_begin, site_begin + n_sites) of any size and order, then nghmm_load_end.
 * "Exactly once" is checked: a chunk that overlaps sites this load has already received is
 * NGHMM_ERR_ARG (nothing of it is taken), and so is nghmm_load_end before all n_sites have
 * arrived.  A chunk that fails for another reason (NGHMM_ERR_NAN, NGHMM_ERR_NOT_PACKABLE, a
 * genotype > 2) may have left cells behind: it ends the load, which starts again with
 * nghmm_load_begin.
 *   nghmm_load_gl_raw_sites      raw likelihoods [n_sites][I][3] as nghmm_load_gl_raw takes them
 *   nghmm_load_gl_raw_sites_dev  the same from a device buffer (left unmodified)
 *   nghmm_load_geno_sites        called genotypes [n_sites][I] as the reader sees them, -1
 *                                (missing), 0, 1, 2 (shared/read_data.cpp:88-98); a value > 2 is
 *                                NGHMM_ERR_ARG ("Genotypes must be coded as {-1,0,1,2} !")
 * The whole-matrix loaders above are these three calls in a row.
 * Device buffers (the _dev / _device loaders): the library runs on a stream of its own that
 * waits for no other, so these calls wait for the WHOLE device (hipDeviceSynchronize) before
 * they read the caller's buffer -- whatever stream wrote it, it is complete. */
int nghmm_load_begin(nghmm_t* h, const double* pos_dist_mb);
int nghmm_load_begin_dev(nghmm_t* h, const double* d_pos_dist_mb);
int nghmm_load_gl_raw_sites(nghmm_t* h, uint64_t site_begin, uint64_t n_sites,
                            const double* gl_raw, int space, int call_geno, int check_nan);
int nghmm_load_gl_raw_sites_dev(nghmm_t* h, uint64_t site_begin, uint64_t n_sites,
                                const double* d_gl_raw, int space, int call_geno, int check_nan);
int nghmm_load_geno_sites(nghmm_t* h, uint64_t site_begin, uint64_t n_sites, const int8_t* geno);
int nghmm_load_end(nghmm_t* h);

/* indF[I], alpha[I], freq[S]; NULL leaves a vector unchanged (parse_args.cpp:245-363). */
int nghmm_set_params(nghmm_t* h, const double* indF, const double* alpha, const double* freq);
int nghmm_get_params(nghmm_t* h, double* indF, double* alpha, double* freq);

/* Emission probabilities of every cell from the current freq
 * (calc_emission, shared/HMM.cpp:144-154, as called at parse_args.cpp:381-386). */
int nghmm_emission(nghmm_t* h);

/* E-step: forward, backward, Fw/Bw consistency check, posteriors
 * (EM.cpp:147-185; shared/HMM.cpp:6-60).  ind_lkl[I] (host, may be NULL). */
int nghmm_estep(nghmm_t* h, double* ind_lkl);

/* Objective of the indF/alpha M-step for a batch of probe points: lkl[p] =
 * forward log-likelihood of individual ind[p] with q = (1-F[p], F[p]) and
 * transition rate alpha[p], under the current emissions (EM.cpp:449-464 returns
 * its negative).  Host pointers. */
int nghmm_lkl_batch(nghmm_t* h, uint32_t n_pts, const uint32_t* ind, const double* F,
                    const double* alpha, double* lkl);

/* indF/alpha M-step for all individuals: one bound-constrained L-BFGS-B problem
 * per individual (EM.cpp:198-201,423-440; shared/bfgs.cpp:83-138), advanced in
 * lock-step rounds with nghmm_lkl_batch as the objective.  stats may be NULL. */
int nghmm_mstep_indf(nghmm_t* h, int indF_fixed, int alpha_fixed, nghmm_mstep_stats* stats);

/* The same lock-step batched L-BFGS-B machinery with a caller-supplied objective
 * (host only, no GPU involved): fn returns the forward log-likelihood of
 * individual `ind` at (F, alpha).  indF/alpha are updated in place.  Lets a host
 * plug another objective in, and lets the CPU test-suite exercise the state
 * machines without a device. */
typedef double (*nghmm_objective_fn)(uint32_t ind, double F, double alpha, void* user);
int nghmm_bfgs_batch_host(uint64_t n_ind, double* indF, double* alpha, int indF_fixed,
                          int alpha_fixed, nghmm_objective_fn fn, void* user,
                          nghmm_mstep_stats* stats);
/* The same with flags: 1 = the finite-difference step eh = (1e-8 (|x| + 1))^0.67
 * (shared/bfgs.cpp:33) by the library's own exp / log instead of libm's pow (what fast mode
 * uses: host and device then agree bit for bit); 2 = run the solver type the device runs
 * (kernels_bfgs.hip), one problem after the other.  Test hook: both give identical bits. */
int nghmm_bfgs_batch_host2(uint64_t n_ind, double* indF, double* alpha, int indF_fixed,
                           int alpha_fixed, nghmm_objective_fn fn, void* user,
                           nghmm_mstep_stats* stats, int flags);

/* Allele-frequency M-step + emission refresh (EM.cpp:210-272; est_maf,
 * shared/gen_func.cpp:974-1009).  freq_est 0 = keep, 1 = per-site EM,
 * 2 = NGHMM_ERR_FREQ_EST2 (the reference aborts).
 *
 * OPT-IN, PARITY UNPINNED -- --freq_est 2 / --e_prob 2 AS INTENDED.  The reference aborts on
 * both at the first site (EM.cpp:235-238 -> shared/gen_func.cpp:1030-1031), so there is no
 * reference output; what is computed is its loop (EM.cpp:224-263) as written -- sites in
 * order, frequencies updated in place, haplotype frequencies of every adjacent site pair by
 * the pair EM of gen_func.cpp:1027-1119 -- with its three defects repaired the smallest way
 * (no pair step at the first site; the normal-space pair iteration, the log-space one loses a
 * logsum at :1160; the LD emission of EM.cpp:258-260 reachable).  Asked for by OR-ing
 * NGHMM_LD_INTENDED into freq_est:
 *   2 | NGHMM_LD_INTENDED                    freq[s] from the pair's haplotype frequencies
 *   2 | NGHMM_LD_INTENDED | NGHMM_EPROB_LD   ... and emissions by calc_emissionLD
 *                                            (shared/HMM.cpp:175-236) past the first site
 *   1 | NGHMM_LD_INTENDED | NGHMM_EPROB_LD   est_maf frequencies, LD emissions
 * NGHMM_EPROB_LD needs NGHMM_MODE_EXACT (materialised emissions).  One unsharded handle, at
 * most 8192 individuals; the chain through the sites is sequential by its definition.  Plain
 * 2 keeps returning the reference's abort. */
enum { NGHMM_LD_INTENDED = 0x20, NGHMM_EPROB_LD = 0x40 };
int nghmm_mstep_freq(nghmm_t* h, int freq_est);

/* E-step + indF/alpha M-step of one EM iteration (EM.cpp:147-201) in one call.  In fast
 * mode the two share a pass over the emissions: the M-step's first objective evaluation
 * f(x) at the current parameters (EM.cpp:449-464) IS the E-step's forward walk, so it runs
 * first and leaves the lane operators and checkpoints the E-step's backward sweep needs;
 * results are those of nghmm_estep followed by nghmm_mstep_indf.  after_estep (may be
 * NULL) is called once on the calling thread as soon as the posteriors are final, before
 * the remaining objective rounds: a multi-GPU host starts its posterior exchange there. */
typedef void (*nghmm_hook_fn)(void* user);
int nghmm_estep_mstep(nghmm_t* h, int indF_fixed, int alpha_fixed, double* ind_lkl,
                      nghmm_mstep_stats* stats, nghmm_hook_fn after_estep, void* user);

/* One whole EM iteration = iter_EM (EM.cpp:139-289). */
int nghmm_iter_em(nghmm_t* h, int freq_est, int indF_fixed, int alpha_fixed, double* ind_lkl,
                  nghmm_mstep_stats* stats);

/* Viterbi decoding with the current parameters (EM.cpp:105-116;
 * shared/HMM.cpp:98-125).  path[I][S] bytes 0/1 (host). */
int nghmm_viterbi(nghmm_t* h, uint8_t* path);

/* Posterior of the IBD state from the last E-step, marg_prob[i][s][1], as
 * [I][S] doubles (host) -- what EM.cpp:347-353 prints. */
int nghmm_get_posteriors(nghmm_t* h, double* marg_ibd);
/* Prepared genotype likelihoods [S][I][3] (natural log, normalised) back to the host:
 * what nghmm_load_gl_raw made of its input. */
int nghmm_get_gl(nghmm_t* h, double* gl_site_major);
/* Genotype posteriors of the .geno output (EM.cpp:367-376) for the sites
 * [site_begin, site_begin + n_sites): out[n_sites][n_ind][3] (host, normal space), with the
 * path of the last nghmm_viterbi call as the prior's F (all zeros before the first call, like
 * the reference's path[][] at an intermediate print_iter) and the current frequencies. */
int nghmm_geno_posteriors(nghmm_t* h, uint64_t site_begin, uint64_t n_sites, double* out);
/* The posterior lines of the .ibd file (EM.cpp:347-353) as text, formatted on the device:
 * for the individuals [ind_begin, ind_begin + n_ind) one line each of n_sites values
 * printed like printf("%f") -- "d.dddddd", the digits glibc prints -- separated by tabs and
 * ended by a newline, i.e. exactly 9 * n_sites bytes per individual; out (host) receives
 * n_ind * 9 * n_sites bytes. */
int nghmm_format_posteriors(nghmm_t* h, uint64_t ind_begin, uint64_t n_ind, char* out);
/* The formatter behind it, for caller-supplied values in [0, 1] (host): rows lines of cols
 * "%f" values, 9 * rows * cols bytes.  NGHMM_ERR_ARG if a value is outside [0, 1]. */
int nghmm_format_fixed6(nghmm_t* h, const double* values, uint64_t rows, uint64_t cols, char* out);

/* ---- IBD tracts ----
 * What scripts/convert_ibd.pl --ibd_pos makes of the .ibd file (convert_ibd.pl:99-130: one BED
 * line per maximal run of 1 in an individual's Viterbi path on one chromosome), called on the
 * device from the state the run left there -- the decoded path and the posteriors that
 * EM.cpp:338-353 prints -- without the file.
 *
 * A tract of individual i is a maximal run of consecutive sites [a, b] such that every site in
 * it is in state IBD and no site in (a, b] starts a chromosome (distance +inf).  In state IBD:
 *   NGHMM_TRACTS_VITERBI    path[i][s] == 1 of the last nghmm_viterbi / nghmm_chain_viterbi
 *                           decode of the loaded data (NGHMM_ERR_ARG if there was none since the
 *                           load); threshold is ignored
 *   NGHMM_TRACTS_POSTERIOR  marg_prob[i][s][1] >= threshold, threshold in (0, 1] (else, NaN
 *                           included, NGHMM_ERR_ARG): the value nghmm_get_posteriors returns
 * post_sum = the sum of marg_prob[i][s][1] over the tract's sites (the posteriors of the last
 * E-step, zeros before the first), added piece by piece in site order: the same bits on every
 * call.  Tracts of fewer than min_sites sites are dropped; records are ordered by
 * (ind, first_site). */
enum { NGHMM_TRACTS_VITERBI = 0, NGHMM_TRACTS_POSTERIOR = 1 };
typedef struct nghmm_tract {  /* 32 bytes */
  uint64_t first_site;        /* handle-local (single handle) or global (chain) */
  uint64_t n_sites;
  uint32_t ind;
  uint32_t reserved;          /* 0 */
  double post_sum;
} nghmm_tract;
/* Tracts of one handle (convert_ibd.pl:99-130 on the path EM.cpp:338-353 prints): *n_total
 * receives the number of tracts, out (host) the first min(cap, *n_total) of them; out may be
 * NULL when cap == 0.  Device scratch grows with the number of tracts (NGHMM_ERR_NOMEM when it
 * cannot be had). */
int nghmm_ibd_tracts(nghmm_t* h, int source, double threshold, uint64_t min_sites,
                     nghmm_tract* out, uint64_t cap, uint64_t* n_total);
/* The same over a chain of site shards (nghmm_chain_setup; convert_ibd.pl:99-130,
 * EM.cpp:338-353): global site indices; a tract that crosses a shard boundary is one tract
 * unless the next shard's first site starts a chromosome; min_sites applies AFTER merging;
 * post_sum = the sum of the pieces in site order.  (Chains of more than one handle are fast
 * mode only, as nghmm_chain_setup requires.) */
int nghmm_chain_ibd_tracts(nghmm_t** hs, int n, int source, double threshold,
                           uint64_t min_sites, nghmm_tract* out, uint64_t cap,
                           uint64_t* n_total);

/* ---- IBD paths sampled from the joint posterior ----
 * Whole paths z drawn from P(z | data, theta) by forward filtering and backward sampling, with
 * the handle's CURRENT parameters and emissions (as nghmm_viterbi uses them, not the last
 * E-step's): what neither the Viterbi path (one path) nor the per-site posteriors (marginals of
 * strongly dependent neighbours) give -- the distribution of anything that spans more than one
 * site: the number of tracts, the longest one, the share of the genome that is IBD.  (The
 * reference has no such function; the forward vector is that of shared/HMM.cpp:6-28.)
 *
 * Definition.  For individual i let a_s(k) ~ P(z_s = k, y_1..s) be the forward vector at site s,
 * c_s = exp(-alpha_i d_s) (0 where d_s = +inf: a chromosome start), q = (1 - F_i, F_i) and
 * T_s(k, l) = (1 - c_s) q_l + [k = l] c_s.  A draw is
 *     z_{S-1}:  1 if u_{S-1} (a(0) + a(1)) < a(1)                       (a = a_{S-1})
 *     z_s    :  1 if u_s (n0 + n1) < n1,  n_k = a_s(k) T_{s+1}(k, z_{s+1}),   s = S-2 ... 0
 * (compared by multiplication; at a chromosome start T does not depend on k and z_s is drawn from
 * a_s alone).  u is a function of (seed, draw, individual, GLOBAL site) only: Philox4x32-10
 * (csrc/philox.h) with key = (seed low 32, seed high 32), counter = (p low 32, p high 32,
 * individual, draw), p = global site >> 1; an even site takes the output words (x0, x1), an odd
 * one (x2, x3); u = (((uint64)x_hi << 32 | x_lo) >> 11) 2^-53, x_lo the first word of the pair.
 * Nothing else enters: not the launch geometry, not n_draws or n_keep, not the sharding.  (The
 * forward vectors carry the mode's rounding -- fast mode within 1e-9 of exact mode -- so two modes
 * or layouts can differ at a site whose u lies that close to its threshold, and from there on.)
 *
 * Per (draw, individual) the device reduces the path to a record, so that many draws never need
 * their paths stored; ibd_mb adds the distances d_s of the sites s that continue a tract, per
 * lane-chunk of the layout and then chunk by chunk in site order -- no atomics: the same bits on
 * every call. */
typedef struct nghmm_path_stats {  /* 32 bytes */
  uint64_t ibd_sites;      /* sites in state 1 */
  uint64_t n_tracts;       /* maximal runs of 1 within a chromosome (nghmm_ibd_tracts' definition) */
  uint64_t longest_sites;  /* sites of the longest such run, 0 if none */
  double ibd_mb;           /* sum over tracts of the distance from first to last site, in Mb */
} nghmm_path_stats;
/* n_draws paths per individual, draw d from (seed, d): stats [n_draws][I] (host, may be NULL);
 * the first n_keep <= n_draws draws are returned as paths [n_keep][I][S] bytes 0/1 (host; NULL iff
 * n_keep == 0).  NGHMM_ERR_ARG for a handle without data, n_draws == 0, n_keep > n_draws, a NULL
 * mismatch.  Leaves the handle's Viterbi path, posteriors and parameters alone. */
int nghmm_sample_paths(nghmm_t* h, uint64_t seed, uint32_t n_draws, nghmm_path_stats* stats,
                       uint32_t n_keep, uint8_t* paths);
/* The same over a chain of site shards (nghmm_chain_setup; the forward vector of
 * shared/HMM.cpp:6-28 continued from shard to shard): paths [n_keep][I][all sites], global site
 * indices in the generator; the forward vectors travel left to right and the sampled states right
 * to left, as in nghmm_viterbi_shard_forward / _back; tracts and ibd_mb that cross a shard
 * boundary are merged as nghmm_chain_ibd_tracts merges them. */
int nghmm_chain_sample_paths(nghmm_t** hs, int n, uint64_t seed, uint32_t n_draws,
                             nghmm_path_stats* stats, uint32_t n_keep, uint8_t* paths);

/* ---- support of a tract: joint posterior and log-odds of a whole run of sites ----
 * How far to trust ONE tract: the posterior probability that individual i is IBD at EVERY site of
 * a closed range [a, b] -- not the sum or mean of the per-site marginals (nghmm_tract.post_sum),
 * which for strongly dependent neighbours says little about the run as a whole -- and the same for
 * non-IBD throughout, exactly and without counting sampled paths.  (The reference has no such
 * function; hap-ibd's LOD and bcftools roh's quality play this role elsewhere.)
 *
 * Definition.  At the handle's CURRENT parameters and emissions (as nghmm_viterbi,
 * nghmm_sample_paths and nghmm_obs_info use them, not the last E-step's), with f and beta the
 * forward and backward vectors, T_s and q as in the sampler's definition above, e_s the emissions
 * and Z the likelihood, for k in {0, 1}:
 *     P(z_a..b = k | y) = f_a(k) prod_{s = a+1..b} T_s(k, k) e_s(k)  beta_b(k) / Z
 *   log_p_ibd      ln P(z_a = ... = z_b = 1 | y, theta)
 *   log_p_non      ln P(z_a = ... = z_b = 0 | y, theta)
 *   post_min       the smallest P(z_s = 1 | y, theta) over s in [a, b] (unsnapped: not rounded to
 *                  0 / 1 within 1e-5 as the E-step's posteriors are)
 *   post_min_site  the lowest site that attains it -- where the tract is most likely to be two;
 *                  handle-local for a single handle, global for a chain
 * At a chromosome start inside (a, b], T_s(k, k) = q_k: the quantity stays defined, and a range
 * need not stay within a chromosome.  A state that the data exclude gives -inf, never NaN: once a
 * factor is 0 the result is -inf, and a 0/0 factor after that counts as 0.
 * The LOD of a tract is (log_p_ibd - log_p_non) / ln 10: the log-odds of IBD throughout against
 * non-IBD throughout, the rest of the genome marginalised.  It is derived by the callers (the
 * Python binding, the command line), not stored.
 *
 * Evaluation.  Every factor has a scale-free local form,
 *     P(z_a..b = k | y) = P(z_a = k | y) prod_{s = a+1..b} P(z_s = k | z_{s-1} = k, y_s..),
 *     P(z_s = k | z_{s-1} = k, y_s..) = T_s(k, k) e_s(k) beta_s(k) / beta_{s-1}(k)
 * (the mirror image of the sampler's P(z_s | z_{s+1}, y_1..s)), in which a common factor of the two
 * emissions cancels.  Fast mode carries the product of a range's factors inside one lane-chunk of
 * the layout as a double in [0.5, 1) with an integer exponent, rescaled after every factor, and
 * takes one logarithm per lane-chunk and state; exact mode adds the factors' logarithms (detmath.h)
 * site by site.  No float atomics: a range that spans several lane-chunks or shards is the sum of
 * its pieces in site order, the minimum is taken in site order with ties to the lowest site -- the
 * same bits on every call, and for a record the same bits whichever other records are passed.
 *  */
typedef struct nghmm_tract_score {  /* 32 bytes */
  double log_p_ibd, log_p_non, post_min;
  uint64_t post_min_site;
} nghmm_tract_score;
#ifdef __cplusplus
static_assert(sizeof(nghmm_tract_score) == 32, "nghmm_tract_score is 32 bytes");
#endif
/* tracts [n] (host): only ind, first_site and n_sites are read; out [n] (host), aligned with it.
 * The ranges must be ordered by (ind, first_site) and disjoint within an individual: what
 * nghmm_ibd_tracts returns from either source, and equally hand-made ranges such as a gene per
 * individual.  n == 0 returns NGHMM_OK and touches nothing.  NGHMM_ERR_ARG, with a message that
 * names the first offending record, for n_sites == 0, a range outside the data, ind >= I, wrong
 * order or overlap; also for a NULL pointer with n > 0 and a handle without data.
 * Self-contained like nghmm_obs_info: it refreshes stale emissions itself and leaves parameters,
 * the posteriors of the last E-step, the Viterbi path, checkpoints and an M-step planned in
 * advance untouched; an EM iteration after the call gives the bits it would have given without it.
 * Device scratch grows with n and with the lane-chunks the ranges touch (NGHMM_ERR_NOMEM when it
 * cannot be had) and is kept by the handle. */
int nghmm_tract_support(nghmm_t* h, const nghmm_tract* tracts, uint64_t n, nghmm_tract_score* out);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices; the forward vectors travel from the first shard to the last and the backward vectors
 * from the last to the first, I x 2 doubles per boundary, as nghmm_chain_sample_paths moves its
 * vectors and states; a range that crosses a shard boundary is the sum of its shards' parts in
 * site order, added on the host.  (Chains of more than one handle are fast mode only.) */
int nghmm_chain_tract_support(nghmm_t** hs, int n_handles, const nghmm_tract* tracts, uint64_t n,
                              nghmm_tract_score* out);

/* ---- bounds of a tract: credible intervals for its two ends ----
 * Where a tract really starts and ends, and how likely two neighbouring calls are one tract --
 * exactly, without keeping sampled paths.  (The reference has no such function.)
 *
 * Definition.  Everything uses the handle's CURRENT parameters and emissions, as
 * nghmm_tract_support does; f, beta, T_s, q, e_s, Z as there.  Of a record only ind, first_site
 * and n_sites are read: its CORE.  Record k has
 *   anchor       c_k.  anchor[k] if given (it must lie inside the core); with anchor == NULL or
 *                anchor[k] == UINT64_MAX the site of the core with the smallest P(z_s = 0 | y),
 *                the lowest such site on ties.  P(z_s = 0 | y) is formed directly, not as
 *                1 - P(z_s = 1 | y): inside a tract the latter saturates at 1 over many sites
 *                while the former keeps its relative precision.  Anchors are strictly ascending
 *                within an individual.
 *   left_limit   max(first site of c_k's chromosome, c_{k-1}); c_{k-1} only where record k - 1
 *                belongs to the same individual
 *   right_limit  min(last site of c_k's chromosome, c_{k+1}), likewise.  A chromosome starts at
 *                site 0 and at every site with distance +inf.
 *   G(s) = P(z_s = ... = z_c = 1 | y) / P(z_c = 1 | y),   left_limit <= s <= c
 *   H(s) = P(z_c = ... = z_s = 1 | y) / P(z_c = 1 | y),   c <= s <= right_limit;  G(c) = H(c) = 1.
 * With the local factors of the support, g_t = T_t(1,1) e_t(1) beta_t(1) / beta_{t-1}(1):
 *   H(s) = prod_{t = c+1..s} g_t,   G(s) = P(z_s = 1 | y) prod_{t = s+1..c} g_t / P(z_c = 1 | y).
 * Both fall monotonically away from the anchor.  levels [n_levels], 1 <= n_levels <= 8, each in
 * (0, 1), strictly descending:
 *   start[k][m]  the lowest s with G(t) >= levels[m] for every t in [s, c]
 *   end[k][m]    the highest s with H(t) >= levels[m] for every t in [c, s]
 * Given z_c = 1, P(true start <= s) = G(s): [start(0.025), start(0.975)] is a 95 % interval of the
 * start and start(0.5) its median; [end(0.975), end(0.025)] is the interval of the end.
 *   post_anchor      P(z_c = 1 | y), unsnapped
 *   log_reach_left   ln G(left_limit)
 *   log_reach_right  ln H(right_limit)
 * Where the limit is a neighbour's anchor, the reach is the probability that the two tracts are
 * one run from anchor to anchor.  A level is CENSORED on a side when the answer equals the limit:
 * when reach >= level.
 * A factor 0 makes everything beyond it 0 (-inf); a 0/0 factor counts as 0; nothing is ever NaN.
 * With post_anchor == 0 every start and end is the anchor and both reaches are -inf.
 * Site indices are handle-local for one handle and global for a chain.
 *
 * Evaluation.  Between two consecutive anchors one set of factors serves the
 * search to the right of the one and to the left of the other.  Fast mode: three walks of the
 * shape of the support's -- the anchors; ln prod g per lane-chunk piece of every stretch between
 * two limits, which the host adds in site order (and in rank order over the shards of a chain);
 * and, knowing the value at every piece's edge, the first failing site per level from the anchor
 * outwards.  Exact mode: the same three passes, one lane per individual in log space.  No float
 * atomics; the same bits on every call; a record's results depend only on that record and its two
 * neighbours in the call. */
typedef struct nghmm_tract_bound {  /* 48 bytes */
  uint64_t anchor, left_limit, right_limit;
  double post_anchor, log_reach_left, log_reach_right;
} nghmm_tract_bound;
#ifdef __cplusplus
static_assert(sizeof(nghmm_tract_bound) == 48, "nghmm_tract_bound is 48 bytes");
#endif
/* tracts [n], anchor [n] or NULL, levels [n_levels], out [n], start and end [n][n_levels] (all
 * host).  The records are checked as nghmm_tract_support checks them, with its messages; an anchor
 * outside its core and bad levels (count, range, order, NaN) are NGHMM_ERR_ARG too.  n == 0
 * returns NGHMM_OK and touches nothing; a NULL pointer other than anchor with n > 0, and a handle
 * without data, are NGHMM_ERR_ARG.  Self-contained and read-only exactly like nghmm_tract_support:
 * it refreshes stale emissions itself and leaves parameters, posteriors, Viterbi path, checkpoints
 * and a planned M-step untouched; an EM iteration after the call gives the bits it would have
 * given without it.  Device scratch is kept by the handle. */
int nghmm_tract_bounds(nghmm_t* h, const nghmm_tract* tracts, uint64_t n, const uint64_t* anchor,
                       const double* levels, uint32_t n_levels, nghmm_tract_bound* out,
                       uint64_t* start, uint64_t* end);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices; the boundary vectors travel as in nghmm_chain_tract_support; every shard reports the
 * pieces of a search that crosses a boundary, the host adds them in rank order and gives each
 * shard its offsets for the locating pass.  (Chains of more than one handle are fast mode only.) */
int nghmm_chain_tract_bounds(nghmm_t** hs, int n_handles, const nghmm_tract* tracts, uint64_t n,
                             const uint64_t* anchor, const double* levels, uint32_t n_levels,
                             nghmm_tract_bound* out, uint64_t* start, uint64_t* end);

/* ---- per-site likelihood in the allele frequency: score, information and curve ----
 * What the data of the whole cohort say about ONE site's allele frequency f_s, with indF, alpha
 * and every other site's frequency held at the handle's current values: the uncertainty of
 * freq[s], a per-site fit score, and how far est_maf's fixed point (gen_func.cpp:974-1009, a
 * mean-field step that feeds the posterior -- which already contains the site's own data -- in as
 * a fractional F) is from a stationary point of the likelihood the rest of the program optimises.
 * (The reference has no such function.)
 *
 * Definition.  For one individual the data of site s enter the likelihood Z_i only through the two
 * emissions of that site, and Z_i is linear in them:
 *     Z_i = C_i [ (1 - c_is) e0_is(f_s) + c_is e1_is(f_s) ],
 *     c_is = P(z_is = 1 | all data of individual i except site s's), the CAVITY probability:
 *            (f_{s-1} T_s)(k) beta_s(k), k = 0, 1, normalised -- the forward prediction before the
 *            emission of s is applied (at site 0 and at a chromosome start: the stationary vector
 *            (1 - F_i, F_i)), times the backward vector;
 *     e0 = p0 (1 - f)^2 + 2 p1 f (1 - f) + p2 f^2,   e1 = p0 (1 - f) + p2 f,   p_g = exp(gl_g)
 * (calc_emission, HMM.cpp:144-154, with calc_HWE's F = 0 and F = 1: the heterozygote has prior 0
 * under IBD).  c_is and C_i do not depend on f_s, so up to a constant the log-likelihood of the
 * cohort as a function of f_s alone is EXACTLY
 *     l_s(f) = sum_i ln[ (1 - c_is) e0_is(f) + c_is e1_is(f) ],
 * every term the logarithm of a quadratic in f.  Everything is evaluated at the handle's CURRENT
 * indF, alpha and freq (as nghmm_tract_support does, with walks of its own): the posteriors of the
 * last E-step will not do -- they are snapped to 0 / 1 within 1e-5 (EM.cpp:184) and one parameter
 * update old -- and are not looked at, nor is the decoded path.
 *
 *   cavity [I][S]   c_is.  The two weights (1 - c) and c are each formed from their own
 *                   unnormalised product, never as 1 - c, so either end keeps its relative
 *                   precision; the sums below use those two weights.
 *   stats [S]       freq   the frequency the record was evaluated at, freq[s]
 *                   ll     l_s(freq): the leave-one-site-out predictive log-likelihood of the
 *                          site's data, a per-site fit score
 *                   score  dl_s/df at freq = sum_i u_i,
 *                          u_i = [(1 - c) e0' + c e1'] / [(1 - c) e0 + c e1]
 *                   info   -d2l_s/df2 at freq = sum_i (u_i^2 - (1 - c) e0'' / [(1 - c) e0 + c e1])
 *                          (e1'' = 0)
 *   curve [S][n_levels]  curve[s][k] = l_s(levels[k]) - l_s(freq[s]), formed as the sum over i of
 *                   ln(ratio of the two brackets), not as a difference of two sums.
 *                   0 <= n_levels <= 8, every level in [0, 1].  Levels 0 and 1 are legal: there
 *                   e0 = e1 = p0 (resp. p2), so -2 curve is a likelihood-ratio statistic against
 *                   a monomorphic site.
 * 1 / sqrt(info) is a standard error of freq[s] CONDITIONAL on indF, alpha and the other sites'
 * frequencies (the cross terms are not formed: if anything it is too small), and only where
 * info > 0 and 0 < freq < 1.  score at est_maf's frequency need not be 0, for the reason above.
 *
 * Zero likelihoods (called genotypes at level 0 or 1): an individual whose bracket is 0 at a level
 * makes that curve entry -inf; if it is 0 at the current frequency, ll = -inf and score, info and
 * the site's curve are NaN.  Otherwise nothing is NaN.
 *
 * Evaluation.  The results are the same bits however the sites are cut into
 * shards, so the vectors cannot come from the E-step's lane-chunk operators and checkpoints (a
 * product of operators is rounded along its grouping, which belongs to a handle's layout).  Fast
 * mode: two plain vector recursions in linear space over the likelihoods and the frequencies, one
 * site after the other, one lane per individual and chromosome -- a chromosome's first site
 * restarts both exactly: its prediction is defined as (1 - F, F), the backward vector in front of
 * it as (1, 1), the scale of a vector being free --; the backward one leaves the two weights of
 * every cell.  Exact mode: one lane per individual in log space (detmath.h), both vectors
 * normalised at every site.  Then a site pass over the weights and the likelihoods.  No float
 * atomics: a site's sums run over the individuals in blocks of 64; within a block (filled up
 * with zeros) the 64 values are added as a butterfly -- x_i += x_{i ^ 32}, then ^ 16, 8, 4, 2, 1 --;
 * the blocks are added in order, the first one's value first (nghmm_ibd_summary's rule for
 * post_sum).  The same bits on every call, whichever outputs are asked for; a site's result
 * depends only on that site's cells and the cavity. */
typedef struct nghmm_freq_stat {  /* 32 bytes; one per site */
  double freq, ll, score, info;
} nghmm_freq_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_freq_stat) == 32, "nghmm_freq_stat is 32 bytes");
#endif
/* levels [n_levels], stats [S], curve [S][n_levels], cavity [I][S] (all host).  stats and cavity
 * may be NULL; curve is NULL iff n_levels == 0 (levels is not read then); at least one of the three
 * outputs is not NULL.  NGHMM_ERR_ARG, with a message, for n_levels > 8, a level outside [0, 1]
 * (NaN included), a NULL mismatch, all outputs NULL, and a handle without data.
 * Self-contained and read-only: parameters, emissions, the posteriors of the last E-step, the
 * Viterbi path, checkpoints and an M-step planned in advance stay as they are; an EM iteration
 * after the call gives the bits it would have given without it.  Both modes form the emissions
 * they need from the likelihoods and the current frequencies themselves, so frequencies installed
 * with nghmm_set_params count at once, with or without nghmm_emission, and the stored emissions
 * are neither read nor written.  A NaN in the walks raises the invalid-likelihood error of the
 * E-step (an individual whose likelihood is 0 on a chromosome of more than one site gives one); a
 * NaN that arises in a site's sums stays in the record.  Device scratch, kept by the handle: 16 bytes per cell for the two weights, 8
 * more when cavity is asked for, and the records (NGHMM_ERR_NOMEM when it cannot be had). */
int nghmm_freq_info(nghmm_t* h, uint32_t n_levels, const double* levels, nghmm_freq_stat* stats,
                    double* curve, double* cavity);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site order,
 * the outputs are the concatenation of the shards' (cavity [I][all sites]).  The forward vectors
 * travel from the first shard to the last and the backward vectors from the last to the first,
 * I x 2 doubles per boundary, the way nghmm_chain_tract_support moves its vectors; a shard goes on
 * from them with the single handle's own operations, so the bytes equal the single handle's.
 * (Chains of more than one handle are fast mode only.)  Groups of individual shards
 * (nghmm_group_*) are out of scope, as for nghmm_ibd_summary. */
int nghmm_chain_freq_info(nghmm_t** hs, int n_handles, uint32_t n_levels, const double* levels,
                          nghmm_freq_stat* stats, double* curve, double* cavity);

/* ---- genotype posteriors under the HMM: calls, heterozygosity, the EM update of a frequency ----
 * The posterior of a cell's genotype given ALL data of the individual, with the IBD state of the
 * site summed out exactly.  nghmm_geno_posteriors (the reference's print_iter) uses the hard
 * Viterbi state as the site's inbreeding coefficient: one wrongly decoded site flips the prior of
 * the heterozygote between 2f(1 - f) and 0, and no heterozygote can be called where the path says
 * IBD.  Putting the marginal posterior there (EM.cpp:371, commented out) counts the site's own
 * data twice.  (The reference has no such function.)
 *
 * Definition.  For cell (i, s), at the handle's CURRENT indF, alpha and freq:
 *     (w0, w1) = (1 - c, c), the two cavity weights exactly as nghmm_freq_info defines and forms
 *                them (each from its own product, never as 1 - x);
 *     p_g = exp(gl_g), f = freq[s];
 *     h0 = ((1 - f)^2, 2 f (1 - f), f^2),  h1 = (1 - f, 0, f)     (calc_HWE with F = 0 and F = 1)
 *     J[z][g] = w_z h_z[g] p_g                      six products; J[1][1] = 0
 *     B       = sum J = (1 - c) e0 + c e1           nghmm_freq_info's bracket
 *     P_g     = (J[0][g] + J[1][g]) / B             the smoothed genotype posterior
 *     pi      = (J[1][0] + J[1][2]) / B             the smoothed IBD posterior (unsnapped)
 *     non     = (J[0][0] + J[0][1] + J[0][2]) / B   1 - pi, from its own sum
 * J / B is the joint posterior of (z_is, g_is) given all data of individual i: it equals the
 * enumeration over all paths.  A called genotype (one p_g = 1, the others 0) has B equal to its
 * one numerator: the posterior is one-hot exactly.  A missing cell gets the cavity-weighted prior.
 *
 *   post [S][I][3]   P_0, P_1, P_2 (site-major: the cell order of nghmm_geno_posteriors)
 *   call [S][I]      the g with the largest P_g, ties to the lowest g; 3 where B = 0 or the
 *                    posterior is NaN
 *   sites [S]        sums over the individuals:
 *                    n0, n1, n2   P_g: the expected genotype counts
 *                    het_prior    w0 2 f (1 - f): the heterozygotes expected before the site's own
 *                                 data are seen (n1 / het_prior far above 1 marks paralogous or
 *                                 mis-mapped sites)
 *                    ibd          pi
 *                    alt_ibd      J[1][2] / B: the IBD individuals that carry the alternative allele
 *   regions [I][n_regions]   sums over the region's sites:
 *                    het          P_1
 *                    het_prior    w0 2 f (1 - f)
 *                    non_ibd      non
 *                    dosage       P_1 + 2 P_2
 *                    het / non_ibd is the heterozygosity outside IBD; het / het_prior the excess
 *                    against the model.
 * Two identities.  (a) The EXACT EM update of f_s under the model is alternative allele copies over
 * allele copies, an IBD individual carrying one copy:
 *     em_freq = (n1 + 2 n2 - alt_ibd) / (2 I - ibd),
 * and by Fisher's identity  score f (1 - f) = (n1 + 2 n2 - alt_ibd) - f (2 I - ibd)  with
 * nghmm_freq_info's score: em_freq - freq is that score in frequency units, 0 exactly where the
 * likelihood is stationary in f_s (est_maf's mean-field step need not end there).  (b) Called
 * genotypes give one-hot posteriors, see above.
 * Everything is CONDITIONAL on indF, alpha and the frequencies, as nghmm_freq_info's results are.
 *
 * Dead cells.  B = 0 only where a called genotype meets a frequency of 0 or 1 that excludes it:
 * the cell has NaN in post and 3 in call, and the NaN stays in the sums it enters (all of a site's
 * and a region's but het_prior).  Nothing else is ever NaN.
 *
 * Evaluation.  The walks of nghmm_freq_info, then one pass over the weights
 * and the likelihoods.  No float atomics.  A site's sums run over the individuals in blocks of 64;
 * within a block (filled up with zeros) a butterfly -- x_i += x_{i ^ 32}, then ^ 16, 8, 4, 2, 1 --;
 * the blocks are added in order, the first one's value first (nghmm_freq_info's rule).  A region's
 * sums follow nghmm_ibd_summary's rule for post_sum: the region is cut at the multiples of 2048 of
 * the handle's own sites, every piece is summed from 0 in site order, and the pieces are added in
 * site order, the first one's value first.  The same bits on every call, and every output's bits
 * do not depend on which other outputs are asked for. */
typedef struct nghmm_geno_site_stat {  /* 48 bytes; one per site */
  double n0, n1, n2, het_prior, ibd, alt_ibd;
} nghmm_geno_site_stat;
typedef struct nghmm_geno_region_stat {  /* 32 bytes; one per individual and region */
  double het, het_prior, non_ibd, dosage;
} nghmm_geno_region_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_geno_site_stat) == 48, "nghmm_geno_site_stat is 48 bytes");
static_assert(sizeof(nghmm_geno_region_stat) == 32, "nghmm_geno_region_stat is 32 bytes");
#endif
/* region_begin, region_end [n_regions], regions [I][n_regions], sites [S], post [S][I][3], call
 * [S][I] (all host).  Regions are nghmm_ibd_summary's: half-open [begin, end), sorted, disjoint,
 * not empty, inside the data; regions, region_begin and region_end are NULL iff n_regions == 0.
 * Every output may be NULL; at least one is not.  NGHMM_ERR_ARG, with a message, for a handle
 * without data, all outputs NULL, the NULL mismatch and bad regions.
 * Self-contained and read-only exactly like nghmm_freq_info: it forms its own emissions from the
 * likelihoods and the current frequencies, and leaves parameters, emissions, posteriors, Viterbi
 * path, checkpoints and a planned M-step untouched; an EM iteration after the call gives the bits
 * it would have given without it.  A NaN in the walks raises the invalid-likelihood error, as
 * there.  Device scratch, kept by the handle in an owner of its own: 16 bytes per cell for the
 * weights, 24 more when post is asked for, 1 more for call, and the records (NGHMM_ERR_NOMEM when
 * it cannot be had). */
int nghmm_geno_smooth(nghmm_t* h, uint64_t n_regions, const uint64_t* region_begin,
                      const uint64_t* region_end, nghmm_geno_region_stat* regions,
                      nghmm_geno_site_stat* sites, double* post, uint8_t* call);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices.  post, call and sites are the concatenation of the shards' and THE SINGLE HANDLE'S
 * BYTES: they depend only on the cell and on the cavity, which has that property
 * (nghmm_chain_freq_info).  A region that crosses a cut is one region, its shards' parts added on
 * the host in rank order: within rounding of the single handle's sums, not their bytes, as for
 * nghmm_chain_ibd_summary.  (Chains of more than one handle are fast mode only.) */
int nghmm_chain_geno_smooth(nghmm_t** hs, int n_handles, uint64_t n_regions,
                            const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_geno_region_stat* regions, nghmm_geno_site_stat* sites,
                            double* post, uint8_t* call);

/* ---- observed information of indF and alpha ----
 * Per individual the log-likelihood, its gradient and its 2x2 Hessian in (F, alpha) at one point,
 * from EXACT derivatives carried through one forward pass (no finite differences): what standard
 * errors of the two estimates, their correlation, and a convergence diagnostic (the gradient at
 * the final parameters) are made of.  (The reference has no such function.)
 *
 * Definition.  l_i(F, alpha) is the forward log-likelihood of individual i that nghmm_lkl_batch
 * defines: under the handle's CURRENT EMISSIONS, with q = (1 - F, F) and c_s = exp(-alpha d_s)
 * (0 where d_s = +inf: a chromosome start).  A site is the operator M_s = (c_s I + (1 - c_s) 1 q^T)
 * diag(e_s), l_i = log(q prod_s M_s 1); the product rule carries dM/dF, dM/dalpha and the three
 * second derivatives along with the product.  THE ALLELE FREQUENCIES ARE HELD FIXED: the
 * emissions do not move with (F, alpha), so standard errors derived from these records are
 * CONDITIONAL ON THE FREQUENCIES (they ignore the uncertainty of the frequency estimates and
 * are, if anything, too small).
 *
 * g_* and h_* are the first and second partial derivatives of l_i itself, not of -l_i: the
 * observed information is -h.  h_xy is formed as Z_xy / Z - g_x g_y (Z the likelihood), which
 * loses about eps |g_x g_y / h_xy| to cancellation far from an optimum.
 * No float atomics: one order of operations, the same bits on every call. */
typedef struct nghmm_info {  /* 48 bytes */
  double lkl;                /* l_i */
  double g_F, g_A;           /* dl/dF, dl/dalpha */
  double h_FF, h_FA, h_AA;   /* d2l/dF2, d2l/dF dalpha, d2l/dalpha2 */
} nghmm_info;
#ifdef __cplusplus
static_assert(sizeof(nghmm_info) == 48, "nghmm_info is six doubles");
#endif
/* out[I] (host).  F and alpha are host [I] arrays: the point of every individual; NULL for BOTH
 * means the handle's current parameters.  NGHMM_ERR_ARG for exactly one NULL, for a point outside
 * the box of EM.cpp:424-438 (F in [1e-15, 1 - 1e-15], alpha in [1e-15, 10]) or NaN, for out ==
 * NULL, for a handle without data.  Self-contained like nghmm_viterbi and nghmm_sample_paths: it
 * refreshes stale emissions itself and leaves parameters, posteriors, the Viterbi path,
 * checkpoints and an M-step planned in advance untouched. */
int nghmm_obs_info(nghmm_t* h, const double* F, const double* alpha, nghmm_info* out);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): every shard
 * reduces its site range to one jet per individual (24 doubles and an exponent), the host
 * multiplies them in rank order and closes once.  (Chains of more than one handle are fast mode
 * only.) */
int nghmm_chain_obs_info(nghmm_t** hs, int n, const double* F, const double* alpha, nghmm_info* out);

/* ---- IBD per region and per site ----
 * The two reductions of the decoded path [I][S] and the posteriors [I][S] that an .ibd file is
 * most often read back for, made on the device where the run left both arrays, in one pass over
 * them: along the sites, per individual and REGION -- the share of a chromosome or of a window
 * that is IBD (F_ROH per chromosome, a genome scan) and its IBD length in Mb --, and along the
 * individuals, per SITE -- how many individuals are IBD there (ROH islands).  (The reference has
 * no such function.)
 *
 * Regions are half-open ranges of sites [region_begin[r], region_end[r]) with begin < end <= S,
 * sorted, not overlapping; gaps are allowed, and a site in no region counts for no region.  Site
 * indices are handle-local for one handle and global for a chain.  A region may span chromosome
 * starts: the vit_mb rule skips the infinite distance there.  The site before a region's first
 * site never contributes to vit_mb.
 *
 * `what` is a bit mask of the sources:
 *   NGHMM_SUMMARY_VITERBI    path[i][s] of the last nghmm_viterbi / nghmm_chain_viterbi decode of
 *                            the loaded data (NGHMM_ERR_ARG if there was none since the load)
 *   NGHMM_SUMMARY_POSTERIOR  marg_prob[i][s][1], the values nghmm_get_posteriors returns (zeros
 *                            before the first E-step); threshold in (0, 1], else -- NaN included --
 *                            NGHMM_ERR_ARG (the threshold is not looked at without this source)
 * The fields of a source that was not asked for are 0.  what == 0 or an unknown bit:
 * NGHMM_ERR_ARG.
 *
 * regions [I][n_regions] (host) is NULL iff n_regions == 0 (then region_begin and region_end are
 * not read); sites [S] (host) may be NULL; at least one of the two is not.  NGHMM_ERR_ARG also for
 * a handle without data, for unsorted, overlapping or empty regions, for end > S, and for a NULL
 * mismatch.
 *
 * No float atomics; every double is added in one fixed order that does not depend on the call:
 * the same bits on every call.  post_sum and vit_mb of a region: the region is cut at the
 * multiples of 2048 sites (of the handle's own sites); within a piece the terms are added to 0 in
 * site order; the pieces are added in site order, the first one's value first.  post_sum of a
 * site: the individuals in blocks of 64; within a block (filled up with zeros) the 64 values are
 * added as a butterfly -- x_i += x_{i ^ 32}, then ^ 16, 8, 4, 2, 1 --; the blocks are added in
 * order, the first one's value first.  
 *
 * Read-only: parameters, posteriors, the Viterbi path, checkpoints and an M-step planned in
 * advance stay as they are; an EM iteration after the call gives the bits it would have given
 * without it.  Device scratch grows with I x (n_regions + S / 2048) and with S
 * (NGHMM_ERR_NOMEM when it cannot be had) and is kept by the handle.
 *
 * Groups of individual shards (nghmm_group_*) are out of scope: every member summarises its own
 * individuals, and a site's records of the members are the caller's to add. */
enum { NGHMM_SUMMARY_VITERBI = 1, NGHMM_SUMMARY_POSTERIOR = 2 };
typedef struct nghmm_region_stat {  /* 32 bytes; one per (individual, region) */
  uint64_t vit_sites;   /* sites of the region with path[i][s] == 1 */
  uint64_t post_sites;  /* sites of the region with marg_prob[i][s][1] >= threshold */
  double post_sum;      /* sum of marg_prob[i][s][1] over the region's sites */
  double vit_mb;        /* sum of d_s over the region's sites s > region begin with
                           path[i][s-1] == path[i][s] == 1 and d_s finite: IBD length in Mb,
                           the per-region counterpart of nghmm_path_stats.ibd_mb */
} nghmm_region_stat;
typedef struct nghmm_site_stat {    /* 16 bytes; one per site */
  uint32_t vit_count;   /* individuals with path[i][s] == 1 */
  uint32_t post_count;  /* individuals with marg_prob[i][s][1] >= threshold */
  double post_sum;      /* sum over individuals of marg_prob[i][s][1] */
} nghmm_site_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_region_stat) == 32 && sizeof(nghmm_site_stat) == 16, "record sizes");
#endif
int nghmm_ibd_summary(nghmm_t* h, int what, double threshold, uint64_t n_regions,
                      const uint64_t* region_begin, const uint64_t* region_end,
                      nghmm_region_stat* regions, nghmm_site_stat* sites);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices; sites [all sites] is the concatenation of the shards' records (each computed on its
 * own device exactly as for one handle: the same bytes); a region that crosses a shard boundary
 * is one region -- every shard reduces its part of it, the parts are added on the host in rank
 * order --, and vit_mb at a shard's first site looks at the last decoded state of the shard
 * before: one byte per individual, moved through the host the way nghmm_viterbi_shard_back moves
 * state_before.  (Chains of more than one handle are fast mode only, as nghmm_chain_setup
 * requires.) */
int nghmm_chain_ibd_summary(nghmm_t** hs, int n, int what, double threshold, uint64_t n_regions,
                            const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_region_stat* regions, nghmm_site_stat* sites);

/* ---- exact expectations over IBD paths: tracts, breakpoints, path entropy ----
 * How many tracts an individual has, how long they are in Mb, where tract ends concentrate, and
 * how uncertain the decode is as a whole -- exactly, where nghmm_sample_paths gives them by Monte
 * Carlo with error 1 / sqrt(draws): closed-form sums of the posterior's pairwise marginals
 * P(z_{s-1}, z_s | y), which the per-site posteriors (marginals of strongly dependent neighbours,
 * and stored snapped to 0 / 1 within 1e-5) cannot give.  (The reference has no such function.)
 *
 * Definition.  At the handle's CURRENT parameters and emissions (as nghmm_tract_support and
 * nghmm_sample_paths use them, not the last E-step's), for individual i, with f and beta the
 * forward and backward vectors, T_s, q and c_s as in the sampler's definition above, e_s the
 * emissions: for a site s that is NOT a chromosome start
 *     m_s(k, l)  = T_s(k, l) e_s(l) beta_s(l)
 *     n_s(k, l)  = f_{s-1}(k) m_s(k, l)
 *     xi_s(k, l) = n_s(k, l) / sum_{k,l} n_s(k, l)            = P(z_{s-1} = k, z_s = l | y)
 *     r_s(k, l)  = m_s(k, l) / (m_s(k, 0) + m_s(k, 1))        = P(z_s = l | z_{s-1} = k, y)
 * and pi_s(l) = P(z_s = l | y) = xi_s(0, l) + xi_s(1, l), unsnapped.  Each of the four entries is
 * formed from its own product, never as 1 - x; a common factor of the two emissions cancels.  At a
 * chromosome start (d_s = +inf, and a handle's or chain's first site) T_s does not depend on k:
 * z_s is independent of z_{s-1} given y, and the site contributes through pi_s alone.
 *
 *   term      not a chromosome start                     chromosome start
 *   ibd_s     pi_s(1)                                    pi_s(1)
 *   start_s   xi_s(0, 1)   (a tract begins at s)         pi_s(1)
 *   on_s      xi_s(0, 1)                                 0
 *   off_s     xi_s(1, 0)                                 0
 *   mb_s      d_s xi_s(1, 1)                             0
 *   h_s       -sum_{k,l} xi_s(k, l) ln r_s(k, l)         -sum_l pi_s(l) ln pi_s(l)
 *   lp_s      ln r_s(z*_{s-1}, z*_s)                     ln pi_s(z*_s)
 * mb_s is the expectation of the term nghmm_path_stats.ibd_mb adds; h_s uses 0 ln 0 = 0; lp_s is
 * only formed with NGHMM_EXPECT_VITERBI, z* being the last nghmm_viterbi / nghmm_chain_viterbi
 * decode of the loaded data.  The posterior is a Markov chain given y, so over all sites
 *     sum start_s = E[n_tracts],  sum ibd_s = E[ibd_sites],  sum mb_s = E[ibd_mb]
 * (nghmm_path_stats' definitions: tracts are cut at chromosome starts),
 *     sum h_s = H(z | y), the entropy of the path posterior in nats,
 *     sum lp_s = ln P(z* | y), the posterior probability of the decoded path itself.
 * A state the data exclude (a heterozygote among called genotypes) makes its xi entries exactly 0;
 * entropy terms with xi = 0 are 0; a 0/0 conditional counts as 0 as in nghmm_tract_support, so
 * log_p_path may be -inf.  Nothing is ever NaN.
 *
 * regions [I][n_regions] (host): every field is the sum of the per-cell terms over the region's
 * sites.  Regions are nghmm_ibd_summary's: half-open, sorted, disjoint, gaps allowed, handle-local
 * indices for one handle and global for a chain.  EVERY site contributes its own term, a region's
 * first site included, and that term looks at the site before it -- unlike vit_mb's rule, which
 * leaves the step into a region's first site out.  So the records of regions that partition the
 * data add up to the whole, and `starts` counts the tracts that BEGIN inside the region.
 * sites [S] (host): each field is the sum over the individuals of on_s, off_s, ibd_s, h_s.
 * regions is NULL iff n_regions == 0; sites may be NULL; at least one of the two is not.
 *
 * `what` is 0 or NGHMM_EXPECT_VITERBI (log_p_path is 0 without it).  NGHMM_ERR_ARG, with a
 * message: the bit set and no decode since the load; an unknown bit; a handle without data; both
 * outputs NULL, a NULL mismatch, unsorted, overlapping or empty regions, end > S.
 *
 * Evaluation and the order of every sum.  ln r comes from the small side: with x = min / max of
 * the pair m(k, 0), m(k, 1), the larger entry's ln r is -log1p(x) and the smaller one's
 * ln(x) - log1p(x) (both terms <= 0: no cancellation).  Exact mode: log1p(x) is u = 1 + x,
 * u == 1 ? x : det_log(u) x / (u - 1).  Fast mode: log1p(x) = 2 atanh(x / (2 + x)) and ln(x) from
 * the same odd series on the mantissa, both to relative accuracy (csrc/kernels_expect.hip).  So
 * the entropy and log_p_path of an almost certain genome, sums of a million
 * tiny terms of one sign, keep relative accuracy.  No float atomics.  Fast mode: a region is cut
 * into pieces at the lane-chunk edges of the handle's layout (multiples of T sites,
 * nghmm_fast_layout); within a piece the terms are added to 0 from the piece's LAST site to its
 * first; the pieces are added in site order, the first one's value first.  Exact mode: one piece,
 * from the region's last site to its first.  A site record: the individuals in blocks of 64; within
 * a block (filled up with zeros) the butterfly x_i += x_{i ^ 32}, then ^ 16, 8, 4, 2, 1; the blocks
 * in order, the first one's value first -- as nghmm_ibd_summary's post_sum.  The same bits on every
 * call, and a region's record does not depend on which other regions or outputs are asked for.
 * 
 *
 * Self-contained and read-only exactly like nghmm_tract_support: it refreshes stale emissions
 * itself and leaves parameters, the posteriors of the last E-step, the Viterbi path, checkpoints
 * and an M-step planned in advance untouched; an EM iteration after the call gives the bits it
 * would have given without it.  Device scratch, kept by the handle: 48 bytes per (individual,
 * piece) and (individual, region); and ONLY when sites is asked for, in a buffer of its own, the
 * per-cell terms: 32 bytes per cell (individual x site, fast mode: x padded site)
 * (NGHMM_ERR_NOMEM when it cannot be had). */
enum { NGHMM_EXPECT_VITERBI = 1 };
typedef struct nghmm_expect_region {  /* 48 bytes; one per (individual, region) */
  double ibd;         /* sum ibd_s: expected sites in state IBD */
  double starts;      /* sum start_s: expected number of tracts that begin in the region */
  double switches;    /* sum on_s + off_s: expected number of state switches */
  double ibd_mb;      /* sum mb_s: expected IBD length in Mb */
  double entropy;     /* sum h_s, nats */
  double log_p_path;  /* sum lp_s (0 without NGHMM_EXPECT_VITERBI; may be -inf) */
} nghmm_expect_region;
typedef struct nghmm_expect_site {    /* 32 bytes; one per site */
  double on, off, ibd, entropy;  /* sums over the individuals of on_s, off_s, ibd_s, h_s */
} nghmm_expect_site;
#ifdef __cplusplus
static_assert(sizeof(nghmm_expect_region) == 48 && sizeof(nghmm_expect_site) == 32, "record sizes");
#endif
int nghmm_ibd_expect(nghmm_t* h, int what, uint64_t n_regions, const uint64_t* region_begin,
                     const uint64_t* region_end, nghmm_expect_region* regions,
                     nghmm_expect_site* sites);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices; the boundary vectors travel as in nghmm_chain_tract_support and the decoded state at a
 * shard's last site as in nghmm_chain_ibd_summary; a region that crosses a shard boundary is one
 * region, its shards' parts added on the host in rank order; sites [all sites] is the
 * concatenation.  The results are within rounding of a single handle's, not its bytes: the
 * lane-chunk grouping of a region's sum belongs to a handle's layout.  (Chains of more than one
 * handle are fast mode only.) */
int nghmm_chain_ibd_expect(nghmm_t** hs, int n_handles, int what, uint64_t n_regions,
                           const uint64_t* region_begin, const uint64_t* region_end,
                           nghmm_expect_region* regions, nghmm_expect_site* sites);

/* ---- exact posterior variances of IBD share and tract count per region ----
 * nghmm_ibd_expect gives the posterior MEANS of the summaries people publish (F_ROH of a genome, a
 * chromosome or a window, the number of tracts, the IBD length in Mb); this call gives their
 * posterior covariance matrix as well, exactly, where nghmm_sample_paths estimates a variance from
 * R draws with relative error about sqrt(2 / R).  (The reference has no such function.)
 *
 * Definition.  At the handle's CURRENT parameters and emissions, as nghmm_ibd_expect; T_s, q, c_s,
 * e_s, the forward vector f, the backward vector beta and what counts as a chromosome start
 * (d_s = +inf, or the first site of a handle or chain) are those of the sampler's and
 * nghmm_ibd_expect's definitions above.  Every step (z_{s-1} = k, z_s = l) contributes
 *
 *   statistic            not a chromosome start     chromosome start
 *   sites  phiN_s(k, l)  [l = 1]                    [l = 1]
 *   tracts phiT_s(k, l)  [k = 0, l = 1]             [l = 1]
 *   Mb     phiL_s(k, l)  d_s [k = 1, l = 1]         0
 *
 * -- exactly the terms nghmm_path_stats adds to a path's ibd_sites, n_tracts and ibd_mb.  For a
 * region R = [a, b):  A_R = sum_{s in R} phiA_s(z_{s-1}, z_s) with A = N, or A = L with the flag
 * NGHMM_MOMENTS_MB, and T_R = sum_{s in R} phiT_s.  As in nghmm_ibd_expect EVERY site contributes
 * its own term, a region's first site included, and that term looks at the site before it.  With
 * M_s = T_s diag(e_s), the tilted product
 *     Z_R(t) = f_{a-1} [prod_{s=a}^{b-1} M_s o exp(t_A phiA_s + t_T phiT_s)] beta_{b-1}
 * (o entrywise; f_{a-1} = q for a = 0 or the chain's first site, beta = 1 behind the last site; f
 * and beta at t = 0, at any scale) is the moment generating function of (A_R, T_R) given y times a
 * constant, so the gradient of log Z_R at 0 is their posterior mean and the Hessian their
 * posterior covariance matrix -- both exactly:
 *     mean_a = d_A log Z_R(0)  = E[A_R | y]       (nghmm_ibd_expect's `ibd` or `ibd_mb`)
 *     mean_t = d_T log Z_R(0)  = E[T_R | y]       (nghmm_ibd_expect's `starts`)
 *     var_a  = d_AA log Z_R(0) = Var(A_R | y)     (a value that rounds below 0 is returned as 0)
 *     cov_at = d_AT log Z_R(0) = Cov(A_R, T_R | y)
 *     var_t  = d_TT log Z_R(0) = Var(T_R | y)     (the same clamp)
 * **Everything is conditional on indF, alpha and the allele frequencies**, as the results of the
 * other calls are: the uncertainty of the parameters (nghmm_obs_info) is not in these variances.
 * A state the data exclude gives exact zeros where it should (a one-site region on an excluded
 * state has variance exactly 0); nothing is ever NaN.  A one-site region has mean_a = pi_s(1) and
 * var_a = pi_s(1) pi_s(0) with A = sites.  The operator at a chromosome start has rank one, so
 * chromosomes are independent given the parameters: the variances and covariances of regions that
 * are whole chromosomes add up to those of the whole data.
 *
 * regions [I][n_regions] (host).  Regions are nghmm_ibd_summary's: half-open, sorted, disjoint,
 * gaps allowed, handle-local indices for one handle and global for a chain; they may span
 * chromosome starts.  NGHMM_ERR_ARG, with a message: an unknown bit in `what`; a handle without
 * data; n_regions == 0; a NULL pointer; unsorted, overlapping or empty regions; end > S.
 *
 * Evaluation and the order of operations.  The t-derivatives of a tilted site are entrywise masks
 * of M_s, so the product rule to second order in (t_A, t_T) is the jet algebra of nghmm_obs_info
 * (six 2x2 matrices, one exponent).  A plain jet loses digits when it is closed -- Z_AA / Z -
 * (Z_A / Z)^2 cancels like eps E[A]^2 / Var, half the digits at 10^6 sites -- so every partial
 * product carries an offset pair next to its jet and stores the jet of the statistics MINUS the
 * offsets; a product adds the offsets and re-centres them by (sum of the entries of V_a) / (sum of
 * the entries of V) wherever it rescales; closing gives mean = offset + Z_a / Z and the
 * covariances unchanged.  Fast mode: the site axis is partitioned by the region edges into
 * segments (the regions and the gaps, at most 2 n_regions + 1) and the segments at the lane-chunk
 * edges of the layout (multiples of T sites, nghmm_fast_layout) into pieces; a lane multiplies its
 * sites in order, rescaling and re-centring every 8; a wave of 64 lane-chunks that lies in one
 * segment multiplies its lanes in an ordered tree into one piece; a segment's pieces are
 * multiplied in runs of ceil(n / 64) consecutive pieces and the runs in an ordered tree; then per
 * individual the backward vectors from the last segment to the first and the forward vectors from
 * the first to the last through the segments' value components, each scaled to sum 1, closing
 * every region on the way.  Exact mode: per individual a backward pass that keeps beta at the
 * region ends, then a forward pass that carries f times the region's centred jet, rescaled and
 * re-centred every 8 sites, and closes at the region's end.  No float atomics: the same arguments
 * give the same bits on every call.  UNLIKE nghmm_ibd_expect, a region's record may depend in its
 * last bits on which other regions are asked for (f and beta come from the other segments'
 * products); it agrees within rounding.  
 *
 * Self-contained and read-only exactly like nghmm_ibd_expect: it refreshes stale emissions itself
 * and leaves parameters, the posteriors of the last E-step, the Viterbi path, checkpoints and an
 * M-step planned in advance untouched; an EM iteration after the call gives the bits it would
 * have given without it.  Device scratch, kept by the handle (NGHMM_ERR_NOMEM when it cannot be
 * had): fast mode 216 bytes per (individual, piece) -- pieces <= 64 C + 2 n_regions + 1, and C +
 * 2 n_regions + 1 when no region edge falls inside a wave --, 232 bytes per (individual, segment),
 * 40 per (individual, region) and tables of 4 bytes per lane-chunk and 8 per piece; exact mode 56
 * bytes per (individual, region). */
enum { NGHMM_MOMENTS_MB = 1 };
typedef struct nghmm_moment_region {  /* 40 bytes; one per (individual, region) */
  double mean_a;  /* E[A_R | y]: expected IBD sites (or Mb with NGHMM_MOMENTS_MB) */
  double mean_t;  /* E[T_R | y]: expected number of tracts that begin in the region */
  double var_a;   /* Var(A_R | y), >= 0 */
  double cov_at;  /* Cov(A_R, T_R | y) */
  double var_t;   /* Var(T_R | y), >= 0 */
} nghmm_moment_region;
#ifdef __cplusplus
static_assert(sizeof(nghmm_moment_region) == 40, "record size");
#endif
int nghmm_ibd_moments(nghmm_t* h, int what, uint64_t n_regions, const uint64_t* region_begin,
                      const uint64_t* region_end, nghmm_moment_region* regions);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices.  Each shard reduces its site range to the centred jets of its parts of the segments;
 * the host multiplies the parts of a segment across the cuts in rank order with the routine the
 * device uses, then scans and closes once.  The results are within rounding of a single handle's,
 * not its bytes.  (Chains of more than one handle are fast mode only.) */
int nghmm_chain_ibd_moments(nghmm_t** hs, int n_handles, int what, uint64_t n_regions,
                            const uint64_t* region_begin, const uint64_t* region_end,
                            nghmm_moment_region* regions);

/* ---- expected IBD above a minimum tract length ----
 * Per individual, region and threshold L_k the expected number of IBD tracts of length >= L_k
 * that begin in the region and the expected total length of those tracts, exactly, at the
 * handle's CURRENT parameters and emissions.  Tracts and lengths are nghmm_path_stats's: runs of
 * z = 1 cut at chromosome starts; in Mb the distance from a tract's first site to its last, so a
 * one-site tract is 0 Mb.  Notation of nghmm_ibd_expect (m_s, xi_s, r_s, pi_s, start_s,
 * chromosome starts, d_s).  Given the data the path is a Markov chain, so with
 *   sigma_s = start_s (xi_s(0, 1), or pi_s(1) at a chromosome start)
 *   rho_s   = r_s(1, 1) = m_s(1, 1) / (m_s(1, 0) + m_s(1, 1)), 0 for 0/0 and at a chromosome
 *             start; the step into s is BLOCKED iff rho_s == 0
 *   W(a, b) = prod_{s = a+1..b} rho_s, W(a, a) = 1
 * a tract begins at a and covers a..b with probability sigma_a W(a, b), and the run goes on beyond
 * b for M_b further sites, D_b further Mb in expectation:
 *   M_s = rho_{s+1} (1 + M_{s+1}),  D_s = rho_{s+1} (d_{s+1} + D_{s+1}),  0 at the last site; a
 *   blocked step gives 0, never inf * 0.
 * K thresholds, 1 <= K <= 8, strictly increasing.  In sites (default) len(a, b) = b - a + 1,
 * rem_b = M_b and the thresholds are integers >= 1; with NGHMM_BYLENGTH_MB len(a, b) = cum_b -
 * cum_a, rem_b = D_b and the thresholds are finite and >= 0, where cum_s = 0 at a chromosome start
 * and cum_{s-1} + d_s elsewhere (formed on the host in double, in site order).  b_k(a) is the
 * smallest b >= a in a's chromosome with len(a, b) >= L_k; if there is none, (a, k) contributes
 * nothing.  Then
 *   tracts_k(a) = sigma_a W(a, b_k(a)),  length_k(a) = tracts_k(a) (len(a, b_k(a)) + rem_{b_k(a)})
 * and the record [i][region][k] is the sum of the terms over the start sites a of the region
 * (nghmm_ibd_summary's regions): a tract belongs to the region in which it BEGINS, with its whole
 * length, even past the region's end; regions that partition the data add up to the whole.  Over
 * all sites tracts = E[number of tracts of length >= L_k | y] and length = E[their total length |
 * y].  With L = 1 site tracts is nghmm_ibd_expect's starts and, over whole chromosomes, length its
 * ibd; with L = 0 Mb length is its ibd_mb.  Both fields are non-increasing in k, length >= L_k
 * tracts, and differences of successive thresholds are the length classes [L_k, L_{k+1}).  A state
 * the data exclude gives exact zeros; nothing is NaN or inf.
 *
 * NGHMM_ERR_ARG with a message: n_lengths of 0 or above 8; thresholds that are not strictly
 * increasing, not finite, negative, or (in sites) not integers >= 1; an unknown bit in what; a
 * handle without data; NULL arguments and region faults as nghmm_ibd_expect reports them.
 *
 * Orders (no float atomics; the same arguments give the same bits on every call, and a region's
 * record does not depend on which other regions are asked for).  W(a, b) is formed as
 * n_b == n_a ? exp(Q_b - Q_a) : 0 from the prefix Q_s = sum of ln rho, which restarts from 0 at
 * every blocked step (a chromosome start is one), and the count n_s of blocked steps at or in
 * front of s; ln rho comes from the small side as in nghmm_ibd_expect.  Fast mode, in the layout
 * of nghmm_fast_layout (a lane-chunk is T consecutive sites): within a lane-chunk Q is added in
 * site order from the value that enters it; that value is the sum of the lane-chunks in front of
 * it back to the last blocked step, where a lane-chunk's own sum is added from its last site to
 * its first, the 64 lane-chunks of a wave in a Hillis-Steele tree (steps 1, 2, .., 32) and the
 * waves in site order.  M and D: per lane-chunk the affine map x -> A x + B of its sites composed
 * from its last site to its first, the maps of a wave composed in the same tree right to left, the
 * waves right to left; inside a lane-chunk the recursion itself from the chunk-end value.  All
 * coefficients lie in [0, 1] (B in units of sites or Mb): nothing cancels.  A region's sum: pieces
 * at the lane-chunk edges, each added from its last site to its first, the pieces in site order,
 * as nghmm_ibd_expect.  Exact mode: one lane per individual in log space, Q in site order, a
 * region's terms added to 0 from its last site to its first.
 *
 * Accuracy of W: Q_b - Q_a is a difference of prefix sums, so the exponent carries an absolute
 * error of about 2^-53 max|Q| between two restarts.  |Q| grows only through stretches that are
 * neither blocked nor confidently IBD; at 10^6 sites a long confidently non-IBD stretch can push
 * it to ~10^6, a relative error of ~1e-10 in a term (and such terms are themselves ~ exp(-|Q|)).
 * nghmm_debug_bylength_qmax (nghmm_debug.h) reports the largest |Q| of the last call.
 *
 * Self-contained and read-only exactly like nghmm_ibd_expect: it refreshes stale emissions itself
 * and leaves parameters, posteriors, the Viterbi path, checkpoints and an M-step planned in advance
 * untouched; an EM iteration after the call gives the bits it would have given without it.  Device
 * scratch, kept by the handle and allocated on first use (NGHMM_ERR_NOMEM when it cannot be had):
 * 36 bytes per cell (sigma, Q, n, M, D) in a buffer of its own; 64 bytes per (individual,
 * lane-chunk); 4 n_lengths + 8 bytes per site for b_k and cum; 16 n_lengths per (individual,
 * piece) and per (individual, region).   */
enum { NGHMM_BYLENGTH_MB = 1 };
typedef struct nghmm_bylength_stat {  /* 16 bytes; one per (individual, region, threshold) */
  double tracts;  /* expected number of tracts of length >= L_k that begin in the region */
  double length;  /* expected total length of those tracts, in sites or Mb */
} nghmm_bylength_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_bylength_stat) == 16, "record size");
#endif
/* stats [I][n_regions][n_lengths] (host) */
int nghmm_ibd_by_length(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length,
                        uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end,
                        nghmm_bylength_stat* stats);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices.  M and D travel right to left across the cuts; a shard receives from its right
 * neighbour Q, n and rem of as many of the neighbour's first sites as its own windows reach (Q
 * and n start afresh in every shard, and a window across the cut is the product of its two
 * parts).  A threshold whose window from a shard's last sites reaches past the NEXT shard is
 * NGHMM_ERR_ARG with a message.  A region across a cut is one region, its parts added on the host
 * in rank order.  The results are within rounding of a single handle's, not its bytes.  (Chains
 * of more than one handle are fast mode only.) */
int nghmm_chain_ibd_by_length(nghmm_t** hs, int n_handles, int what, uint32_t n_lengths,
                              const double* min_length, uint64_t n_regions, const uint64_t* region_begin,
                              const uint64_t* region_end, nghmm_bylength_stat* stats);

/* ---- the longest IBD tract ----
 * Per individual, region and threshold L_k the probability that SOME IBD run of the region is of
 * length >= L_k, and that none is, exactly, at the handle's CURRENT indF, alpha and freq.  (The
 * tracts of nghmm_ibd_by_length bound p_any from above only -- Markov's inequality.)  Notation of
 * nghmm_ibd_expect / nghmm_ibd_by_length: pi_s(l) the posterior of state l at site s; r_s(k, l) =
 * P(z_s = l | z_{s-1} = k, y), each entry from its own product, 0 for 0/0; rho_s = r_s(1, 1), 0 at a
 * chromosome start, and the step into s is BLOCKED iff rho_s == 0.  Chromosome starts, d_s, cum_s,
 * len(a, b), the thresholds (1 <= K <= 8, strictly increasing; whole numbers of sites >= 1, or with
 * NGHMM_LONGEST_MB finite and >= 0 Mb) and the table b_k(a) are nghmm_ibd_by_length's.
 *
 * For a region [lo, hi) (nghmm_ibd_summary's regions) a RUN is a maximal stretch of z = 1 INSIDE
 * the region, cut at chromosome starts and at the region's two edges; over whole chromosomes it is
 * a tract of nghmm_path_stats.  Per threshold, over the sites of the region inside one chromosome,
 * with N the mass with z_s = 0 and no hit yet, V the mass inside a run that has not reached L_k
 * and Hit the absorbed mass:
 *   s = lo:  N = pi_lo(0);  tau_lo = pi_lo(1);  V = tau_lo - G_lo
 *   s > lo:  tau_s = N r_s(0, 1);  N' = N r_s(0, 0) + V r_s(1, 0);  V' = V rho_s + tau_s - G_s (>= 0)
 *   G_s = sum over a >= lo with b_k(a) = s of tau_a W(a, s),  W(a, s) = prod_{t = a+1..s} rho_t
 *   Hit += G_s;   p_any = Hit(hi - 1),   p_none = N(hi - 1) + V(hi - 1)  (its own sum, not 1 - p_any)
 * Chromosomes are independent given the parameters: a region's parts per chromosome are combined
 * in site order, any = any_prev + none_prev any_part, none = none_prev none_part.  pi is formed at
 * a chromosome's first site from q e beta normalised and propagated from there, pi_s(l) =
 * pi_{s-1}(0) r_s(0, l) + pi_{s-1}(1) r_s(1, l), the same operations wherever the sites are cut.
 * At L = 1 site (and at 0 Mb) a one-site region gives p_any = pi_s(1).  p_any is non-increasing
 * in k.  A state the data exclude gives exact zeros; nothing is NaN; a threshold no chromosome
 * reaches gives p_any = 0 exactly.
 *
 * Orders (no float atomics; the same arguments give the same bits on every call, and a region's
 * record does not depend on which other regions are asked for).  b_k is non-decreasing inside a
 * chromosome, so a lane keeps a pointer to the oldest unresolved start and a ring of (tau_a, Q_a)
 * of the starts since; the starts that resolve at s are added to G_s oldest first; a blocked step
 * discards the ring.  W(a, s) = exp(Q_s - Q_a) with Q the running sum of ln rho (from the small
 * side, as nghmm_ibd_expect), restarted from 0 at every blocked step and at a part's first site:
 * nghmm_ibd_by_length's rule and accuracy, an absolute error of about 2^-53 max|Q| in the
 * exponent.  p_none is accurate to an ABSOLUTE error of that size, not a relative one.  Both modes
 * walk one lane per (individual, chromosome part of the handle): right to left beta and the steps
 * r_s, left to right the recursion, a threshold's operations not depending on the other thresholds
 * (they may share a lane or have lanes of their own: the same bits); fast mode
 * in linear space with power-of-two rescaling of beta, exact mode with beta and r_s in log space
 * through detmath.h.  The parts of a region are combined on the host.
 *
 * NGHMM_ERR_ARG with a message as nghmm_ibd_by_length.  Self-contained and read-only exactly like
 * nghmm_freq_info: an EM iteration after the call gives the bits it would have given without it.
 * Device scratch, kept by the handle and allocated on first use (NGHMM_ERR_NOMEM when it cannot be
 * had): 40 bytes per cell (the four steps and ln rho); per individual 16 bytes times the sum over
 * the handle's chromosome parts and the thresholds of the longest window b_k(a) - a + 1 of that
 * threshold in that part; 4 n_lengths bytes per site of the whole data for b_k; 16 n_lengths per
 * (individual, region part).   */
enum { NGHMM_LONGEST_MB = 1 };
typedef struct nghmm_longest_stat {  /* 16 bytes; one per (individual, region, threshold) */
  double p_any;   /* P(some run of the region has length >= L_k | y) */
  double p_none;  /* P(no run has), from its own sum */
} nghmm_longest_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_longest_stat) == 16, "record size");
#endif
/* stats [I][n_regions][n_lengths] (host) */
int nghmm_ibd_longest(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length,
                      uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end,
                      nghmm_longest_stat* stats);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices.  beta crosses the cuts right to left, the forward lane state left to right through the
 * host (pi, Q and per threshold N, V, Hit, the pointer and the ring's live entries); a shard goes
 * on with the single handle's own operations, so the chain returns the single handle's BYTES, and
 * no threshold is refused for reaching past a shard.  (Chains of more than one handle are fast
 * mode only.) */
int nghmm_chain_ibd_longest(nghmm_t** hs, int n_handles, int what, uint32_t n_lengths,
                            const double* min_length, uint64_t n_regions, const uint64_t* region_begin,
                            const uint64_t* region_end, nghmm_longest_stat* stats);

/* ---- the number of long IBD tracts ----
 * Per individual, region and threshold L_k the DISTRIBUTION of C_k, the number of IBD runs of the
 * region whose length is >= L_k (NROH above L_k), exactly, at the handle's CURRENT indF, alpha and
 * freq.  Everything is nghmm_ibd_longest's unless stated: runs (maximal stretches of z = 1 inside
 * the region, cut at chromosome starts and at the region's two edges), pi_s, r_s(k, l), rho_s and
 * blocked steps, Q and W(a, s) = exp(Q_s - Q_a), the thresholds (1 <= K <= 8, in sites or with
 * NGHMM_COUNT_MB in Mb) and the table b_k(a), regions and their parts per chromosome.
 *
 * n_counts = M, 1 <= M <= 16.  Per (individual, region, threshold) the output is M + 1 doubles:
 * prob[c] = P(C_k = c | y) for c < M and prob[M] = P(C_k >= M | y), each from its own sum, never as
 * 1 - the rest.  Masses per threshold, over the sites of the region inside one chromosome, for
 * c = 0 .. M - 1:  N_c: z_s = 0, c long runs so far;  V_c: inside a run that has not reached L_k,
 * c long runs before it;  R_c (c >= 1): inside a run that has reached L_k, itself counted among the
 * c;  Top: the absorbed mass with count >= M.
 *   s = lo:  N_0 = pi_lo(0);  tau_0 = pi_lo(1);  every other mass 0
 *   s > lo:  tau_c = N_c r_s(0, 1)
 *            N_c'  = N_c r_s(0, 0) + V_c r_s(1, 0) [+ R_c r_s(1, 0) for c >= 1]
 *            G_c(s) = sum over starts a >= lo with b_k(a) = s of tau_{a,c} W(a, s)   (oldest first)
 *            V_c'  = max(V_c rho_s + tau_c - G_c(s), 0)
 *            R_c'  = R_c rho_s + G_{c-1}(s)            (1 <= c < M)
 *            Top  += G_{M-1}(s)
 *   end:     prob[c] = N_c + V_c + R_c  (c < M),   prob[M] = Top
 * A blocked step discards the ring; a ring entry holds (Q_a, tau_{a,0..M-1}).  The parts of a region
 * in different chromosomes are independent: the host combines them in site order by a convolution
 * cut off at M, j ascending, every output from its own sum, the top level absorbing
 * (top = top_prev + sum over a < M of prev[a] P(part >= M - a)).  With M = 1 the operations are
 * nghmm_ibd_longest's: prob[0] is its p_none and prob[1] its p_any.  prob[..][c] for c < M does not
 * depend on M beyond rounding.  A state the data exclude gives exact zeros, and where pi_lo(1) is
 * exactly 0, N_0 = 1 exactly (the propagated pi_lo(0) carries the roundings of its sum); nothing is
 * NaN; a part that no window of the threshold fits into (b_k of its first site is none or beyond
 * it) has no long run: prob[0] = 1 exactly and zeros elsewhere, so a threshold no chromosome reaches
 * gives exactly that.
 *
 * Orders: no float atomics; the same arguments give the same bits on every call, and a region's
 * record does not depend on which other regions are asked for.  One lane per (individual,
 * chromosome part of the handle, threshold) in both modes; the backward walk is
 * nghmm_ibd_longest's.
 *
 * NGHMM_ERR_ARG with a message under nghmm_ibd_longest's conditions, and for n_counts outside
 * 1..16.  Self-contained and read-only exactly like nghmm_ibd_longest: an EM iteration after the
 * call gives the bits it would have given without it.  Device scratch: nghmm_ibd_longest's, shared
 * with it (NGHMM_ERR_NOMEM when it cannot be had) -- 40 bytes per cell; per individual
 * 8 (n_counts + 1) bytes instead of 16 times the sum over the handle's chromosome parts and the
 * thresholds of the longest window b_k(a) - a + 1 of that threshold in that part; 4 n_lengths bytes
 * per site for b_k; 8 n_lengths (n_counts + 1) per (individual, region part).  One handle only:
 * there is no call over a chain of site shards yet.   */
enum { NGHMM_COUNT_MB = 1 };
/* prob [I][n_regions][n_lengths][n_counts + 1] (host) */
int nghmm_ibd_count(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, uint32_t n_counts,
                    uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end, double* prob);

/* ---- mean and variance of IBD in long tracts ----
 * Per individual, region and threshold L_k the posterior mean and covariance matrix of
 *   A_k = the total length of the region's IBD runs whose length is >= L_k   (F_ROH above L_k)
 *   C_k = their number                                                         (NROH above L_k)
 * exactly, at the handle's CURRENT indF, alpha and freq.  Everything is nghmm_ibd_count's unless
 * stated: runs (maximal stretches of z = 1 inside the region, cut at chromosome starts and at the
 * region's two edges), regions and their parts per chromosome, pi_s, r_s(k, l), rho_s and blocked
 * steps, Q and W(a, s) = exp(Q_s - Q_a), the thresholds (1 <= K <= 8, in sites or with
 * NGHMM_LONG_MOMENTS_MB in Mb) and the table b_k(a).  The length of a run a..b is len(a, b) =
 * b - a + 1 in sites and cum_b - cum_a in Mb, as nghmm_ibd_by_length measures it.
 *
 * Per threshold over the sites of one part (one chromosome's share of a region, first site lo)
 * every mass class X in {N, V, R} is a vector of six doubles: the mass and the moments of
 * (A - oA, C - oC) on it in the order (1, A, C, A^2, AC, C^2); (oA, oC) is the lane's offset pair,
 * (0, 0) at lo.  N: z_s = 0;  V: inside a run that has not reached L_k;  R: inside a run that has
 * reached L_k and is counted.  Sh(m; l, c), the moments of (A + l, C + c):
 *   m0' = m0;  mA' = mA + l m0;  mC' = mC + c m0;  mAA' = mAA + 2 l mA + l^2 m0;
 *   mAC' = mAC + l mC + c mA + l c m0;  mCC' = mCC + 2 c mC + c^2 m0
 *   s = lo:  N = (pi_lo(0), 0, ..) (mass 1 exactly where pi_lo(1) == 0, as nghmm_ibd_count);
 *            tau = (pi_lo(1), 0, ..);  V = R = 0
 *   s > lo:  tau = N r_s(0, 1);   N' = N r_s(0, 0) + V r_s(1, 0) + R r_s(1, 0)
 *   for each start a with b_k(a) = s, oldest first:
 *            g_a = Sh(tau_a W(a, s); oA_a - oA, oC_a - oC)   (the entry at the lane's current offsets)
 *            G += g_a;   Gs += Sh(g_a; len(a, s), 1)
 *   V' = V rho_s + tau - G component-wise; the whole vector is 0 if its mass is <= 0
 *   R' = Sh(R rho_s; delta_s, 0) + Gs,   delta_s = 1 in sites and d_s in Mb
 * A ring entry holds (Q_a, oA_a, oC_a, tau_a[6]); a blocked step discards the ring.  After the
 * update at every site with (s - lo) % 8 == 7 the vectors are re-centred: with t = (N + V) + R,
 * dA = t_A / t_0 and dC = t_C / t_0:  X <- Sh(X; -dA, -dC) for N, V, R;  oA += dA;  oC += dC.  (The
 * raw moments would lose E[A]^2 / Var(A) digits when they are closed; the centred ones do not.)
 * At the end of the part, with t as above, m0 = t_0, muA = t_A / m0 and muC = t_C / m0:
 *   mean_a = oA + muA;   mean_t = oC + muC;   var_a = max(t_AA / m0 - muA^2, 0);
 *   cov_at = t_AC / m0 - muA muC;   var_t = max(t_CC / m0 - muC^2, 0)
 * A part that no window of the threshold fits into gives five exact zeros.  Chromosomes are
 * independent given the parameters: the host adds a region's parts in site order, all five fields.
 * Everything is conditional on indF, alpha and the allele frequencies, as nghmm_ibd_moments.  At
 * L = 1 site (and 0 Mb) over whole chromosomes the record is nghmm_ibd_moments'; over whole
 * chromosomes mean_t is nghmm_ibd_by_length's tracts and mean_a its length; mean_t and var_t are
 * the mean and variance of nghmm_ibd_count's distribution.  A state the data exclude gives exact
 * zeros; nothing is ever NaN.
 *
 * Orders: no float atomics; the same arguments give the same bits on every call, and a record does
 * not depend on which other regions or thresholds are asked for.  One lane per (individual,
 * chromosome part of the handle, threshold) in both modes; the backward walk is nghmm_ibd_longest's.
 *
 * NGHMM_ERR_ARG with a message under nghmm_ibd_count's conditions.  Self-contained and read-only
 * exactly like it: an EM iteration after the call gives the bits it would have given without it.
 * Device scratch: nghmm_ibd_longest's, shared with it (NGHMM_ERR_NOMEM when it cannot be had) --
 * 40 bytes per cell; per individual 72 bytes times the sum over the handle's chromosome parts and
 * the thresholds of the longest window b_k(a) - a + 1 of that threshold in that part;
 * 4 n_lengths + 16 bytes per site; 40 n_lengths per (individual, region part).  One handle only:
 * there is no call over a chain of site shards.   */
enum { NGHMM_LONG_MOMENTS_MB = 1 };
typedef struct nghmm_long_moment_stat {  /* 40 bytes; one per (individual, region, threshold) */
  double mean_a;  /* E[A_k | y]: expected sites (or Mb) of the region inside runs of length >= L_k */
  double mean_t;  /* E[C_k | y]: expected number of such runs */
  double var_a;   /* Var(A_k | y), >= 0 */
  double cov_at;  /* Cov(A_k, C_k | y) */
  double var_t;   /* Var(C_k | y), >= 0 */
} nghmm_long_moment_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_long_moment_stat) == 40, "record size");
#endif
/* stats [I][n_regions][n_lengths] (host) */
int nghmm_ibd_long_moments(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, uint64_t n_regions,
                           const uint64_t* region_begin, const uint64_t* region_end, nghmm_long_moment_stat* stats);

/* ---- per-site posterior of lying in a long IBD tract ----
 * Per individual, site and threshold L_k the probability P_k(s) that site s lies in an IBD tract
 * of length >= L_k, exactly, at the handle's CURRENT indF, alpha and freq: the track "this site
 * lies in a ROH above 1 Mb".  Everything is nghmm_ibd_by_length's unless stated: tracts (runs of
 * z = 1 cut at chromosome starts), len(a, b), cum_s, d_s, sigma_a, rho_s, blocked steps, W(a, b),
 * the thresholds (1 <= K <= 8, strictly increasing; whole numbers of sites >= 1, or with
 * NGHMM_LONG_MB finite and >= 0 Mb) and the table b_k(a).  pi_s = P(z_s = 1 | y), unsnapped.
 * Per threshold k and site s, with c0 the first site of s's chromosome:
 *   lo_k(s) = the largest a <= s in s's chromosome with len(a, s) >= L_k, or none; non-decreasing
 *             in s inside a chromosome, a host table like b_k (one two-pointer pass, the
 *             comparison that forms b_k, so that a <= lo_k(s) iff b_k(a) <= s)
 *   T_k(a)  = sigma_a W(a, b_k(a)), 0 where b_k(a) is none: nghmm_ibd_by_length's tracts term
 *   A_k(s)  = pi_lo W(lo, s) with lo = lo_k(s), 0 if there is none: the paths that are IBD on the
 *             whole minimal window that ends at s
 *   B_k(s)  = the sum of T_k(a) over a = lo + 1 .. s (a = c0 .. s if lo is none): the runs that
 *             begin too late to be long at s but get there
 *   P_k(s)  = A_k(s) + B_k(s)
 * 0 <= P_k(s) <= pi_s; P_k is non-increasing in k; at L = 1 site and at 0 Mb P = pi, bit for bit;
 * a state the data exclude and a threshold no chromosome reaches give exactly 0; nothing is NaN.
 * P_k(s) - T_k(s) = P(s - 1 and s lie in the same tract of length >= L_k | y).
 *
 * Outputs, each optional (NULL skips it; not all three); no output's bits depend on which others
 * are asked for, or on which other regions are:
 *   post [K][I][S_tot]  P_k, each plane in the layout of nghmm_get_posteriors' IBD state
 *   site_stats [S_tot][K]  sum = sum_i P_k(s), the individuals added in index order; count = the
 *             individuals with P_k(s) >= threshold (in [0, 1], as nghmm_ibd_summary's)
 *   region_stats [I][n_regions][K], nghmm_ibd_summary's regions:
 *             sites = sum over the region's sites of P_k(s)
 *             mb    = sum over its sites that are no chromosome start of d_s max(P_k(s) - T_k(s), 0)
 *             Every site contributes its own term (not the tract's whole length to the region it
 *             begins in), so regions that partition the data add up; both fields are filled
 *             whichever unit the thresholds are in.  Over whole chromosomes sites is
 *             nghmm_ibd_by_length's length with thresholds in sites and mb its length with
 *             thresholds in Mb; at L = 1 site sites is nghmm_ibd_expect's ibd and at 0 Mb mb its
 *             ibd_mb, on any region.
 *
 * Orders (no float atomics; the same arguments give the same bits on every call).  The cells
 * sigma_s, Q_s, n_s are nghmm_ibd_by_length's, in its orders, and pi_s = xi_s(0, 1) + xi_s(1, 1)
 * comes from the same walk.  T_k(a) = sigma_a (n_b == n_a ? exp(Q_b - Q_a) : 0) at b = b_k(a).  A
 * term T_k(a) with a blocked step in (a, s] is exactly 0 when its window reaches beyond s, so
 * B_k is a difference of the prefix U of T_k that restarts at every blocked step (where Q does):
 *   n_lo == n_s:  P = pi_lo exp(Q_s - Q_lo) + max(U_s - U_lo, 0);   otherwise (and without lo)  P = U_s;
 *   then P = min(P, pi_s), so that 0 <= P <= pi and P = 0 where pi = 0 hold exactly.
 * U in fast mode (a lane-chunk is T consecutive sites of nghmm_fast_layout): within a lane-chunk
 * T_k is added in site order from 0, restarting at a blocked step; what enters a lane-chunk is
 * the sum of the lane-chunks in front of it back to the last blocked step, the 64 lane-chunks of
 * a wave in a Hillis-Steele tree (steps 1, 2, .., 32) and the waves in site order; U_s = (what
 * enters, if the lane-chunk has no blocked step up to s) + (the lane-chunk's own sum).  A
 * region's sums: pieces at the lane-chunk edges, each added from its last site to its first, the
 * pieces in site order, as nghmm_ibd_by_length.  Exact mode: one lane per individual, U in site
 * order, a region's terms added to 0 from its last site to its first; exp through detmath.h.
 *
 * Accuracy: W as nghmm_ibd_by_length (2^-53 max|Q| in the exponent); the difference U_s - U_lo
 * carries an absolute error of 2^-53 U, U being the expected number of long-tract starts since
 * the last blocked step -- below W's own error.
 *
 * NGHMM_ERR_ARG with a message as nghmm_ibd_by_length, and for a threshold outside [0, 1] (NaN
 * included) and for three NULL outputs; region_stats, region_begin and region_end are NULL iff
 * n_regions == 0.  Self-contained and read-only exactly like nghmm_ibd_by_length: it refreshes stale
 * emissions itself, and an EM iteration after the call gives the bits it would have given without
 * it.  Device scratch, kept by the handle and allocated on first use (NGHMM_ERR_NOMEM when it
 * cannot be had): nghmm_ibd_by_length's 36 bytes per cell (sigma, Q, n; pi in the place of D, T_k
 * in the place of M) and 40 bytes per cell more (a packed 32-byte record pi, Q, U, n that the
 * gather at lo_k(s) reads, and P_k), 8 more when post is asked for: one threshold is worked at a
 * time, so nothing per cell grows with K; 84 bytes per (individual, lane-chunk); 8 n_lengths bytes
 * per site for b_k and lo_k; 16 per (individual, piece), 16 n_lengths per (individual, region) and
 * per site with site records.   */
enum { NGHMM_LONG_MB = 1 };
typedef struct nghmm_long_region_stat {  /* 16 bytes; one per (individual, region, threshold) */
  double sites;  /* expected number of the region's sites in tracts of length >= L_k */
  double mb;     /* expected Mb of the region inside such tracts */
} nghmm_long_region_stat;
typedef struct nghmm_long_site_stat {  /* 16 bytes; one per (site, threshold) */
  double sum;      /* sum over the individuals of P_k(s) */
  uint64_t count;  /* individuals with P_k(s) >= threshold */
} nghmm_long_site_stat;
#ifdef __cplusplus
static_assert(sizeof(nghmm_long_region_stat) == 16 && sizeof(nghmm_long_site_stat) == 16, "record size");
#endif
int nghmm_ibd_long(nghmm_t* h, int what, uint32_t n_lengths, const double* min_length, double threshold,
                   uint64_t n_regions, const uint64_t* region_begin, const uint64_t* region_end,
                   nghmm_long_region_stat* region_stats, nghmm_long_site_stat* site_stats, double* post);
/* include/nghmm_chain_long.h declares the same call over a chain of site shards. */

/* ---- pairwise IBD sharing between individuals ----
 * How much IBD two individuals share over the sites [site_begin, site_end): three host matrices
 * [I][I], full and symmetric, reduced on the matrix cores from the decoded path and the
 * posteriors where the run left them.  Site indices are handle-local for one handle and global
 * for a chain; site_begin < site_end <= S, else NGHMM_ERR_ARG.
 *   vit_both[i][j]   the sites s of the range with path[i][s] == path[j][s] == 1, path the last
 *                    nghmm_viterbi / nghmm_chain_viterbi decode of the loaded data
 *                    (NGHMM_ERR_ARG if there was none since the load)
 *   post_both[i][j]  the sites with marg_prob[i][s][1] >= threshold and
 *                    marg_prob[j][s][1] >= threshold
 *   post_prod[i][j]  the sum over the sites of marg_prob[i][s][1] * marg_prob[j][s][1]: the
 *                    expected number of sites at which both are IBD (given the data the
 *                    individuals are independent in this model)
 * The diagonal is included: vit_both[i][i] and post_both[i][i] are i's own IBD sites,
 * post_prod[i][i] is the sum of its squared posteriors.
 *
 * `what` is a bit mask of the sources: NGHMM_SHARING_VITERBI gives vit_both,
 * NGHMM_SHARING_POSTERIOR gives post_both, post_prod or both.  The pointers of a source that is
 * not asked for must be NULL; of a source that is, at least one is not NULL (a NULL one is not
 * computed).  threshold in (0, 1], else -- NaN included -- NGHMM_ERR_ARG; it is only looked at
 * when post_both is asked for.  NGHMM_ERR_ARG also for a handle without data, what == 0 or an
 * unknown bit, and a NULL mismatch.
 *
 * No float atomics.  post_prod: the range is cut into K-splits -- first = site_begin rounded down
 * to a multiple of 64, n = min(ceil((site_end - first) / 1024), max(1, min(1024, 2^28 / (8 I^2)))),
 * len = ceil((site_end - first) / n) rounded up to a multiple of 64, split k = the sites of the
 * range in [first + k len, first + (k + 1) len) --, a function of (I, site_begin, site_end) alone.
 * Within a split v_mfma_f64_16x16x4_f64 accumulates four sites a step, the steps in ascending
 * site order from the split's first site; the splits are added in site order, the first one's
 * value first.  So the same call on the same handle gives the same bits every time, whatever
 * `what` is and whichever other outputs are asked for.  The order of the four products inside one
 * instruction is the hardware's: the value is defined to a bound -- within (n_sites + 1) 2^-53
 * relative of the exact sum of its non-negative terms --, not to a bit.  The counts are exact
 * (int32 within a split, which holds fewer than 2^31 sites, uint64 across splits).
 * 
 *
 * Read-only, like nghmm_ibd_summary: an EM iteration after the call gives the bits it would have
 * given without it.  Device scratch (kept by the handle): the splits' partial matrices, at most
 * max(2^28, 8 I^2) bytes, one result matrix, and for post_both one byte per cell of the range
 * (NGHMM_ERR_NOMEM when it cannot be had).
 *
 * Groups of individual shards (nghmm_group_*) are out of scope, as for the summary. */
enum { NGHMM_SHARING_VITERBI = 1, NGHMM_SHARING_POSTERIOR = 2 };
int nghmm_ibd_sharing(nghmm_t* h, int what, double threshold, uint64_t site_begin, uint64_t site_end,
                      uint64_t* vit_both, uint64_t* post_both, double* post_prod);
/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): every shard the
 * range touches computes the matrices of its part of the range on its own device exactly as one
 * handle would (a shard outside the range is not launched), and the host adds the shards'
 * matrices in rank order, the first one's value first: the counts exactly, the doubles in that
 * fixed order. */
int nghmm_chain_ibd_sharing(nghmm_t** hs, int n, int what, double threshold, uint64_t site_begin,
                            uint64_t site_end, uint64_t* vit_both, uint64_t* post_both,
                            double* post_prod);

/* ---- multi-GPU (individuals sharded over ranks) ----
 * The allele-frequency step needs every individual of a site.  A rank owns the
 * individuals [ind_begin, ind_begin + n_ind) of n_ind_total for all sites, and
 * the sites [site_begin, site_begin + n_sites_own) for the frequency step.
 * The host moves posteriors between ranks with an all-to-all and frequencies with
 * an all-gather (RCCL through torch.distributed or rccl.h); these calls take raw
 * DEVICE pointers to the exchange buffers. */
int nghmm_shard_config(nghmm_t* h, uint64_t n_ind_total, uint64_t ind_begin, uint64_t site_begin,
                       uint64_t n_sites_own);
/* static site-shard copy of the GLs of ALL individuals: [n_sites_own][n_ind_total][3] (host) */
int nghmm_load_gl_site_shard(nghmm_t* h, const double* gl_site_shard);
/* same, from a device buffer */
int nghmm_load_gl_site_shard_dev(nghmm_t* h, const double* d_gl_site_shard);
/* packed handles: the own individuals' genotype codes of the sites [site_lo, site_hi) as one
 * byte per cell (0, 1, 2, 3 = missing), d_out[(s - site_lo) * n_ind + i] (device) -- what the
 * host exchanges once to build the site shards -- and the static site-shard copy from such
 * bytes, [n_sites_own][n_ind_total] (device) */
int nghmm_get_geno_codes_dev(nghmm_t* h, uint64_t site_lo, uint64_t site_hi, uint8_t* d_out);
int nghmm_load_geno_site_shard_dev(nghmm_t* h, const uint8_t* d_codes_bytes);
/* pack posteriors of the own individuals for destination rank r's site range:
 * d_out[(s - site_lo) * n_ind + i], s in [site_lo, site_hi); with [0, n_sites) the whole
 * site-major matrix = the send buffer of all equal contiguous ranges at once */
int nghmm_pack_posteriors_dev(nghmm_t* h, uint64_t site_lo, uint64_t site_hi, double* d_out);
/* d_marg_sites: [n_sites_own][n_ind_total] posteriors of the own site range (device);
 * runs est_maf on them, writes d_freq_out[n_sites_own] (device) */
int nghmm_mstep_freq_sites_dev(nghmm_t* h, const double* d_marg_sites, double* d_freq_out);
/* install the gathered freq[S] (device pointer) and refresh the own emissions */
int nghmm_set_freq_dev(nghmm_t* h, const double* d_freq_all);

/* ---- one process, several GPUs: a GROUP of n handles ----
 * What EM.cpp:147-272 does for all individuals at once, split over n handles (one per GPU; or
 * several on one GPU): handle r owns the individuals [r I, (r+1) I) of n I for all sites --
 * create and load it with those -- and, after nghmm_group_setup, the sites [r S/n, (r+1) S/n)
 * of the allele-frequency step.  nghmm_group_iter_em = iter_EM for the whole cohort: per
 * handle, on its own host thread, the E-step and the indF/alpha M-step; the posteriors move
 * to their site owners by direct peer copies (every GPU pair of an MI355X node has its own
 * xGMI link: the n (n-1) copies are the all-to-all) under the remaining objective rounds;
 * est_maf per site range in global individual order; the frequencies go to everybody.  The
 * result does not depend on n (tests/test_gpu_sharded.py).  Equal I and S, S divisible by n,
 * NGHMM_MODE_FAST for n > 1; ind_lkl [n I] (host, may be NULL).  Between processes the same
 * steps run over RCCL (ngsf-hmm_amd/distributed.py). */
int nghmm_group_setup(nghmm_t** handles, int n);
int nghmm_group_iter_em(nghmm_t** handles, int n, int freq_est, int indF_fixed, int alpha_fixed,
                        double* ind_lkl, nghmm_mstep_stats* stats);
/* the allele-frequency step alone (nghmm_mstep_freq for the cohort), from the posteriors the
 * handles hold: all zero before the first E-step, which is `--freq e` */
int nghmm_group_mstep_freq(nghmm_t** handles, int n, int freq_est);

/* ---- multi-GPU, fast mode: shard the SITES instead ----
 * (what bench.py --gpus N and ngsf-hmm_amd/distributed.py use by default.)  A handle holds ALL
 * individuals for a contiguous range of sites -- created and loaded like a data set of its
 * own, with the true distance in front of its first site (+inf only at a chromosome start) --
 * and the ranges follow each other in rank order.  A run of sites is a product of 2x2
 * operators, so what the ranges owe each other is six doubles per individual and E-step, and
 * per objective point and round: forward / backward vectors, log-likelihoods and objective
 * values are then those of the whole chain, and every handle computes the same values and
 * takes the same L-BFGS-B steps for all individuals (shared/HMM.cpp:6-60 and EM.cpp:423-464
 * over all sites).  The allele-frequency step (EM.cpp:224-247) has every individual of a
 * handle's sites at hand: no posterior ever leaves the GPU (the individual shards above move
 * 8 bytes per site and individual per iteration, 8 GB at 1000 x 1M, over one xGMI link per GPU
 * pair).  Not for NGHMM_MODE_EXACT: its log-space recursion is one chain of roundings over all
 * sites.
 *
 * nghmm_site_shard_setup: send_dev / recv_dev are the caller's device buffers of
 * nghmm_site_shard_bytes(h) and world times that many bytes; `allgather(user, n)` must make
 * recv_dev = [rank][n bytes] of every handle's first n bytes of send_dev, ORDERED ON THE
 * HANDLE'S STREAM (nghmm_stream): the library has enqueued the writes of send_dev there before
 * the call and enqueues the reads of recv_dev after it; the function may block (a host-staged
 * exchange) or only enqueue (an RCCL all-gather on that stream).  It is called from inside
 * nghmm_estep / _lkl_batch / _mstep_indf / _estep_mstep / _iter_em, by every handle of the
 * chain the same number of times with the same n.  Non-zero return = failure (NGHMM_ERR_HIP).
 * world == 1 detaches.  Everything else (est_maf, emissions, posteriors, parameters, output
 * formatting) works on the handle's own sites as on any handle; nghmm_get_params' indF / alpha
 * are the cohort's and equal on all handles.
 *
 * Viterbi (shared/HMM.cpp:98-125) over the chain: nghmm_viterbi_shard_forward in rank order
 * (scores_in = NULL on the first handle, else the scores_out [I][2] of the handle before), then
 * nghmm_viterbi_shard_back in reverse order (state_after = NULL on the last handle, else the
 * state_before [I] of the handle after); path = [I][n_sites of the handle].  The same
 * operations in the same order per individual as nghmm_viterbi on one handle over all sites. */
typedef int (*nghmm_allgather_fn)(void* user, uint64_t n_bytes);
uint64_t nghmm_site_shard_bytes(nghmm_t* h);
int nghmm_site_shard_setup(nghmm_t* h, int rank, int world, void* send_dev, void* recv_dev,
                           uint64_t bytes_per_rank, nghmm_allgather_fn allgather, void* user);
int nghmm_viterbi_shard_forward(nghmm_t* h, const double* scores_in, double* scores_out);
int nghmm_viterbi_shard_back(nghmm_t* h, const uint8_t* state_after, uint8_t* state_before,
                             uint8_t* path);

/* ---- one process, several GPUs, fast mode: a CHAIN of site shards ----
 * n handles of one process (one per GPU, or several on one), handle r holding all individuals
 * for the r-th site range: nghmm_chain_setup installs the all-gather of nghmm_site_shard_setup
 * among them (direct device-to-device copies between the handles' buffers -- over the GPU
 * pair's xGMI link where the devices differ -- between two barriers of the handles' host
 * threads) and owns the buffers; nghmm_chain_iter_em = iter_EM (EM.cpp:139-289) for the whole
 * chain, every handle on a host thread of its own; ind_lkl [I] (host, may be NULL).
 * nghmm_chain_mstep_freq: the allele-frequency step alone (`--freq e`), every handle on its
 * own sites.  nghmm_chain_viterbi: path [I][all sites] (host).  n == 1 is the plain handle.
 * This is what the C++ host's --n_gpus N uses; destroying a member dissolves the chain. */
int nghmm_chain_setup(nghmm_t** handles, int n);
int nghmm_chain_iter_em(nghmm_t** handles, int n, int freq_est, int indF_fixed, int alpha_fixed,
                        double* ind_lkl, nghmm_mstep_stats* stats);
int nghmm_chain_mstep_freq(nghmm_t** handles, int n, int freq_est);
int nghmm_chain_viterbi(nghmm_t** handles, int n, uint8_t* path);

/* Page-locked host memory for buffers the library copies results into (nghmm_get_*,
 * nghmm_format_posteriors, nghmm_geno_posteriors, nghmm_viterbi ...): copies from the device
 * into such a buffer run at the PCIe rate instead of through a staging buffer.  Any host memory
 * works; this is for hosts that move gigabytes (the .ibd / .geno writers).  NULL when it cannot
 * be had. */
void* nghmm_alloc_host(uint64_t bytes);
void nghmm_free_host(void* p);

/* Device pointer + stream access for host-side plumbing (torch tensors, events). */
void* nghmm_stream(nghmm_t* h);
int nghmm_synchronize(nghmm_t* h);
/* Measurement and debugging entry points (switches of a handle, kernel timing, counters of the
 * rare code paths, emission read-back) are declared in nghmm_debug.h: tests, bench.py and the
 * profiling scripts use them; a host that only runs analyses does not need them. */

#ifdef __cplusplus
}
#endif
#endif /* NGHMM_H */
