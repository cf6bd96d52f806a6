/*
 * philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
 * 1, 2, 3", SC'11), host and device, and the uniform a sampled IBD path draws per site
 * (include/nghmm.h, nghmm_sample_paths).  A counter-based generator: the four output words are a
 * function of (key, counter) alone, so a draw does not depend on who computes it or in what order.
 */
#ifndef NGH_PHILOX_H
#define NGH_PHILOX_H

#include <stdint.h>

#if defined(__HIPCC__)
#define NGH_PX_HD __host__ __device__ __forceinline__
#else
#define NGH_PX_HD static inline
#endif

struct ngh_philox4 {
  uint32_t x[4];
};

NGH_PX_HD ngh_philox4 ngh_philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                        uint32_t c2, uint32_t c3) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;  /* the key schedule: bumped between rounds */
    k1 += 0xBB67AE85u;
  }
  ngh_philox4 o;
  o.x[0] = c0;
  o.x[1] = c1;
  o.x[2] = c2;
  o.x[3] = c3;
  return o;
}

/* The four words a pair of sites shares: key = seed, counter = (pair low, pair high, individual,
 * draw), pair = global site >> 1. */
NGH_PX_HD ngh_philox4 ngh_sample_words(uint64_t seed, uint32_t draw, uint32_t ind, uint64_t pair) {
  return ngh_philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pair,
                           (uint32_t)(pair >> 32), ind, draw);
}

/* u in [0, 1) of a site from its pair's words: an even site takes (x0, x1), an odd one (x2, x3);
 * 53 bits, the first word of the pair the low one. */
NGH_PX_HD double ngh_sample_uniform(const ngh_philox4& w, uint64_t site) {
  const uint32_t lo = (site & 1) ? w.x[2] : w.x[0], hi = (site & 1) ? w.x[3] : w.x[1];
  return (double)((((uint64_t)hi << 32) | lo) >> 11) * 1.1102230246251565404e-16; /* 2^-53 */
}

#endif
