/*
 * nghmm_chain_long.h -- nghmm_ibd_long (include/nghmm.h) over a chain of site shards.
 *
 * A header of its own for the size of include/nghmm.h alone: it is a public header like that one.
 * tests/test_replica_battery_cpu.py and tests/test_chain_battery_cpu.py read every header under
 * include/ but nghmm_debug.h, so nghmm_ibd_long and this twin are held to the replica, layout and
 * chain batteries (tests/replica_util.py, tests/layout_util.py, tests/chain_util.py) like every
 * other output entry point.
 */
#ifndef NGHMM_CHAIN_LONG_H
#define NGHMM_CHAIN_LONG_H

#include "nghmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same over a chain of site shards (nghmm_chain_setup, else NGHMM_ERR_ARG): global site
 * indices; fast mode only for more than one handle.  Q, n and U start afresh in every shard and a
 * window across a cut is the product of its two parts.  A shard takes from its RIGHT neighbour Q
 * and n of the neighbour's first sites as far as its b_k windows reach (as
 * nghmm_chain_ibd_by_length), and from its LEFT neighbour's last sites, as far as its lo_k
 * windows reach: pi, the sum of ln rho and the blocked steps from the site to the cut, and T_k,
 * added on the host from the cut outwards; and the neighbour's U at the cut.  Across a cut B_k is
 * that sum plus the shard's own U: no difference is taken.  A threshold whose window reaches past
 * the neighbouring shard is NGHMM_ERR_ARG with a message that says in which direction.  A region
 * across a cut is one region, its parts added on the host in rank order; post and the site
 * records are the concatenation of the shards'.  The results are within rounding of a single
 * handle's, not its bytes. */
int nghmm_chain_ibd_long(nghmm_t** hs, int n_handles, int what, uint32_t n_lengths, const double* min_length,
                         double threshold, uint64_t n_regions, const uint64_t* region_begin,
                         const uint64_t* region_end, nghmm_long_region_stat* region_stats,
                         nghmm_long_site_stat* site_stats, double* post);

#ifdef __cplusplus
}
#endif

#endif
