// expect_region.hpp -- a region of one handle and its pieces, as kernels_expect.hip and
// kernels_bylength.hip read them and as the C ABI layer cuts them (capi_chain_host.hpp).  Nothing
// here needs the HIP runtime: the host-only logic and its CPU test include it too.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define NGHMM_HOST_DEVICE __host__ __device__
#else
#define NGHMM_HOST_DEVICE
#endif

namespace nghmm {

// A region of one handle, in handle-local sites, half-open; the regions are sorted and disjoint and
// the same for every individual.  Fast mode: piece0 = slot of the region's first piece within an
// individual's pieces (one piece per lane-chunk the region touches).
struct ExpectRegion {
  uint64_t begin, end, piece0, pad;
};
static_assert(sizeof(ExpectRegion) == 32, "ExpectRegion");

// pieces of a region [begin, end) in a layout of T sites per lane
NGHMM_HOST_DEVICE inline uint64_t expect_pieces(uint64_t begin, uint64_t end, uint64_t T) {
  return (end - 1) / T - begin / T + 1;
}

}  // namespace nghmm
