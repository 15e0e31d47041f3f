// ld_records.h -- the consumer side of the pair records on the device: which record a lane of a work item reads, a TSV
// column's field of a record, a wavefront's max and sum, the words of the sum / max / linked accumulators.  Shared by the TSV rows (ld_text.hip) and the record passes of ngsld_prune,
// ngsld_decay, ngsld_blocks, ngsld_site_ld, ngsld_clusters, ngsld_grid and ngsld_linked_pairs (prune.hip, decay.hip, blocks.hip,
// site_ld.hip, cluster.hip, grid.hip, linked.hip), which all map one wavefront to an item and one lane to a candidate.  Not part of the ld_device.h umbrella: the pair kernels never see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ngsld.h"

namespace ngsld {

// the record of candidate c of an item, in a buffer that starts at global record out_base: an item's records are its
// computed candidates (mask bits set) in order, so this is meaningful only where bit c of the mask is set
__device__ __forceinline__ uint64_t record_of(const ngsld_item &it, uint32_t c, uint64_t out_base) {
  return it.first_record - out_base + (uint64_t)__popcll(it.mask & ((1ull << c) - 1ull));
}

// field f of a record: 0 r2_ExpG, 1 D, 2 D', 3 r2 (TSV columns 4..7, the order of ngsld_rec_std)
__device__ __forceinline__ double field_of(const ngsld_rec_std &r, int f) {
  return f == 0 ? r.r2_ExpG : f == 1 ? r.D : f == 2 ? r.Dp : r.r2;
}

// The accumulators of ngsld_site_ld and ngsld_grid are words [1 + 3 * fields][entries]: rows; then per field the int64 sum (two's
// complement), the maximum, the linked rows (record_pass.h unpacks them on the host).
// a maximum is kept as q + kMaxBias > 0 (|q| < 2^38): 0 is "no row yet", and an unsigned max does the rest
constexpr unsigned long long kMaxBias = 1ull << 38;
__device__ __forceinline__ bool is_max_word(uint32_t w) { return w > 0 && (w - 1) % 3 == 1; }

// the max of v over the 64 lanes, in every lane
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(v, o);
    v = x > v ? x : v;
  }
  return v;
}

// the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace ngsld
