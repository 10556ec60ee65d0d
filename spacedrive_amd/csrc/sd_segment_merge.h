// sd_segment_merge.h — the cross-lane half of the chunk-parallel kernels (K1L in
// cas_hash.hip, K1P in cas_inplace.hip): the lanes of a file segment each hold one subtree
// CV, and the segment merges them level by level into BLAKE3's left-balanced tree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake3_device.hpp"

namespace sdcas {

// Value of `x` held by lane (lane + S) of the same file segment (S < SEG, a power of two;
// lanes past the wave's end read 0 and are never used).  S < 16 stays inside a DPP row:
// DPP row_shl:S (lane i reads lane i + S of its 16-lane row) — no LDS, no extra issue.
// S = 16, 32 (only in 64-lane segments) cross rows: ds_bpermute (__shfl_down).
template <uint32_t S>
__device__ __forceinline__ uint32_t from_lane_above(uint32_t x) {
  if constexpr (S < 16)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 | (int)S, 0xF, 0xF, true);
  else
    return __shfl_down(x, S, 64);
}

// Level-wise pair-and-promote across the lanes of a segment: item i (a subtree CV) sits in
// segment lane i*s at the level with stride s; the left lane of a pair pulls its partner's
// 8 CV words with one cross-lane move each and compresses the parent.  `count` items at
// entry; ROOT on the last pair.  Every lane runs the moves (DPP needs full exec).
template <int SEG, uint32_t S>
__device__ __forceinline__ void segment_merge(uint32_t (&cv)[8], uint32_t sl, uint32_t& count) {
  if constexpr (S < (uint32_t)SEG) {
    uint32_t r[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) r[w] = from_lane_above<S>(cv[w]);
    const bool left = (sl & (2u * S - 1u)) == 0u;
    if (count > 1u && left && sl / S + 1u < count) parent(cv, cv, r, count == 2u ? (uint32_t)ROOT : 0u);
    count = (count + 1u) >> 1;
    segment_merge<SEG, 2u * S>(cv, sl, count);
  }
}

}  // namespace sdcas
