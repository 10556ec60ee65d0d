// dup_slice.hpp — one slice of a content in a wave's registers and its compare, shared by K1V's
// row compare (dup_verify.hip) and the whole-content compare (content_compare.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_dup_runs.h"

namespace sdcas {

// lane l holds quads u * DUP_WAVE + l of the slice, u < DUP_SLICE_QUADS: every wave-load is 64
// lanes x 16 B contiguous
struct DupSlice { uint4 q[DUP_SLICE_QUADS]; };

__device__ __forceinline__ bool dup_slices_differ(const DupSlice& a, const DupSlice& b) {
  uint32_t d = 0;
#pragma unroll
  for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u)
    d |= (a.q[u].x ^ b.q[u].x) | (a.q[u].y ^ b.q[u].y) | (a.q[u].z ^ b.q[u].z) | (a.q[u].w ^ b.q[u].w);
  return __builtin_amdgcn_ballot_w64(d != 0) != 0;  // (wave-uniform)
}
__device__ __forceinline__ uint32_t dup_first_bit(uint32_t m) {  // m != 0, uniform
  return (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctz(m));
}

}  // namespace sdcas
