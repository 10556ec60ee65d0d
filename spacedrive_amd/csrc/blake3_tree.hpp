// blake3_tree.hpp — the level-wise pair-and-promote that makes BLAKE3's left-balanced tree, once:
// the level rule (TreeLevel), the in-LDS reduction over a scope of lanes (K3, the validator's
// batch kernels) and the cross-lane merge of a wave segment (K1L, K1P).  The rule and the per-slot
// phases compile for the host: tests/native/tree_reduce_test.cpp runs them over simulated lanes
// against the recursive definition and the oracle, under sanitizers.
#pragma once
#include "blake3_device.hpp"
#if defined(__HIPCC__)
#include "sd_debug.h"
#endif

namespace sdcas {

// One level over `count` CVs: slots 2p and 2p+1 form parent p, an odd last CV is carried to
// slot count/2, and the parent formed from the last two CVs is the tree's top.  A level of
// <= 1 CVs does nothing and stays, so lanes that are done may idle through further levels.
struct TreeLevel {
  uint32_t count;
  SD_B3_HD bool merges(uint32_t p) const { return p < (count >> 1); }
  SD_B3_HD bool carries(uint32_t p) const { return count > 1u && (count & 1u) && p == (count >> 1); }
  SD_B3_HD bool top() const { return count == 2u; }
  SD_B3_HD TreeLevel next() const { return TreeLevel{(count + 1u) >> 1}; }
  SD_B3_HD bool merges_at(uint32_t lane, uint32_t S) const {  // stride form: item i in lane i*S
    const bool left = (lane & (2u * S - 1u)) == 0u;
    return count > 1u && left && lane / S + 1u < count;
  }
};

// ---- in LDS: cvs[count][8] -> cvs[0] ---------------------------------------------------------
// A level's two phases for slot p.  A scope's lanes own slots lane, lane + lanes, ...; every
// lane's reads finish before any lane's writes (parent p overwrites slot p, which another
// lane's pair may read).  `root_last`: the top parent carries ROOT.
SD_B3_HD void level_read(TreeLevel lv, const uint32_t (*cvs)[8], uint32_t p, bool root_last, uint32_t (&out)[8]) {
  if (lv.merges(p)) {
    uint32_t l[8], r[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) { l[w] = cvs[2 * p][w]; r[w] = cvs[2 * p + 1][w]; }
    parent(out, l, r, (root_last && lv.top()) ? (uint32_t)ROOT : 0u);
  } else if (lv.carries(p)) {
#pragma unroll
    for (int w = 0; w < 8; ++w) out[w] = cvs[lv.count - 1u][w];
  }
}
SD_B3_HD void level_write(TreeLevel lv, uint32_t (*cvs)[8], uint32_t p, const uint32_t (&out)[8]) {
  if (lv.merges(p) || lv.carries(p)) {
#pragma unroll
    for (int w = 0; w < 8; ++w) cvs[p][w] = out[w];
  }
}

// ---- stride form: one CV per lane of a segment, item i stays in lane i*S (a carry does not move)
// The level with stride S for one lane: cv is its own item, r that of lane + S.  ROOT on the top.
SD_B3_HD void stride_level(TreeLevel lv, uint32_t (&cv)[8], const uint32_t (&r)[8], uint32_t lane, uint32_t S) {
  if (lv.merges_at(lane, S)) parent(cv, cv, r, lv.top() ? (uint32_t)ROOT : 0u);
}

#if defined(__HIPCC__)
// wave-synchronous LDS phases (no workgroup barrier: orders this wave's own LDS accesses)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Who reduces together.  `trips(count)` is a count whose levels every lane that reaches the
// syncs runs: the scope's own, or, where the slices of one wave differ, the largest possible.
struct Workgroup256 {
  static constexpr uint32_t lanes = 256;
  __device__ static uint32_t lane() { return threadIdx.x; }
  __device__ static uint32_t trips(uint32_t count) { return count; }
  __device__ static void sync() { __syncthreads(); }
};
template <uint32_t SEG>  // a SEG-lane slice of a wave with its own count; 64: the wave
struct WaveSlice {
  static constexpr uint32_t lanes = SEG;
  __device__ static uint32_t lane() { return threadIdx.x % SEG; }
  __device__ static uint32_t trips(uint32_t count) { return SEG == 64 ? count : SEG; }
  __device__ static void sync() { wave_sync(); }
};

// Pair-and-promote `count` (<= 2 * PER * lanes) CVs in the scope's LDS slice down to cvs[0]:
// per level all reads and parents, sync, all writes, sync.
template <class Scope, int PER>
__device__ __forceinline__ void tree_reduce(uint32_t (*cvs)[8], uint32_t count, bool root_last) {
  SD_DBG_CHECK(count <= 2u * PER * Scope::lanes, "tree reduce: %u CVs, %u lanes x %d", count, Scope::lanes, PER);
  TreeLevel lv{count};
#pragma unroll 1
  for (TreeLevel trip{Scope::trips(count)}; trip.count > 1u; trip = trip.next(), lv = lv.next()) {
    uint32_t out[PER][8];
#pragma unroll
    for (int k = 0; k < PER; ++k) level_read(lv, cvs, Scope::lane() + k * Scope::lanes, root_last, out[k]);
    Scope::sync();
#pragma unroll
    for (int k = 0; k < PER; ++k) level_write(lv, cvs, Scope::lane() + k * Scope::lanes, out[k]);
    Scope::sync();
  }
}

// Value of `x` held by lane (lane + S) of the same file segment (S < SEG, a power of two; lanes
// past the wave's end read 0 and are never used).  S < 16: DPP row_shl:S (lane i reads lane i + S
// of its 16-lane row) — no LDS, no extra issue.  S = 16, 32 cross rows: ds_bpermute (__shfl_down).
template <uint32_t S>
__device__ __forceinline__ uint32_t from_lane_above(uint32_t x) {
  if constexpr (S < 16)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 | (int)S, 0xF, 0xF, true);
  else
    return __shfl_down(x, S, 64);
}

// Across the lanes of a segment (K1L, K1P): `count` items at entry, item i in segment lane
// i; the left lane of a pair pulls its partner's 8 CV words with one cross-lane move each.
// Every lane runs the moves (DPP needs full exec).
template <int SEG, uint32_t S>
__device__ __forceinline__ void segment_merge(uint32_t (&cv)[8], uint32_t sl, uint32_t& count) {
  if constexpr (S < (uint32_t)SEG) {
    uint32_t r[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) r[w] = from_lane_above<S>(cv[w]);
    stride_level(TreeLevel{count}, cv, r, sl, S);
    count = TreeLevel{count}.next().count;
    segment_merge<SEG, 2u * S>(cv, sl, count);
  }
}
#endif  // __HIPCC__

}  // namespace sdcas
