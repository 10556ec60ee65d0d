// cas_sampled.hpp — the sampled path's lane program and its region epilogue: what K1 and K1G
// (cas_hash.hip), K1V (dup_verify.hip) and tools/ubench_k1.hip share.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake3_lane.hpp"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_mix.h"

namespace sdcas {

// ---- K1: the sampled path, specialised --------------------------------------------
// Every message is le64(size) || 57,344 B: 56 full chunks (448 block PAIRS) + one 8-byte
// tail chunk.  A lane fetches one whole 128-B line (a block pair, 8 x dwordx4 issued back
// to back) per batch, so each line is consumed while it is still in L2 (fetching 64 B per
// block let the other half be evicted between blocks and doubled the HBM traffic), and
// each line is requested one compression ahead of its first block (cas_lane_sampled).

constexpr uint32_t SAMPLED_PAIRS = SAMPLED_CONTENT_LEN / 128;  // 448
constexpr uint32_t SAMPLED_CHUNKS = SAMPLED_CONTENT_LEN / 1024;  // 56 full chunks
static_assert(SAMPLED_PAIRS == 8 * SAMPLED_CHUNKS, "the sampled content is whole chunks of 8 lines");

// line() pinned where the source puts it: the machine scheduler otherwise sinks a line's
// loads down the basic block towards the next line's (same base register), which takes the
// lead that K1's schedule below is built for away again.
// (The A/B variants of the load — non-temporal loads, 1.6x slower; 64-file tiled LINE / QUAD
// layouts — live in tools/ubench_k1.hip with their measurements.)
__device__ __forceinline__ void load_pair_here(const uint4* __restrict__ q, uint32_t P,
                                               uint4 (&buf)[8]) {
  __builtin_amdgcn_sched_barrier(0);
  line(q, P, buf);
  __builtin_amdgcn_sched_barrier(0);
}

// The 5-deep chaining-value stack lives in LDS, word-major [depth][word][thread] so every
// push/pop is a conflict-free dword access.  It is touched once per 1 KiB chunk (16
// compressions), and moving its 40 words per lane out of VGPRs takes the kernel from 3
// to 4 waves per SIMD (VGPR budget <= 128); 80 KiB per 512-lane block = 2 blocks/CU.
constexpr int SAMPLED_DEPTH = 5;  // popcount(55) pending subtrees at most
constexpr int SAMPLED_BLOCK = 512;  // 256: 1-2 % slower, 128: 4 % (profiles/r01_k1_block_ab.log)

template <int B = SAMPLED_BLOCK>
using LdsStack = CvStack<B, false>;  // sp is wave-uniform on the sampled path

template <int BLK = SAMPLED_BLOCK>
__device__ __forceinline__ uint64_t cas_lane_sampled(const uint4* __restrict__ q, uint64_t size,
                                                     LdsStack<BLK>& stk) {
  uint4 A[8], B[8];
  uint32_t cv[8];
  // (through a lambda: called directly, the inliner's order changes and with it K1's code)
  auto push_chunk = [&](uint32_t total) { merge_push(stk, cv, total); };
  // The 448 lines are one flat sequence through two buffers, each refilled IN PLACE: A holds
  // the even lines and B the odd ones, and a buffer's next line is requested one compression
  // after its last block, once the first block of the OTHER buffer's line has read the
  // 2-word carry from the buffer's tail where it lies.  So every line is requested one
  // compression before its first block, nothing is renamed across the back edge and no
  // carry is copied (679.0 VALU instructions per compression in this loop, 101 VGPRs).
  // Requesting a line right after its buffer's last block gives it two compressions of
  // lead, but the carry then has to be copied out of the buffer first (2 moves per line)
  // and it measured slower than this (profiles/k1_pipeline/).
  B[7].z = (uint32_t)size;  // the carry into line 0: the le64(size) prefix
  B[7].w = (uint32_t)(size >> 32);
  line(q, 0, A);
  for (uint32_t c = 0;; ++c) {
    set_iv(cv);
#pragma unroll 1
    for (uint32_t pp = 0; pp < 4; ++pp) {  // 4 x (line in A, line in B) = 16 blocks
      const uint32_t P = 8u * c + 2u * pp;
      compress_lo<PREFIXED>(cv, A, B[7].z, B[7].w, c, pp == 0 ? (uint32_t)CHUNK_START : 0u);
      load_pair_here(q, P + 1, B);  // P is even and < 448: so is P + 1
      compress_hi<PREFIXED>(cv, A, c, 0u);
      compress_lo<PREFIXED>(cv, B, A[7].z, A[7].w, c, 0u);
      // Wave-uniform guard: no line >= 448 is ever requested (a batch's last row may end
      // with its allocation).  It is the loop's EXIT and not a branch around the loads: a
      // conditional load joins the old and the new buffer in a phi, which came out as a
      // second buffer and 64 v_mov_b64 per iteration (152 VGPRs, 3 waves per SIMD).
      if (P + 2u >= SAMPLED_PAIRS) goto last_block;
      load_pair_here(q, P + 2, A);
      compress_hi<PREFIXED>(cv, B, c, pp == 3 ? (uint32_t)CHUNK_END : 0u);
    }
    push_chunk(c + 1);
  }
last_block:  // line 447 is in B; nothing is left to request
  compress_hi<PREFIXED>(cv, B, SAMPLED_CHUNKS - 1, CHUNK_END);
  push_chunk(SAMPLED_CHUNKS);
  const uint32_t c0 = B[7].z, c1 = B[7].w;
  // tail chunk 56: the last 8 content bytes (the carry), one 8-byte block
  {
    const uint32_t m[16] = {c0, c1, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    set_iv(cv);
    compress(cv, m, SAMPLED_CHUNKS, 0u, 8u, CHUNK_START | CHUNK_END);
  }
  // 56 = 0b111000: the stack holds the 32-, 16- and 8-chunk subtrees
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    uint32_t left[8];
    stk.pop(left);
    parent(cv, left, cv, d == 2 ? (uint32_t)ROOT : 0u);
  }
  return key_of(cv);
}

constexpr int SAMPLED_BLOCK_NARROW = 256;

// A lane's output: its key, rep[f] = f and its (mixed key, file) row in the region of its
// coarse bucket.  The whole workgroup calls it (barriers) once every lane has its root: the
// stack columns are dead by then and their LDS holds the per-bucket ranks.
template <int B>
__device__ __forceinline__ void region_epilogue(uint32_t (&stack_lds)[SAMPLED_DEPTH][8][B],
                                                bool live, uint64_t f, uint64_t key,
                                                uint64_t* __restrict__ keys, const RegionOut& ro) {
  if (live) {
    keys[f] = key;
    ro.rep[f] = (uint32_t)f;
  }
  // REGIONS counters, REGIONS run bases, REGIONS spill offsets, the spill total and base
  uint32_t* hist = &stack_lds[0][0][0];
  uint32_t* base = hist + REGIONS;
  uint32_t* spoff = base + REGIONS;
  uint32_t* sp = spoff + REGIONS;  // sp[0] = this workgroup's spilled rows, sp[1] = their base
  static_assert(3 * REGIONS + 2 <= SAMPLED_DEPTH * 8 * B, "the epilogue fits the stack LDS");
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < REGIONS; i += B) hist[i] = 0;
  if (threadIdx.x == 0) sp[0] = 0;
  __syncthreads();
  const uint64_t m = mix64(key);
  const uint32_t bkt = (uint32_t)(m >> (64 - REGION_BITS));
  const uint32_t r = live ? atomicAdd(&hist[bkt], 1u) : 0u;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < REGIONS; i += B) {
    const uint32_t h = hist[i];
    const uint32_t g = h ? atomicAdd(&ro.cursor[i], h) : 0u;
    base[i] = g;
    // rows past the region's capacity: this workgroup's run of them for region i
    const uint64_t lo = g > ro.cap ? g : ro.cap;
    const uint32_t over = g + h > lo ? (uint32_t)(g + h - lo) : 0u;
    spoff[i] = over ? atomicAdd(&sp[0], over) : 0u;
    if (g <= ro.cap && g + h > ro.cap) atomicAdd(&ro.cursor[REGION_SPILL_WORD + 1], 1u);  // it filled
  }
  __syncthreads();
  if (sp[0]) {  // (uniform) a region is full: one spill reservation for the workgroup
    if (threadIdx.x == 0) {
      sp[1] = atomicAdd(&ro.cursor[REGION_SPILL_WORD], sp[0]);
      atomicOr(ro.overflow, 1u);
    }
    __syncthreads();
  }
  if (live) {
    const uint64_t slot = (uint64_t)base[bkt] + r;
    if (slot < ro.cap) {
      ro.rkeys[(uint64_t)bkt * ro.cap + slot] = m;
      ro.rfile[(uint64_t)bkt * ro.cap + slot] = (uint32_t)f;
    } else {
      const uint64_t d = (uint64_t)sp[1] + spoff[bkt] + (slot - (base[bkt] > ro.cap ? base[bkt] : ro.cap));
      ro.spill_keys[d] = m;
      ro.spill_file[d] = (uint32_t)f;
    }
  }
}

}  // namespace sdcas
