// cas_hash.hip — batched generate_cas_id on gfx950 (K1 sampled path, K2 whole-file path).
//
// Replaces, per batch, the per-file hashing of core/src/object/cas.rs:23-62:
//   message M(s) = le64(size) || content, content = whole file (size <= 102,400,
//   cas.rs:27-29) or header 8 KiB || 4 x 10 KiB samples || footer 8 KiB (cas.rs:31-58,
//   gathered on the host); cas_id = hex(BLAKE3(M)[0..8]) (cas.rs:61).
//
// Mapping: ONE FILE PER LANE.  Every lane walks its own message and keeps the BLAKE3
// chaining-value stack in an LDS column of its own.  For the sampled path every file has
// the same 57 chunks, so all control flow (block loop, stack merges) is wave-uniform and
// every lane does useful work in every instruction: 953 compressions per lane, no
// cross-lane traffic.  For the whole-file path files are pre-sorted by message length
// (on-device key sort) so the lanes of a wave finish together.
//
// Memory: each lane streams its message in 128-B lines (a block pair, 8 x
// global_load_dwordx4), two lines per loop iteration.  The le64(size) prefix
// shifts the content by exactly two 32-bit words, which becomes register renaming (a
// 2-word carry), not byte shuffling.
//
// Bound: VALU issue.  On gfx950 v_alignbit_b32 / v_add3_u32 (like every 3-input or SDWA
// VALU op except v_bitop3) issue at half rate (tools/ubench_valu.hip,
// profiles/r01_ubench_valu.log), so a compression costs ~1014 full-rate issue slots.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake3_lane.hpp"
#include "blake3_tree.hpp"
#include "dup_slice.hpp"
#include "sd_debug.h"
#include "sd_dup_probe.h"
#include "sd_dup_runs.h"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_mix.h"
#include "sd_ws.h"

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

// K1: sampled path, uniform 57,344-B contents at a fixed stride (>= 57,344, 16-B aligned).
// Two grid shapes of the same lane program: 512-lane workgroups (80 KiB of LDS stack, 2 per
// CU) for batches of >= 2 quanta, and 256-lane workgroups (40 KiB, 4 per CU) below: a batch
// of one quantum is 128 workgroups of 512 lanes, which the dispatcher puts on 128 CUs at 2
// waves per SIMD — half the chip idle and twice the latency (measured 2.27 vs 1.15 ms for
// 65,536 files, profiles/r02_latency_sweep.log) — while 256 workgroups of 256 lanes put one
// wave on every SIMD.
template <int B>
__device__ __forceinline__ void sampled_kernel_body(const uint8_t* __restrict__ content,
                                                    uint64_t stride,
                                                    const uint64_t* __restrict__ sizes, uint64_t n,
                                                    uint64_t* __restrict__ keys) {
  __shared__ uint32_t stack_lds[SAMPLED_DEPTH][8][B];
  const uint64_t f = (uint64_t)blockIdx.x * B + threadIdx.x;
  if (f >= n) return;  // no barrier below: each lane only touches its own stack column
  LdsStack<B> stk{stack_lds, threadIdx.x};
  const uint4* q = reinterpret_cast<const uint4*>(content + f * stride);
  keys[f] = cas_lane_sampled<B>(q, sizes[f], stk);
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK)
sd_cas_sampled_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                      const uint64_t* __restrict__ sizes, uint64_t n,
                      uint64_t* __restrict__ keys) {
  sampled_kernel_body<SAMPLED_BLOCK>(content, stride, sizes, n, keys);
}

constexpr int SAMPLED_BLOCK_NARROW = 256;
extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK_NARROW)
sd_cas_sampled_kernel_256(const uint8_t* __restrict__ content, uint64_t stride,
                          const uint64_t* __restrict__ sizes, uint64_t n,
                          uint64_t* __restrict__ keys) {
  sampled_kernel_body<SAMPLED_BLOCK_NARROW>(content, stride, sizes, n, keys);
}

// ---- K1G: K1 + the grouping's partition, fused (sd_cas_hash_group_sampled_dev) ----------
// The Object grouping needs each key once more after K1 has written it: the standalone chain
// reads the keys back (bucket totals, 8 B/key), prefills rep (4 B/key), then scatters the
// keys into coarse-bucket order (8 B read + 12 B write) before the bucket tables.  K1 holds
// every key in a register when it finishes, so K1G does that partition in its epilogue
// instead: the lane's (mixed key, file) row goes straight into a FIXED-capacity region of
// its coarse bucket (the top 8 bits of mix64(key)); the workgroup ranks its lanes per bucket
// in LDS (the CV stack's LDS, dead by then) and reserves each bucket's run with one device
// atomic.  The chain after K1G is one bucket-table launch.  Regions are sized mean + 8
// sigma + 64 rows for uniform keys; a bucket that outgrows its region (heavily duplicated
// content: every copy of a file lands in one bucket) keeps counting in its cursor, appends
// its extra rows to the set's spill list (one reservation per workgroup that has any) and
// sets *overflow; that region's table workgroup reads its region rows and its spilled rows
// (sd_bucket_min_regions) — only the overflowed regions pay, on the device, no host regroup.
struct RegionOut {
  uint64_t* rkeys;     // [REGIONS][cap] mixed keys
  uint32_t* rfile;     // [REGIONS][cap] file index
  uint32_t* cursor;    // [REGION_SET_WORDS] rows reserved per region, then the spill count and
                       // the full-region count at REGION_SPILL_WORD; zero on entry (the bucket
                       // tables re-zero them)
  uint64_t cap;
  uint64_t* spill_keys;   // rows past their region's capacity (mixed key, file), unordered
  uint32_t* spill_file;
  uint32_t* rep;       // rep[f] = f: the bucket tables store only where a key's minimum differs
  uint32_t* overflow;  // set when a region is full
  // objects[0]: zeroed here, the bucket tables add the distinct keys; objects[1]: zeroed
  // here, the tables' carve cursor for the global tables of overflowed regions
  unsigned long long* objects;
};

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

template <int B>
__device__ __forceinline__ void sampled_group_kernel_body(const uint8_t* __restrict__ content,
                                                          uint64_t stride,
                                                          const uint64_t* __restrict__ sizes,
                                                          uint64_t n, uint64_t* __restrict__ keys,
                                                          RegionOut ro) {
  __shared__ uint32_t stack_lds[SAMPLED_DEPTH][8][B];
  const uint64_t f = (uint64_t)blockIdx.x * B + threadIdx.x;
  const bool live = f < n;
  uint64_t key = 0;
  if (live) {  // exactly K1's lane program
    LdsStack<B> stk{stack_lds, threadIdx.x};
    const uint4* q = reinterpret_cast<const uint4*>(content + f * stride);
    key = cas_lane_sampled<B>(q, sizes[f], stk);
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) ro.objects[threadIdx.x] = 0;
  region_epilogue<B>(stack_lds, live, f, key, keys, ro);
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK)
sd_cas_sampled_group_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                            const uint64_t* __restrict__ sizes, uint64_t n,
                            uint64_t* __restrict__ keys, RegionOut ro) {
  sampled_group_kernel_body<SAMPLED_BLOCK>(content, stride, sizes, n, keys, ro);
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK_NARROW)
sd_cas_sampled_group_kernel_256(const uint8_t* __restrict__ content, uint64_t stride,
                                const uint64_t* __restrict__ sizes, uint64_t n,
                                uint64_t* __restrict__ keys, RegionOut ro) {
  sampled_group_kernel_body<SAMPLED_BLOCK_NARROW>(content, stride, sizes, n, keys, ro);
}

// ---- K1V: K1G with duplicate contents verified by comparison, not hashed -----------------
// Two files of equal size and equal 57,344 content bytes have the same message, so the same
// key: the second one's 953 compressions buy nothing.  Proving the bytes equal costs one more
// read of the copy's row, one read of the original's row per run of its copies, and ~40 VALU
// instructions per 128-B line against 1,360 to hash it.
//   1. sd_dup_probe_kernel: a 64-bit probe per file (sd_dup_probe.h: size, first and last 32 B);
//      the hash grouping gives cand[f] = the smallest file with f's probe.  cand[f] == f: hash
//      f.  Otherwise f is a candidate duplicate of cand[f] (which is hashed: cand[cand[f]] ==
//      cand[f]).
//   2. sd_dup_compact_kernel: list H (to hash), and each candidate's rank among the candidates
//      of its original (cnt[cand[f]]++); exclusive_scan_u32 of cnt gives every original's first
//      slot and sd_dup_order_kernel writes list C, the candidates ordered by original.  The
//      order inside a group is the atomics' (no result depends on it); the counts stay on the
//      device.
//   3. sd_cas_dup_mixed_kernel, K1G's grid + 1 workgroup: hash tiles run K1G's lane program and
//      epilogue on H[tile * B + lane]; compare tiles take a wave per task, a window of
//      DUP_RUN_K entries of list C (sd_dup_runs.h), read the original once per run of its
//      copies and write same[f].  Compare tiles lie among the hash tiles, so their loads run
//      beside the hash waves' VALU work, and at the grid's end, where they fill the last hash
//      round's drain.  Which workgroup does what is either fixed before launch (dup_tile_of) or,
//      for large grids, taken at run time by each workgroup as it starts: at most one compare
//      workgroup of one wave per SIMD on a CU, the others hashing (sd_dup_runs.h).
//   4. sd_cas_dup_finish_kernel over C: a verified file takes keys[cand[f]]; an unverified one
//      (a probe collision) is hashed here, under a wave-level branch; every C file then gets
//      rep[f] = f and its region row through the same epilogue.
// The bucket tables after it see the same rows as after K1G, in another order.
struct DupLists {
  const uint32_t* cand;  // [n] smallest file with the same probe
  uint32_t* list_h;      // [n] files to hash (counters[0] of them)
  uint32_t* list_c;      // [n] candidates (counters[1]), the copies of one original consecutive
  uint32_t* same;        // [n] same[f] = 1: f's size and bytes equal cand[f]'s (C files only)
  uint32_t* cnt;         // [n] cnt[g] = candidates of original g (zeroed by the probe kernel)
  uint32_t* first;       // [n] first[g] = list C slot of g's first candidate (cnt's scan)
  uint32_t* rank;        // [n] rank[f] = f's place among cand[f]'s candidates (C files only)
  uint32_t* counters;    // DUP_COUNTERS words
  uint32_t* cu;          // DUP_CU_SLOTS words: compare workgroups resident per CU (run-time roles)
  uint32_t tail_tiles;   // compare tiles at the grid's end (the mixed kernel), >= 1; 0: roles are
                         // taken at run time (sd_dup_runs.h)
  uint32_t slots;        // workgroups of the main kernel that the chip holds at once
  // the host's view of this call, in pinned host memory: {seq, candidates, files}, seq stored last
  volatile uint32_t* note;
  uint32_t seq, files;
};
// counters: files to hash, candidates, verified, rehashed, the mixed kernel's task queue,
// groups (originals with a candidate), tasks run, reference rows read (one per run of a task);
// run-time roles: the hash-tile queue, compare workgroups started; the debug library's conservation
// check: hash tiles run, and how many the launched grid shape has
constexpr uint32_t DUP_N_HASH = 0, DUP_N_CAND = 1, DUP_VERIFIED = 2, DUP_REHASHED = 3, DUP_QUEUE = 4,
                   DUP_GROUPS = 5, DUP_TASKS = 6, DUP_REFS = 7, DUP_HASH_QUEUE = 8, DUP_COMPARE_WGS = 9,
                   DUP_TILES_RUN = 10, DUP_TILES_WANT = 11;
static_assert(DUP_TILES_RUN < DUP_TILES_WANT && DUP_TILES_WANT < DUP_COUNTERS, "counters");

extern "C" __global__ void __launch_bounds__(256)
sd_dup_probe_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                    const uint64_t* __restrict__ sizes, uint64_t n, uint64_t* __restrict__ probes,
                    uint32_t* __restrict__ counters, uint32_t* __restrict__ cu,
                    uint32_t* __restrict__ cnt) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < DUP_COUNTERS) counters[threadIdx.x] = 0;
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < DUP_CU_SLOTS; i += 256) cu[i] = 0;
  if (f < n) {
    probes[f] = dup_probe(sizes[f], content + f * stride);
    cnt[f] = 0;
  }
}

// One reservation per workgroup for list H, which keeps the file order inside a workgroup's run.
// wcnt rows: files to hash, candidates, groups (candidates of rank 0).
extern "C" __global__ void __launch_bounds__(256)
sd_dup_compact_kernel(uint64_t n, DupLists dl) {
  __shared__ uint32_t wcnt[3][4], base;
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const bool live = f < n;
  const uint32_t g = live ? dl.cand[f] : 0u;
  const bool h = live && g == (uint32_t)f;
  const bool c = live && !h;
  uint32_t r = 1;
  if (c) {
    r = atomicAdd(&dl.cnt[g], 1u);
    dl.rank[f] = r;
  }
  const uint64_t bh = __ballot(h), bc = __ballot(c), bg = __ballot(r == 0);
  const uint64_t below = (1ull << lane) - 1ull;
  if (lane == 0) {
    wcnt[0][w] = (uint32_t)__popcll(bh);
    wcnt[1][w] = (uint32_t)__popcll(bc);
    wcnt[2][w] = (uint32_t)__popcll(bg);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    constexpr uint32_t word[3] = {DUP_N_HASH, DUP_N_CAND, DUP_GROUPS};
    const uint32_t t = wcnt[threadIdx.x][0] + wcnt[threadIdx.x][1] + wcnt[threadIdx.x][2] +
                       wcnt[threadIdx.x][3];
    const uint32_t b = t ? atomicAdd(&dl.counters[word[threadIdx.x]], t) : 0u;
    if (threadIdx.x == 0) base = b;
  }
  __syncthreads();
  uint32_t oh = base + (uint32_t)__popcll(bh & below);
  for (uint32_t i = 0; i < w; ++i) oh += wcnt[0][i];
  if (h) dl.list_h[oh] = (uint32_t)f;
}

// list C: candidate f goes to its original's first slot + its rank (< counters[DUP_N_CAND])
extern "C" __global__ void __launch_bounds__(256)
sd_dup_order_kernel(uint64_t n, DupLists dl) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const uint32_t g = dl.cand[f];
  if (g != (uint32_t)f) dl.list_c[dl.first[g] + dl.rank[f]] = (uint32_t)f;
}

// One wave runs task t: entries [first, first + m) of list C, entry e in lane e.  Sizes are
// compared once per entry; then, slice by slice (sd_dup_runs.h: 8 KiB, 8 quads per lane), the
// wave holds the current original's slice in registers and streams the slices of the entries
// still alive against it, the next entry's loads issued before the current one is compared.
// The reference is loaded again only where cand changes among the alive entries, and a refuted
// entry is not read again.  Returns the task's runs (reference rows); writes same[f].  Nothing
// is read past a row's 57,344th byte: the largest offset is dup_slice_quad_offset(6, 7, 63) + 16.
// A lane is known by its byte offset in a 1-KiB load (voff = 16 lane) alone, and the lane number
// is derived from it afresh where a task needs it (dup_lane_of: opaque to the optimizer, which
// would otherwise keep both in registers over the loop and take the kernel past K1G's 101 VGPRs).
// (DupSlice, dup_slices_differ and dup_first_bit: dup_slice.hpp)
// row is wave-uniform.  The loads go through a buffer descriptor of the row's 57,344 bytes: a
// lane's address is its one 32-bit offset, each quad's offset in the row is scalar, and the
// hardware bounds every load to the row.
typedef uint32_t dup_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dup_load_slice(DupSlice& d, const uint8_t* __restrict__ content,
                                               uint64_t stride, uint32_t file, uint32_t s, uint32_t voff) {
  const uint64_t a = (uint64_t)content + (uint64_t)file * stride;
  const uint64_t row = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, (int)DUP_ROW_BYTES, 0x00020000);
#pragma unroll
  for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u) {
    const dup_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff,
                                                              (int)dup_slice_quad_offset(s, u, 0), 0);
    d.q[u] = make_uint4(v.x, v.y, v.z, v.w);
  }
}
__device__ __forceinline__ uint32_t dup_lane_of(uint32_t voff) {
  uint32_t lane;
  asm volatile("v_lshrrev_b32 %0, 4, %1" : "=v"(lane) : "v"(voff));
  return lane;
}

__device__ __forceinline__ uint32_t dup_compare_task(const uint8_t* __restrict__ content, uint64_t stride,
                                                     const uint64_t* __restrict__ sizes,
                                                     const DupLists& dl, uint32_t t, uint32_t n_cand,
                                                     uint32_t voff) {
  uint32_t lane = dup_lane_of(voff);
  const uint32_t first = dup_task_first(t), m = dup_task_entries(t, n_cand);
  uint32_t f = 0, g = 0;
  bool ok = false;
  if (lane < m) {
    f = dl.list_c[first + lane];
    g = dl.cand[f];
    ok = sizes[f] == sizes[g];
  }
  // a run starts at the window's first entry and at an original's first slot of list C
  bool head = lane < m;
  if (head && lane) head = dl.first[g] == first + lane;
  const uint32_t heads = (uint32_t)__ballot(head);  // (uniform) bit e: entry e starts a run
  const uint32_t runs = (uint32_t)__builtin_popcount(heads);
  uint32_t alive = (uint32_t)__ballot(ok);  // entries not refuted yet (uniform; m <= 32)
#pragma unroll 1
  for (uint32_t s = 0; s < DUP_SLICES && alive; ++s) {
    DupSlice ref, cur, nxt;
    uint32_t left = alive;
    uint32_t e = dup_first_bit(left);
    // e's run is the number of heads up to e; its original is read from cand[] where the run
    // changes, so the lanes keep their entry's file and not its original over the loop
    uint32_t fe = (uint32_t)__builtin_amdgcn_readlane((int)f, (int)e);
    uint32_t loaded = (uint32_t)__builtin_popcount(heads & ((2u << e) - 1u));
    dup_load_slice(ref, content, stride, (uint32_t)__builtin_amdgcn_readfirstlane((int)dl.cand[fe]), s, voff);
    dup_load_slice(cur, content, stride, fe, s, voff);
#pragma unroll 1
    for (;;) {
      left &= left - 1u;
      uint32_t e2 = 0;
      if (left) {  // (uniform) the next alive entry's slice, in flight during this compare
        e2 = dup_first_bit(left);
        fe = (uint32_t)__builtin_amdgcn_readlane((int)f, (int)e2);
        dup_load_slice(nxt, content, stride, fe, s, voff);
      }
      if (dup_slices_differ(ref, cur)) alive &= ~(1u << e);
      if (!left) break;
      e = e2;
      cur = nxt;
      const uint32_t run = (uint32_t)__builtin_popcount(heads & ((2u << e) - 1u));
      if (run != loaded) {  // (uniform) the window's next original
        loaded = run;
        dup_load_slice(ref, content, stride, (uint32_t)__builtin_amdgcn_readfirstlane((int)dl.cand[fe]), s, voff);
      }
    }
  }
  lane = dup_lane_of(voff);
  if (lane < m) dl.same[f] = (alive >> lane) & 1u;
  return runs;
}

// The CU this wave runs on, as a slot of DupLists::cu.
__device__ __forceinline__ uint32_t dup_this_cu_slot() {
  constexpr int HW_REG_HW_ID = 4, HW_REG_XCC_ID = 20, WHOLE = 31 << 11;  // simm16: id | offset << 6 | (size - 1) << 11
  return dup_cu_slot(__builtin_amdgcn_s_getreg(HW_REG_XCC_ID | WHOLE),
                     __builtin_amdgcn_s_getreg(HW_REG_HW_ID | WHOLE));
}

template <int B>
__device__ __forceinline__ void dup_mixed_kernel_body(const uint8_t* __restrict__ content,
                                                      uint64_t stride,
                                                      const uint64_t* __restrict__ sizes,
                                                      uint64_t* __restrict__ keys, RegionOut ro,
                                                      DupLists dl) {
  __shared__ uint32_t stack_lds[SAMPLED_DEPTH][8][B];
  const uint32_t n_hash = dl.counters[DUP_N_HASH], n_cand = dl.counters[DUP_N_CAND];
  // the grid is n / B + 1 workgroups: TH hash tiles, and at least one compare tile
  const uint32_t G = gridDim.x;
  const uint32_t TH = (n_hash + B - 1) / B;
  // The last tail_tiles workgroups of the grid are compare tiles that run until the task queue
  // is empty: they start as the last round of hash tiles drains and fill the slots it frees
  // (a hash tile is one indivisible ~4 ms; a task is a few hundred us at most).  The other
  // compare tiles lie evenly among the hash tiles and take one tile's worth of entries each (a
  // lane's worth per lane: dup_tile_wave_tasks), so compare loads run beside the hashing from
  // the start (dup_tile_of, sd_dup_runs.h).
  DupTile tile;
  uint32_t quota = dup_tile_wave_tasks();
  bool leaves_cu = false;  // (uniform) a compare workgroup that is counted in its CU's slot
  const bool roles = B == (int)DUP_ROLE_BLOCK && dl.tail_tiles == 0;  // (uniform)
  if (roles) {
    // Roles taken at run time (sd_dup_runs.h): lane 0 decides, and the workgroup reads the role
    // from a stack word that is dead until the hashing starts (hence the second barrier).
    const uint32_t n_tasks = dup_task_count(n_cand);
    if (threadIdx.x == 0) {
      uint32_t role = DUP_ROLE_COMPARE;
      bool compare = dup_wants_compare(
          __hip_atomic_load(&dl.counters[DUP_QUEUE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), n_tasks,
          __hip_atomic_load(&dl.counters[DUP_HASH_QUEUE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), TH);
      if (compare) {
        const uint32_t slot = dup_this_cu_slot();
        compare = dup_cu_has_room(atomicAdd(&dl.cu[slot], 1u)) &&
                  atomicAdd(&dl.counters[DUP_COMPARE_WGS], 1u) < dup_compare_budget(G, TH);
        if (!compare) atomicSub(&dl.cu[slot], 1u);
        stack_lds[0][0][1] = slot;  // a compare workgroup never touches the stack: kept for its exit
      }
      if (!compare) {
        role = atomicAdd(&dl.counters[DUP_HASH_QUEUE], 1u);
        if (role >= TH) role = DUP_ROLE_DRAIN;  // no hash tile left: the drain fills itself
      }
      stack_lds[0][0][0] = role;
    }
    __syncthreads();
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)stack_lds[0][0][0]);
    __syncthreads();
    // (a compare workgroup of a grid that is resident all at once has no quota: sd_dup_runs.h)
    tile = DupTile{role >= DUP_ROLE_COMPARE, role == DUP_ROLE_DRAIN || !dup_compare_has_quota(G, dl.slots), role};
    quota = dup_role_wave_tasks();
    leaves_cu = role == DUP_ROLE_COMPARE;
  } else {
    tile = dup_tile_of(blockIdx.x, G, TH, dl.tail_tiles);
  }
#if SD_DBG
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) dl.counters[DUP_TILES_WANT] = TH;
    if (!tile.compare) atomicAdd(&dl.counters[DUP_TILES_RUN], 1u);
  }
#endif
  if (blockIdx.x == 0 && threadIdx.x < 2) ro.objects[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && dl.note) {
    dl.note[1] = n_cand;
    dl.note[2] = dl.files;
    __threadfence_system();
    dl.note[0] = dl.seq;
  }
  if (!tile.compare) {  // a hash tile: K1G's lane program on list H
    const uint32_t i = tile.hash_tile * B + threadIdx.x;
    const bool live = i < n_hash;
    uint64_t f = 0, key = 0;
    if (live) {
      f = dl.list_h[i];
      LdsStack<B> stk{stack_lds, threadIdx.x};
      const uint4* q = reinterpret_cast<const uint4*>(content + f * stride);
      key = cas_lane_sampled<B>(q, sizes[f], stk);
    }
    region_epilogue<B>(stack_lds, live, f, key, keys, ro);
  } else {  // compare tile: a wave per task, handed out from one queue over list C's windows
    const uint32_t voff = dup_slice_quad_offset(0, 0, threadIdx.x & 63u);
    const uint32_t n_tasks = dup_task_count(n_cand);
    uint32_t done = 0, refs = 0;
    for (uint32_t k = 0; tile.tail || k < quota; ++k) {
      uint32_t t = 0;
      if (voff == 0) t = atomicAdd(&dl.counters[DUP_QUEUE], 1u);
      t = __builtin_amdgcn_readfirstlane(t);
      if (t >= n_tasks) break;
      refs += dup_compare_task(content, stride, sizes, dl, t, n_cand, voff);
      ++done;
    }
    if (voff == 0 && done) {
      atomicAdd(&dl.counters[DUP_TASKS], done);
      atomicAdd(&dl.counters[DUP_REFS], refs);
    }
    if (leaves_cu) {  // its CU may hold another compare workgroup
      __syncthreads();
      if (threadIdx.x == 0) atomicSub(&dl.cu[stack_lds[0][0][1]], 1u);
    }
  }
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK)
sd_cas_dup_mixed_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                        const uint64_t* __restrict__ sizes, uint64_t* __restrict__ keys,
                        RegionOut ro, DupLists dl) {
  dup_mixed_kernel_body<SAMPLED_BLOCK>(content, stride, sizes, keys, ro, dl);
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK_NARROW)
sd_cas_dup_mixed_kernel_256(const uint8_t* __restrict__ content, uint64_t stride,
                            const uint64_t* __restrict__ sizes, uint64_t* __restrict__ keys,
                            RegionOut ro, DupLists dl) {
  dup_mixed_kernel_body<SAMPLED_BLOCK_NARROW>(content, stride, sizes, keys, ro, dl);
}

// The grid covers n files; the workgroups past list C's end leave at once.
extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK_NARROW)
sd_cas_dup_finish_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                         const uint64_t* __restrict__ sizes, uint64_t* __restrict__ keys,
                         RegionOut ro, DupLists dl) {
  constexpr int B = SAMPLED_BLOCK_NARROW;
  __shared__ uint32_t stack_lds[SAMPLED_DEPTH][8][B];
  const uint32_t n_cand = dl.counters[DUP_N_CAND];
#if SD_DBG
  // conservation of the main kernel's work, whichever way its workgroups got their roles
  if (blockIdx.x == 0) {
    SD_DBG_CHECK(threadIdx.x != 0 || dl.counters[DUP_TILES_RUN] == dl.counters[DUP_TILES_WANT],
                 "dup roles: %u hash tiles run of %u", dl.counters[DUP_TILES_RUN], dl.counters[DUP_TILES_WANT]);
    SD_DBG_CHECK(threadIdx.x != 0 || dl.counters[DUP_TASKS] == dup_task_count(n_cand),
                 "dup roles: %u tasks run of %u", dl.counters[DUP_TASKS], dup_task_count(n_cand));
    for (uint32_t i = threadIdx.x; i < DUP_CU_SLOTS; i += B)
      SD_DBG_CHECK(dl.cu[i] == 0, "dup roles: CU slot %u left at %u", i, dl.cu[i]);
  }
#endif
  if (blockIdx.x * B >= n_cand) return;  // (uniform)
  const uint32_t i = blockIdx.x * B + threadIdx.x;
  const bool live = i < n_cand;
  uint64_t f = 0, key = 0;
  bool ok = false;
  if (live) {
    f = dl.list_c[i];
    ok = dl.same[f] != 0;
    if (ok) key = keys[dl.cand[f]];  // written by the mixed kernel's hash tiles
  }
  const uint64_t verified = __ballot(ok), failed = __ballot(live && !ok);
  if ((threadIdx.x & 63u) == 0) {
    if (verified) atomicAdd(&dl.counters[DUP_VERIFIED], (uint32_t)__popcll(verified));
    if (failed) atomicAdd(&dl.counters[DUP_REHASHED], (uint32_t)__popcll(failed));
  }
  if (failed) {  // (wave-uniform) a probe collision in this wave: those lanes hash their file
    if (live && !ok) {
      LdsStack<B> stk{stack_lds, threadIdx.x};
      const uint4* q = reinterpret_cast<const uint4*>(content + f * stride);
      key = cas_lane_sampled<B>(q, sizes[f], stk);
    }
  }
  region_epilogue<B>(stack_lds, live, f, key, keys, ro);
}

// ---- K2: the whole-file (packed) path ------------------------------------------------
// Ragged messages of up to PACKED_MAX_CHUNKS chunks, one file per lane, lanes visited
// longest-first (on-device length sort) so a wave's lanes run the same trip counts.
// Same line-batched loads as K1 (a 128-B block pair per batch, prefetched one pair
// ahead; quads past the content are not loaded, bytes past the message are masked) and
// an LDS CV stack (per-lane depth, word-major).
// popcount(c) <= 6 pending subtrees for c <= 103 completed chunks: the bottom one (the
// largest subtree) stays in VGPRs and the other 5 live in LDS, 160 B per lane = 40 KiB per
// 256-lane block, so 4 blocks fill a CU's 160 KiB and K2 runs 4 waves per SIMD (a 6-deep
// LDS stack, 48 KiB per block, held it to 3).
constexpr int PACKED_DEPTH = 6;
constexpr int PACKED_LDS_DEPTH = PACKED_DEPTH - 1;
constexpr int PACKED_BLOCK = 256;

// The lane program is blake3_lane.hpp's lane_message<PREFIXED>: full chunks on the fixed
// 16-block schedule, only the last chunk generic.  Lanes of a wave share the chunk count (the
// visiting order is sorted on it), so the full-chunk loop is wave-uniform.
using PackedStack = CvStack<PACKED_BLOCK, true>;

// ---- K1L: chunk-parallel latency path (small batches) ---------------------------------
// A file per wave (a lane per 1 KiB chunk) or per 16-lane segment (4+ chunks per lane),
// then a level-wise pair-and-promote merge of the lanes' subtree CVs across lanes (DPP row
// shifts inside a 16-lane row: segment_merge, blake3_tree.hpp).  A file's latency is ~16 + log2(chunks) compression times
// instead of the lane-per-file kernels' 953, at ~68 % (wave per file) / ~84 % (4 files per
// wave) lane efficiency — the right trade when a batch is too small to fill the chip (the
// reference's job step is 100 files, file_identifier/mod.rs:34).  Chosen by the host below
// sd_cas_set_latency_threshold; the shape by sd_cas_set_chunkpar_split.
constexpr int CP_MAX_CHUNKS = 104;

// CV of chunk c of M = le64(size) || content[0, clen); ROOT when M is a single chunk.
__device__ __forceinline__ void cas_chunk_cv(const uint4* __restrict__ q, uint32_t clen,
                                             uint64_t size, uint32_t c, uint32_t (&cv)[8]) {
  const uint32_t nblocks = (clen + 8u + 63u) >> 6;
  const uint32_t nchunks = (clen + 8u + 1023u) >> 10;
  const bool last = (c + 1 == nchunks);
  const bool root = last && c == 0;
  const uint32_t cblocks = last ? (nblocks - 16u * c) : 16u;
  // message words [256c, 256c+2) = content words [256c-2, 256c): the size for chunk 0
  uint32_t c0 = (uint32_t)size, c1 = (uint32_t)(size >> 32);
  if (c > 0) {
    const uint4 p = q[(64u * c - 1u) * 16u < clen ? 64u * c - 1u : 0u];
    c0 = p.z;
    c1 = p.w;
  }
  uint4 A[8], B[8];
  line_clamped(q, 8u * c, clen, A);
  last_chunk<PREFIXED>(q, clen, c, cblocks, root, cv, A, B, c0, c1);
}

// K1L: a file per SEG-lane segment (64/SEG files per wave).  Segment lane l hashes the
// CPL consecutive chunks [l*CPL, (l+1)*CPL) (CPL = the smallest power of two with
// CPL*SEG >= chunks), merges them into one subtree CV through an LDS stack column of its
// own, and the segment then merges the lanes' subtree CVs across lanes.  Aligned
// power-of-two groups make this exactly BLAKE3's left-balanced tree (level-wise
// pair-and-promote, oracle formulation 3).
//   SEG = 64: one file per wave, CPL = 1 for sampled messages (57 chunks): latency ~16 + 6
//             compression times — the smallest batches;
//   SEG = 16: four files per wave, CPL = 4: 64 + 3 block/parent compressions per lane and
//             4 cross-lane levels — ~25 % fewer wave-compressions per file, 3x the latency,
//             for mid-size batches (crossovers in profiles/r01_k1l_seg_sweep.log).
constexpr int CP_DEPTH = 3;  // CPL <= 8 -> at most 3 pending subtrees per lane

template <int SEG>
__device__ __forceinline__ void chunkpar_wave(const uint8_t* __restrict__ arena,
                                              const uint64_t* __restrict__ offs, uint64_t stride,
                                              const uint32_t* __restrict__ lens, uint32_t fixed_len,
                                              const uint64_t* __restrict__ sizes, uint64_t n,
                                              const uint32_t* __restrict__ order,
                                              uint64_t* __restrict__ keys) {
  __shared__ uint32_t stack_lds[CP_DEPTH][8][64];
  const uint32_t lane = threadIdx.x;
  const uint32_t sl = lane % SEG;
  const uint64_t slot = (uint64_t)blockIdx.x * (64 / SEG) + lane / SEG;
  const uint64_t f = slot < n ? (order ? (uint64_t)order[slot] : slot) : n;
  uint32_t clen = 0, nchunks = 0;
  uint64_t size = 0;
  const uint4* q = nullptr;
  if (f < n) {
    q = reinterpret_cast<const uint4*>(arena + (offs ? offs[f] : f * stride));
    clen = offs ? lens[f] : fixed_len;
    size = sizes[f];
    nchunks = (clen + 8u + 1023u) >> 10;
  }
  const bool ok = nchunks != 0 && nchunks <= CP_MAX_CHUNKS;  // caller contract: <= 104 chunks
  uint32_t cpl = 1;
  while (cpl * SEG < nchunks) cpl <<= 1;
  const bool whole = nchunks <= cpl;  // the file fits in segment lane 0: it holds the root
  const uint32_t c0 = ok ? sl * cpl : 0u;
  const uint32_t c1 = ok ? min(nchunks, c0 + cpl) : 0u;
  uint32_t cv[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  CvStack<64, false> stk{stack_lds, lane};
  for (uint32_t c = c0; c < c1; ++c) {
    cas_chunk_cv(q, clen, size, c, cv);  // ROOT already set for a one-chunk message
    merge_push(stk, cv, c - c0 + 1u, (whole && c + 1u == nchunks) ? (uint32_t)ROOT : 0u);
  }
  // a partial (last) group: merge its pending subtrees right to left
  if (stk.sp > 0u) {
    stk.pop(cv);
    fold(stk, cv, whole ? (uint32_t)ROOT : 0u);
  }
  uint32_t count = whole ? 1u : (nchunks + cpl - 1u) / cpl;  // lane subtrees of this file
  segment_merge<SEG, 1u>(cv, sl, count);
  if (f < n && sl == 0u) keys[f] = ok ? key_of(cv) : 0ull;
}

// offs == nullptr: content i at arena + i*stride with length fixed_len (the sampled
// layout); else arena + offs[i], lens[i] bytes.  One 64-lane workgroup = 64/SEG files,
// visited in `order` (nullptr = identity): ragged files sorted by chunk count so the 4
// files of a 16-lane-segment wave share one chunks-per-lane class.
template <int SEG>
__global__ void __launch_bounds__(64)
sd_cas_chunkpar_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                       uint64_t stride, const uint32_t* __restrict__ lens, uint32_t fixed_len,
                       const uint64_t* __restrict__ sizes, uint64_t n,
                       const uint32_t* __restrict__ order, uint64_t* __restrict__ keys) {
  chunkpar_wave<SEG>(arena, offs, stride, lens, fixed_len, sizes, n, order, keys);
}

// K2: whole-file path, content length <= MAX_PACKED_CONTENT_LEN, files visited in `order`.
extern "C" __global__ void __launch_bounds__(PACKED_BLOCK)
sd_cas_packed_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                     const uint32_t* __restrict__ lens, const uint64_t* __restrict__ sizes,
                     const uint32_t* __restrict__ order, uint64_t n,
                     uint64_t* __restrict__ keys) {
  __shared__ uint32_t stack_lds[PACKED_LDS_DEPTH][8][PACKED_BLOCK];
  const uint64_t t = (uint64_t)blockIdx.x * PACKED_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint32_t f = order ? order[t] : (uint32_t)t;
  const uint4* q = reinterpret_cast<const uint4*>(arena + offs[f]);
  PackedStack stk{stack_lds, threadIdx.x};
  uint32_t cv[8];
  lane_message<PREFIXED>(q, lens[f], sizes[f], stk, cv);
  keys[f] = key_of(cv);
}

SD_DBG_ACCESSOR(sd_dbg_violations_cas_hash)

}  // namespace sdcas

// ---- host launchers ----------------------------------------------------------------
namespace sdcas {

// Sort key for the K2 visiting order: (window of LEN_WINDOW consecutive files, descending
// block count).  Inside a window the lanes of a wave get (nearly) equal trip counts; the
// window keeps a wave's 64 lanes inside ~LEN_WINDOW files of the arena instead of spread
// over all of it (a global length sort scattered every wave over the whole arena and
// thrashed address translation: 4x slower on 1M files / 51 GB).
// Visiting order = STABLE sort on the descending exact BLAKE3 chunk count of the message
// (ceil((len + 8) / 1024)): the longest messages start first (no tail of late long waves),
// the lanes of a wave share the chunk count (so K2's full-chunk loop is wave-uniform and
// only the last chunk runs the generic per-block code) and, the sort being stable, the
// files of one bucket keep their arena order, so a wave's 64 lanes stay close in memory.
// Measured on 1M ragged files (profiles/r01_k2_order.txt): exact-length global sort 41 ms,
// per-window exact sort 31.7 ms, chunk buckets 17.4 ms.
// SD_K2_BLOCK_KEY=1 keys on the exact 64-B BLOCK count instead, so a wave's lanes would also
// share the last chunk's block count — measured 2.5x SLOWER (1M files: 41.2 vs 16.8 ms,
// profiles/r04_ab_keys.log): 1,664 block buckets of ~600 files spread each wave's 64 lanes over
// the whole 51 GB arena (the address-translation thrash of a global length sort), where ~104
// chunk buckets keep them within ~330 MB.  Off.
#ifndef SD_K2_BLOCK_KEY
#define SD_K2_BLOCK_KEY 0
#endif
// SD_K2_KEY_SHIFT = s: key on chunks >> s (buckets of 2^s chunk counts: a wave's lanes may
// differ by up to 2^s - 1 chunks, but a bucket's files lie 2^s times closer in the arena) —
// measured monotonically slower, 1M files 16.95 / 17.05 / 17.3 / 17.9 ms for s = 0..3
// (profiles/r04_ab_k2_keyshift.log): the lanes' balance matters, the arena distance does not
#ifndef SD_K2_KEY_SHIFT
#define SD_K2_KEY_SHIFT 0
#endif
constexpr uint32_t CHUNK_KEY_BITS = SD_K2_BLOCK_KEY ? 11 : 7;  // blocks <= 1,664 / chunks <= 104

extern "C" __global__ void __launch_bounds__(256)
sd_cas_length_keys(const uint32_t* __restrict__ lens, uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint64_t units = SD_K2_BLOCK_KEY ? ((uint64_t)lens[i] + 8u + 63u) >> 6
                                           : ((uint64_t)lens[i] + 8u + 1023u) >> (10 + SD_K2_KEY_SHIFT);
    out[i] = ((1ull << CHUNK_KEY_BITS) - 1) - units;
  }
}

int length_key_bits(uint64_t) { return (int)CHUNK_KEY_BITS; }

hipError_t hash_sampled(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                        uint64_t n, uint64_t* keys, hipStream_t s, uint32_t cus) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
  // One file per lane at 4 waves per SIMD: the 512-lane grid fills the chip in rounds of
  // two quanta (one workgroup per CU per round), the 256-lane grid in rounds of one.  The
  // wide grid is 1-2 % faster per file (profiles/r01_k1_block_ab.log) but an odd number of
  // quantum rounds leaves half its last round's SIMDs idle (3 quanta: 4.96 vs ~3.5 ms), so
  // it runs only when the batch spans an even number of quanta.
  const uint64_t quanta = cus ? (n + (uint64_t)cus * 256 - 1) / ((uint64_t)cus * 256) : 0;
  if (cus && (blocks < cus || (quanta & 1))) {
    const uint64_t nb = (n + SAMPLED_BLOCK_NARROW - 1) / SAMPLED_BLOCK_NARROW;
    sd_cas_sampled_kernel_256<<<(uint32_t)nb, SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride, sizes,
                                                                           n, keys);
  } else {
    sd_cas_sampled_kernel<<<(uint32_t)blocks, SAMPLED_BLOCK, 0, s>>>(content, stride, sizes, n, keys);
  }
  return hipGetLastError();
}

hipError_t hash_sampled_regions(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                                uint64_t n, uint64_t* keys, uint32_t* rep, uint64_t* rkeys,
                                uint32_t* rfile, uint32_t* cursor, uint64_t cap, uint64_t* spill_keys,
                                uint32_t* spill_file, uint32_t* overflow, uint64_t* objects,
                                hipStream_t s, uint32_t cus) {
  if (n == 0) return hipSuccess;
  const RegionOut ro{rkeys, rfile, cursor, cap, spill_keys, spill_file, rep, overflow,
                     (unsigned long long*)objects};
  const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
  const uint64_t quanta = cus ? (n + (uint64_t)cus * 256 - 1) / ((uint64_t)cus * 256) : 0;
  if (cus && (blocks < cus || (quanta & 1))) {  // the grid choice of hash_sampled
    const uint64_t nb = (n + SAMPLED_BLOCK_NARROW - 1) / SAMPLED_BLOCK_NARROW;
    sd_cas_sampled_group_kernel_256<<<(uint32_t)nb, SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride,
                                                                                 sizes, n, keys, ro);
  } else {
    sd_cas_sampled_group_kernel<<<(uint32_t)blocks, SAMPLED_BLOCK, 0, s>>>(content, stride, sizes, n,
                                                                          keys, ro);
  }
  return hipGetLastError();
}

DupVerifyWs dup_verify_layout(void* ws, uint64_t n) {
  WsCarve w(ws);  DupVerifyWs L;
  L.probes = w.take<uint64_t>(n);  L.cand = w.take<uint32_t>(n);
  L.list_h = w.take<uint32_t>(n);  L.list_c = w.take<uint32_t>(n);  L.same = w.take<uint32_t>(n);
  L.cnt = w.take<uint32_t>(n);  L.first = w.take<uint32_t>(n);  L.rank = w.take<uint32_t>(n);
  L.partial = w.take<uint32_t>(n / 4096 + 1);  // exclusive_scan_u32's scratch
  L.counters = w.take<uint32_t>(DUP_COUNTERS);  L.cu = w.take<uint32_t>(DUP_CU_SLOTS);
  L.objects = w.take<uint64_t>(1);
  L.bytes = w.bytes();  return L;
}
size_t dup_verify_workspace_bytes(uint64_t n) { return dup_verify_layout(nullptr, n).bytes; }

// tail compare tiles = slots x NUM / DEN (hash_sampled_regions_verify; a build-time knob for the sweep)
#ifndef SD_DUP_TAIL_NUM
#define SD_DUP_TAIL_NUM 5u
#define SD_DUP_TAIL_DEN 7u
#endif

hipError_t dup_candidates(const uint8_t* content, uint64_t stride, const uint64_t* sizes, uint64_t n,
                          const DupVerifyWs& L, void* group_ws, uint32_t* totals, hipStream_t s) {
  if (n == 0) return hipSuccess;
  sd_dup_probe_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(content, stride, sizes, n, L.probes,
                                                                  L.counters, L.cu, L.cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hash_group_min(L.probes, nullptr, n, L.cand, L.objects, group_ws, totals, s);
}

hipError_t hash_sampled_regions_verify(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                                       uint64_t n, uint64_t* keys, uint32_t* rep, uint64_t* rkeys,
                                       uint32_t* rfile, uint32_t* cursor, uint64_t cap,
                                       uint64_t* spill_keys, uint32_t* spill_file, uint32_t* overflow,
                                       uint64_t* objects, const DupVerifyWs& L, uint32_t* note,
                                       uint32_t seq, hipStream_t s, uint32_t cus, bool cu_roles) {
  if (n == 0) return hipSuccess;
  const RegionOut ro{rkeys, rfile, cursor, cap, spill_keys, spill_file, rep, overflow,
                     (unsigned long long*)objects};
  const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
  const uint64_t quanta = cus ? (n + (uint64_t)cus * 256 - 1) / ((uint64_t)cus * 256) : 0;
  // static placement: the grid choice of hash_sampled.  Run-time roles (sd_dup_runs.h): 256-lane
  // workgroups for every batch shape, so a compare workgroup is one wave on each SIMD of its CU
  const bool narrow = cu_roles || (cus && (blocks < cus || (quanta & 1)));
  // Static placement's tail compare tiles: the last round of hash tiles frees the chip's workgroup
  // slots one by one over a tile's time, half the slots x that time in all, and a compare tile of B pairs
  // took ~0.7 of a hash tile's time beside hash tiles (profiles/dup_verify/): slots / 2 / 0.7.
  // A tile of B entries in runs reads ~0.8 of the rows a tile of B pairs did, which would put
  // the count near 0.9 slots; the sweep on the run kernel (profiles/dup_groups/: 1 / 192 / 365 /
  // 448 / 512 / all 768 tail tiles: 22.55 / 21.3 / 20.9 / 21.15 / 20.75 / 22.55 ms) is flat from
  // 365 to 512 within the process-to-process spread, so 5/7 stays.
  const uint32_t slots = (cus ? cus : 256u) * (narrow ? 4u : 2u);
  const uint32_t tail_tiles = cu_roles ? 0u : slots * SD_DUP_TAIL_NUM / SD_DUP_TAIL_DEN;  // (static: >= 1)
  const DupLists dl{L.cand, L.list_h, L.list_c, L.same, L.cnt, L.first, L.rank, L.counters, L.cu,
                    tail_tiles, slots, note, seq, (uint32_t)n};
  const uint32_t nb256 = (uint32_t)((n + 255) / 256);
  sd_dup_compact_kernel<<<nb256, 256, 0, s>>>(n, dl);
  hipError_t e = exclusive_scan_u32(L.cnt, L.first, n, L.partial, s);
  if (e != hipSuccess) return e;
  sd_dup_order_kernel<<<nb256, 256, 0, s>>>(n, dl);
  if (narrow) {
    static_assert(SAMPLED_BLOCK_NARROW == (int)DUP_ROLE_BLOCK, "dup_role_grid is this grid");
    sd_cas_dup_mixed_kernel_256<<<dup_role_grid(n), SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride, sizes,
                                                                                 keys, ro, dl);
  } else {
    sd_cas_dup_mixed_kernel<<<(uint32_t)blocks + 1, SAMPLED_BLOCK, 0, s>>>(content, stride, sizes, keys,
                                                                          ro, dl);
  }
  const uint64_t fb = (n + SAMPLED_BLOCK_NARROW - 1) / SAMPLED_BLOCK_NARROW;
  sd_cas_dup_finish_kernel<<<(uint32_t)fb, SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride, sizes, keys,
                                                                        ro, dl);
  return hipGetLastError();
}

// A copy of pinned host memory into HBM by the shader instead of the SDMA engine (the
// path gather's streamed pieces: A/B SD_PATHS_PULL): each lane moves 16-B quads, a wave
// 1 KiB per load instruction over the host link, U quads per lane in flight.  Measured one
// piece at a time (tools/ubench_pull.hip, profiles/r04_ubench_pull.log): a 128 KiB piece
// 7.8 us with U = 1 (32 workgroups) vs 11.3 with U = 4 (8 workgroups: too few CUs issue);
// from 1 MiB on U = 4 wins (1 MiB 25.2 vs 29.0 us, 4 MiB 85.7 vs 102.6); SDMA 18 / 34 / 91 us.
// So pieces under SD_PULL_WIDE_BYTES take U = 1, larger ones SD_PULL_UNROLL.
#ifndef SD_PULL_UNROLL
#define SD_PULL_UNROLL 4  // 4 vs 1 for every piece: 100 sampled files 0.29 -> 0.26 ms
                          // (profiles/r04_ab_jobstep_pull.log)
#endif
#ifndef SD_PULL_WIDE_BYTES
#define SD_PULL_WIDE_BYTES (512u << 10)
#endif
template <int U>
__global__ void __launch_bounds__(256)
sd_pull_host(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t quads) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += step * U) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * step < quads) v[u] = src[i + u * step];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * step < quads) dst[i + u * step] = v[u];
  }
}

hipError_t pull_host(void* dst, const void* src, uint64_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  if ((bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15))
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  const uint64_t quads = bytes >> 4;
  const int u = bytes < SD_PULL_WIDE_BYTES ? 1 : SD_PULL_UNROLL;
  uint64_t blocks = (quads + 256 * u - 1) / (256 * u);
  if (blocks > 2048) blocks = 2048;
  if (u == 1)
    sd_pull_host<1><<<(uint32_t)blocks, 256, 0, s>>>((const uint4*)src, (uint4*)dst, quads);
  else
    sd_pull_host<SD_PULL_UNROLL><<<(uint32_t)blocks, 256, 0, s>>>((const uint4*)src, (uint4*)dst, quads);
  return hipGetLastError();
}

hipError_t hash_packed(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                       const uint64_t* sizes, const uint32_t* order, uint64_t n, uint64_t* keys,
                       hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  sd_cas_packed_kernel<<<(uint32_t)blocks, 256, 0, s>>>(arena, offs, lens, sizes, order, n, keys);
  return hipGetLastError();
}

hipError_t hash_chunkpar(const uint8_t* arena, const uint64_t* offs, uint64_t stride,
                         const uint32_t* lens, uint32_t fixed_len, const uint64_t* sizes,
                         uint64_t n, uint64_t* keys, int seg, hipStream_t s,
                         const uint32_t* order) {
  if (n == 0) return hipSuccess;
  if (n >= (1ull << 31)) return hipErrorInvalidValue;
  if (seg == 16)
    sd_cas_chunkpar_kernel<16><<<(uint32_t)((n + 3) / 4), 64, 0, s>>>(
        arena, offs, stride, lens, fixed_len, sizes, n, order, keys);
  else
    sd_cas_chunkpar_kernel<64><<<(uint32_t)n, 64, 0, s>>>(arena, offs, stride, lens, fixed_len,
                                                         sizes, n, order, keys);
  return hipGetLastError();
}

hipError_t length_keys(const uint32_t* lens, uint64_t n, uint64_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  sd_cas_length_keys<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(lens, n, out);
  return hipGetLastError();
}

}  // namespace sdcas
