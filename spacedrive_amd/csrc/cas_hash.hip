// cas_hash.hip — batched generate_cas_id on gfx950: K1 (the sampled path) and K1G (K1 + the
// grouping's partition), K2 (the whole-file path), K1L (the chunk-parallel latency path), the
// shader's host copy (pull_host) and their launchers.  The sampled lane program itself is
// cas_sampled.hpp; K1V, the fused chain with duplicates verified by comparison, is dup_verify.hip.
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
#include "cas_sampled.hpp"
#include "sd_debug.h"
#include "sd_kernels.h"

namespace sdcas {

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
// (RegionOut: sd_kernels.h; the epilogue: cas_sampled.hpp)
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

// One file per lane at 4 waves per SIMD: the 512-lane grid fills the chip in rounds of
// two quanta (one workgroup per CU per round), the 256-lane grid in rounds of one.  The
// wide grid is 1-2 % faster per file (profiles/r01_k1_block_ab.log) but an odd number of
// quantum rounds leaves half its last round's SIMDs idle (3 quanta: 4.96 vs ~3.5 ms), so
// it runs only when the batch spans an even number of quanta.
bool sampled_grid_is_narrow(uint64_t n, uint32_t cus) {
  const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
  const uint64_t quanta = cus ? (n + (uint64_t)cus * 256 - 1) / ((uint64_t)cus * 256) : 0;
  return cus && (blocks < cus || (quanta & 1));
}

hipError_t hash_sampled(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                        uint64_t n, uint64_t* keys, hipStream_t s, uint32_t cus) {
  if (n == 0) return hipSuccess;
  if (sampled_grid_is_narrow(n, cus)) {
    const uint64_t nb = (n + SAMPLED_BLOCK_NARROW - 1) / SAMPLED_BLOCK_NARROW;
    sd_cas_sampled_kernel_256<<<(uint32_t)nb, SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride, sizes,
                                                                           n, keys);
  } else {
    const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
    sd_cas_sampled_kernel<<<(uint32_t)blocks, SAMPLED_BLOCK, 0, s>>>(content, stride, sizes, n, keys);
  }
  return hipGetLastError();
}

hipError_t hash_sampled_regions(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                                uint64_t n, uint64_t* keys, const RegionOut& ro, hipStream_t s,
                                uint32_t cus) {
  if (n == 0) return hipSuccess;
  if (sampled_grid_is_narrow(n, cus)) {
    const uint64_t nb = (n + SAMPLED_BLOCK_NARROW - 1) / SAMPLED_BLOCK_NARROW;
    sd_cas_sampled_group_kernel_256<<<(uint32_t)nb, SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride,
                                                                                 sizes, n, keys, ro);
  } else {
    const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
    sd_cas_sampled_group_kernel<<<(uint32_t)blocks, SAMPLED_BLOCK, 0, s>>>(content, stride, sizes, n,
                                                                          keys, ro);
  }
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
