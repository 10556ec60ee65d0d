// object_stats.hip — what a grouping is worth, on gfx950: copies per Object, the library's
// bytes without duplicates, and the duplicate sets that waste the most space.
//
// The reference keeps the slot and leaves it empty: core/src/library/statistics.rs:42,46
// writes total_object_count = 0 and total_unique_bytes = "0" into the `statistics` row
// (core/prisma/schema.prisma:83,87).  Both are pure functions of two arrays this library
// already holds in HBM — rep (the grouping: rep[i] = the first row with row i's key) and
// sizes (the le64(size) prefix K1 hashes) — so they are computed here in a few elementwise
// passes.  Integer work bound by HBM and, for the counts, by same-address atomics; every byte
// sum is u64 (mod 2^64), nothing is a float.
//
//   head       a row with rep[i] == i: one Object
//   valid row  rep[i] <= i and rep[rep[i]] == rep[i]; any other row is BAD: it is counted in
//              STAT_BAD_ROWS only and its rep is never used as an index (rep[i] <= i < n is
//              tested first)
//   copies[i]  the number of valid rows of row i's set (every member carries it), 0 if bad
//   waste(h)   (copies[h] - 1) * sizes[h]
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_debug.h"
#include "sd_group.h"
#include "sd_links.h"
#include "sd_object_stats.h"

namespace sdcas {

__device__ __forceinline__ bool stat_row(const uint8_t* state, uint64_t i) {
  return !state || state[i] == SD_LINKS_HASHED;
}

// ---- count -----------------------------------------------------------------------------
// The caller's copies array is accumulator and output.  Pass 1: copies[i] = 1 for a valid row,
// 0 for a bad (or not hashed) one; workgroup 0 also zeroes the totals' shards.
constexpr int CNT_THREADS = 256;
// totals shards: STAT_SHARDS lines of 128 B (16 u64), workgroup b adds into shard b %
// STAT_SHARDS — the pattern of group_hash.hip's Object count (one device counter serialises
// at ~12.8 ns per atomic).  Word STAT_COUNT of a line is the debug build's conservation sum.
constexpr uint32_t STAT_SHARDS = 64, STAT_STRIDE = 16;
constexpr int STAT_SLOTS = STAT_COUNT + 1;

extern "C" __global__ void __launch_bounds__(CNT_THREADS)
sd_stats_init(const uint32_t* __restrict__ rep, const uint8_t* __restrict__ state, uint64_t n,
              uint32_t* __restrict__ copies, unsigned long long* __restrict__ shards) {
  if (blockIdx.x == 0)
    for (uint32_t k = threadIdx.x; k < STAT_SHARDS * STAT_STRIDE; k += CNT_THREADS) shards[k] = 0ull;
  const uint64_t i = (uint64_t)blockIdx.x * CNT_THREADS + threadIdx.x;
  if (i >= n) return;
  bool valid = false;
  if (stat_row(state, i)) {
    const uint32_t r = rep[i];
    if (r <= i) valid = r == i || rep[r] == r;
  }
  copies[i] = valid ? 1u : 0u;
}

// Pass 2: every valid non-head row adds 1 to its head's entry.  A non-head's own entry is
// stable here (adds only reach heads), so copies[i] != 0 is its validity — no second gather
// through rep.  The adds are combined per wave before they reach memory: the first pending
// lane's head is broadcast and compared (one ballot), its lanes leave with ONE atomic of the
// ballot's popcount; a wave whose rows share one head (a hot key) is done after that step.
// CNT_PEEL such leaders are peeled, then the remaining lanes add 1 each (distinct small sets,
// where the atomics spread over many addresses).  Unaggregated, a 1.31 M-row hot key would be
// 1.31 M atomics on one address (~17 ms at 12.8 ns); per wave it is 20,480 (~0.26 ms).
constexpr int CNT_PEEL = 4;
extern "C" __global__ void __launch_bounds__(CNT_THREADS)
sd_stats_count(const uint32_t* __restrict__ rep, uint64_t n, uint32_t* __restrict__ copies) {
  const uint64_t i = (uint64_t)blockIdx.x * CNT_THREADS + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t r = 0;
  bool active = false;
  if (i < n) {
    r = rep[i];
    active = r != (uint32_t)i && copies[i] != 0u;  // a head's entry is never read here
  }
  uint64_t todo = __ballot(active);
  for (int p = 0; p < CNT_PEEL && todo; ++p) {
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
    const uint32_t h = __shfl(r, (int)leader, 64);
    const uint64_t same = __ballot(active && r == h);
    if (lane == leader) atomicAdd(&copies[h], (uint32_t)__popcll(same));
    todo &= ~same;
    if (r == h) active = false;
  }
  if (active) atomicAdd(&copies[r], 1u);
}

// ---- finalize --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t lo = __shfl_down((uint32_t)x, d, 64), hi = __shfl_down((uint32_t)(x >> 32), d, 64);
    x += ((uint64_t)hi << 32) | lo;
  }
  return x;  // lane 0
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t y = __shfl_down(x, d, 64);
    x = y > x ? y : x;
  }
  return x;  // lane 0
}

// One pass over the rows: a non-head takes its head's count as its own (nobody else reads a
// non-head's entry and a head's entry is final, so in place is safe) and compares its size
// with its head's; every row feeds the totals — per thread over FIN_ITEMS rows, per wave by
// shuffles, per workgroup through LDS, then one atomic per total into the workgroup's shard.
constexpr int FIN_THREADS = 256, FIN_ITEMS = 8, FIN_WAVES = FIN_THREADS / 64;
constexpr uint64_t FIN_ROWS = (uint64_t)FIN_THREADS * FIN_ITEMS;
extern "C" __global__ void __launch_bounds__(FIN_THREADS)
sd_stats_finalize(const uint32_t* __restrict__ rep, const uint64_t* __restrict__ sizes,
                  const uint8_t* __restrict__ state, uint64_t n, uint32_t* copies,
                  unsigned long long* __restrict__ shards) {
  __shared__ uint64_t part[FIN_WAVES][STAT_SLOTS];
  uint64_t v[STAT_SLOTS];
#pragma unroll
  for (int k = 0; k < STAT_SLOTS; ++k) v[k] = 0;
  uint32_t mx = 0;
#pragma unroll
  for (int u = 0; u < FIN_ITEMS; ++u) {
    const uint64_t i = blockIdx.x * FIN_ROWS + (uint64_t)u * FIN_THREADS + threadIdx.x;
    if (i >= n || !stat_row(state, i)) continue;
    const uint32_t c = copies[i];
    if (c == 0u) {  // bad: rep[i] is not looked at again
      v[STAT_BAD_ROWS] += 1;
      continue;
    }
    const uint32_t r = rep[i];
    const uint64_t sz = sizes[i];
    v[STAT_ROWS] += 1;
    v[STAT_TOTAL_BYTES] += sz;
    if (r == (uint32_t)i) {
      v[STAT_OBJECTS] += 1;
      v[STAT_UNIQUE_BYTES] += sz;
      v[STAT_DUPLICATE_SETS] += c >= 2u ? 1 : 0;
      mx = c > mx ? c : mx;
      v[STAT_COUNT] += c;
    } else {
      copies[i] = copies[r];
      v[STAT_SIZE_MISMATCH_ROWS] += sizes[r] != sz ? 1 : 0;
    }
  }
  v[STAT_MAX_COPIES] = wave_max32(mx);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < STAT_SLOTS; ++k) {
    if (k == STAT_MAX_COPIES) continue;
    if (!SD_DBG && k == STAT_COUNT) continue;
    v[k] = wave_sum64(v[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < STAT_SLOTS; ++k) part[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < STAT_SLOTS) {
    const uint32_t k = threadIdx.x;
    uint64_t x = part[0][k];
    for (int q = 1; q < FIN_WAVES; ++q) {
      const uint64_t y = part[q][k];
      x = k == STAT_MAX_COPIES ? (y > x ? y : x) : x + y;
    }
    unsigned long long* dst = shards + (blockIdx.x % STAT_SHARDS) * STAT_STRIDE + k;
    if (x) {
      if (k == STAT_MAX_COPIES) atomicMax(dst, (unsigned long long)x);
      else atomicAdd(dst, (unsigned long long)x);
    }
  }
}

// one wave: totals[k] = the shards' sum (STAT_MAX_COPIES: their maximum)
extern "C" __global__ void __launch_bounds__(64)
sd_stats_fold(const unsigned long long* __restrict__ shards, uint64_t* __restrict__ totals) {
  uint64_t rows = 0;
  for (int k = 0; k < (SD_DBG ? STAT_SLOTS : STAT_COUNT); ++k) {
    uint64_t x = threadIdx.x < STAT_SHARDS ? shards[threadIdx.x * STAT_STRIDE + k] : 0ull;
    if (k == STAT_MAX_COPIES) x = wave_max32((uint32_t)x);  // copies are u32
    else x = wave_sum64(x);
    if (threadIdx.x == 0) {
      if (k == STAT_ROWS) rows = x;
      if (k < STAT_COUNT) totals[k] = x;
      // conservation: the heads' counts add up to the valid rows
      else SD_DBG_CHECK(x == rows, "object_stats: heads' copies sum to %llu, valid rows %llu",
                        (unsigned long long)x, (unsigned long long)rows);
    }
  }
  (void)rows;
}

// ---- top list: select ------------------------------------------------------------------
// The k sets with the largest waste, ties by ascending head: select, then sort.  Sorting
// every duplicate set (millions) for a list of <= 65,536 would move 12 B per set per radix
// pass; instead a 65-bin histogram of floor(log2(waste)) + 1 finds the threshold bin, a STABLE
// compaction keeps the heads at or above it (row order, so heads ascend), and the stable LSD
// sort runs over those candidates only, on the key bits that can differ.  The top path reads
// copies and sizes at heads only and never indexes through rep.
__device__ __forceinline__ bool top_set(const uint32_t* rep, const uint64_t* sizes,
                                        const uint32_t* copies, uint64_t i, uint64_t n,
                                        uint64_t* waste) {
  if (i >= n) return false;
  const uint32_t c = copies[i];
  if (c < 2u || rep[i] != (uint32_t)i) return false;
  *waste = (uint64_t)(c - 1u) * sizes[i];
  return true;
}
__device__ __forceinline__ uint32_t waste_bin(uint64_t w) {
  return w ? 64u - (uint32_t)__clzll((long long)w) : 0u;
}

extern "C" __global__ void __launch_bounds__(TOP_THREADS)
sd_top_hist(const uint32_t* __restrict__ rep, const uint64_t* __restrict__ sizes,
            const uint32_t* __restrict__ copies, uint64_t n, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t h[TOP_BINS];
  if (threadIdx.x < TOP_BINS) h[threadIdx.x] = 0u;
  __syncthreads();
  for (uint32_t u = 0; u < TOP_ITEMS; ++u) {
    const uint64_t i = blockIdx.x * TOP_TILE + (uint64_t)u * TOP_THREADS + threadIdx.x;
    uint64_t w;
    if (top_set(rep, sizes, copies, i, n, &w)) atomicAdd(&h[waste_bin(w)], 1u);
  }
  __syncthreads();
  if (threadIdx.x < TOP_BINS && h[threadIdx.x])
    atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

extern "C" __global__ void __launch_bounds__(64)
sd_top_pick(const unsigned long long* __restrict__ hist, uint64_t k, uint64_t* __restrict__ sel) {
  if (threadIdx.x) return;
  uint64_t above = 0, t = 0, top = 0;
  bool have_t = false, have_top = false;
  for (int b = (int)TOP_BINS - 1; b >= 0; --b) {
    const uint64_t x = hist[b];
    if (x && !have_top) { top = (uint64_t)b; have_top = true; }
    above += x;
    if (!have_t && above >= k) { t = (uint64_t)b; have_t = true; }
  }
  sel[TOP_SEL_T] = t;
  sel[TOP_SEL_TOP] = top;
  sel[TOP_SEL_SETS] = above;
}

__device__ __forceinline__ bool top_cand(const uint32_t* rep, const uint64_t* sizes,
                                         const uint32_t* copies, uint64_t i, uint64_t n,
                                         uint32_t t, uint64_t* waste) {
  return top_set(rep, sizes, copies, i, n, waste) && waste_bin(*waste) >= t;
}

// The stable compaction: count per tile, the tile counts' exclusive scan (group.hip's
// exclusive_scan_u32), emit at the tile's offset in row order — the pattern of links.hip's
// sd_links_pre_count / _bscan / _emit.
extern "C" __global__ void __launch_bounds__(TOP_THREADS)
sd_top_count(const uint32_t* __restrict__ rep, const uint64_t* __restrict__ sizes,
             const uint32_t* __restrict__ copies, uint64_t n, const uint64_t* __restrict__ sel,
             uint32_t* __restrict__ bcount) {
  __shared__ uint32_t wsum[TOP_THREADS / 64];
  const uint32_t t = (uint32_t)sel[TOP_SEL_T];
  uint32_t c = 0;
  for (uint32_t u = 0; u < TOP_ITEMS; ++u) {
    const uint64_t i = blockIdx.x * TOP_TILE + (uint64_t)u * TOP_THREADS + threadIdx.x;
    uint64_t w;
    c += (uint32_t)__popcll(__ballot(top_cand(rep, sizes, copies, i, n, t, &w)));
  }
  if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < TOP_THREADS / 64; ++w) s += wsum[w];
    bcount[blockIdx.x] = s;
  }
}

extern "C" __global__ void __launch_bounds__(TOP_THREADS)
sd_top_emit(const uint32_t* __restrict__ rep, const uint64_t* __restrict__ sizes,
            const uint32_t* __restrict__ copies, uint64_t n, const uint64_t* __restrict__ sel,
            const uint32_t* __restrict__ boff, uint64_t* __restrict__ ckeys,
            uint32_t* __restrict__ cvals) {
  __shared__ uint32_t wbase[TOP_ITEMS][TOP_THREADS / 64];
  const uint32_t t = (uint32_t)sel[TOP_SEL_T];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t m[TOP_ITEMS], waste[TOP_ITEMS];
  for (uint32_t u = 0; u < TOP_ITEMS; ++u) {
    const uint64_t i = blockIdx.x * TOP_TILE + (uint64_t)u * TOP_THREADS + threadIdx.x;
    waste[u] = 0;
    m[u] = __ballot(top_cand(rep, sizes, copies, i, n, t, &waste[u]));
    if (lane == 0) wbase[u][w] = (uint32_t)__popcll(m[u]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // row order = (u, wave) order: exclusive prefix in place
    uint32_t s = boff[blockIdx.x];
    for (uint32_t u = 0; u < TOP_ITEMS; ++u)
      for (uint32_t q = 0; q < TOP_THREADS / 64; ++q) {
        const uint32_t c = wbase[u][q];
        wbase[u][q] = s;
        s += c;
      }
  }
  __syncthreads();
  for (uint32_t u = 0; u < TOP_ITEMS; ++u) {
    if (!((m[u] >> lane) & 1ull)) continue;
    const uint64_t i = blockIdx.x * TOP_TILE + (uint64_t)u * TOP_THREADS + threadIdx.x;
    const uint32_t d = wbase[u][w] + (uint32_t)__popcll(m[u] & below);
    ckeys[d] = ~waste[u];  // ascending ~waste = descending waste
    cvals[d] = (uint32_t)i;
  }
}

extern "C" __global__ void __launch_bounds__(256)
sd_top_write(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ svals,
             uint64_t found, uint64_t k, uint32_t* __restrict__ heads, uint64_t* __restrict__ waste) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  heads[j] = j < found ? svals[j] : SD_LINKS_NO_OBJECT;
  waste[j] = j < found ? ~skeys[j] : 0ull;
}

// ---- launchers -------------------------------------------------------------------------
size_t stats_shard_bytes() { return (size_t)STAT_SHARDS * STAT_STRIDE * 8; }
size_t top_tiles(uint64_t n) { return (size_t)((n + TOP_TILE - 1) / TOP_TILE); }
// scan: the tiles' counts | their offsets | exclusive_scan_u32's partial sums
size_t top_scan_bytes(uint64_t n) { return (2 * top_tiles(n) + top_tiles(n) / 4096 + 1) * 4; }

hipError_t object_stats(const uint32_t* rep, const uint64_t* sizes, const uint8_t* state, uint64_t n,
                        uint32_t* copies, uint64_t* totals, uint64_t* shards, hipStream_t s) {
  if (n == 0 || n >= (1ull << 32)) return hipErrorInvalidValue;
  const uint32_t g = (uint32_t)((n + CNT_THREADS - 1) / CNT_THREADS);
  unsigned long long* sh = (unsigned long long*)shards;
  sd_stats_init<<<g, CNT_THREADS, 0, s>>>(rep, state, n, copies, sh);
  sd_stats_count<<<g, CNT_THREADS, 0, s>>>(rep, n, copies);
  sd_stats_finalize<<<(uint32_t)((n + FIN_ROWS - 1) / FIN_ROWS), FIN_THREADS, 0, s>>>(
      rep, sizes, state, n, copies, sh);
  sd_stats_fold<<<1, 64, 0, s>>>(sh, totals);
  return hipGetLastError();
}

hipError_t top_select(const uint32_t* rep, const uint64_t* sizes, const uint32_t* copies, uint64_t n,
                      uint64_t k, uint64_t* hist, uint64_t* sel, uint32_t* scan, hipStream_t s) {
  if (n == 0 || n >= (1ull << 32) || k == 0) return hipErrorInvalidValue;
  const uint32_t nb = (uint32_t)top_tiles(n);
  uint32_t *bcount = scan, *boff = scan + nb, *partial = scan + 2 * (size_t)nb;
  hipError_t e = hipMemsetAsync(hist, 0, TOP_BINS * 8, s);
  if (e != hipSuccess) return e;
  sd_top_hist<<<nb, TOP_THREADS, 0, s>>>(rep, sizes, copies, n, (unsigned long long*)hist);
  sd_top_pick<<<1, 64, 0, s>>>((const unsigned long long*)hist, k, sel);
  sd_top_count<<<nb, TOP_THREADS, 0, s>>>(rep, sizes, copies, n, sel, bcount);
  return exclusive_scan_u32(bcount, boff, nb, partial, s, (unsigned long long*)(sel + TOP_SEL_M));
}

hipError_t top_emit(const uint32_t* rep, const uint64_t* sizes, const uint32_t* copies, uint64_t n,
                    const uint64_t* sel, const uint32_t* scan, uint64_t* ckeys, uint32_t* cvals,
                    hipStream_t s) {
  if (n == 0) return hipSuccess;
  sd_top_emit<<<(uint32_t)top_tiles(n), TOP_THREADS, 0, s>>>(rep, sizes, copies, n, sel,
                                                             scan + top_tiles(n), ckeys, cvals);
  return hipGetLastError();
}

hipError_t top_write(const uint64_t* skeys, const uint32_t* svals, uint64_t found, uint64_t k,
                     uint32_t* heads, uint64_t* waste, hipStream_t s) {
  if (k == 0) return hipSuccess;
  sd_top_write<<<(uint32_t)((k + 255) / 256), 256, 0, s>>>(skeys, svals, found, k, heads, waste);
  return hipGetLastError();
}

SD_DBG_ACCESSOR(sd_dbg_violations_object_stats)

}  // namespace sdcas
