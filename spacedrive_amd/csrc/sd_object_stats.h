// sd_object_stats.h — launchers of the Object statistics kernels (object_stats.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

// The eight totals (the same indices as SD_CAS_STAT_* of include/sd_hip_cas.h).
constexpr int STAT_ROWS = 0, STAT_OBJECTS = 1, STAT_TOTAL_BYTES = 2, STAT_UNIQUE_BYTES = 3,
              STAT_DUPLICATE_SETS = 4, STAT_MAX_COPIES = 5, STAT_SIZE_MISMATCH_ROWS = 6,
              STAT_BAD_ROWS = 7, STAT_COUNT = 8;

// copies[i] and totals[STAT_COUNT] of a grouping `rep` (rep[i] = the first row with row i's
// key) and the rows' sizes.  state: NULL, or per row SD_LINKS_* — a row that is not HASHED
// takes no part (copies 0, counted nowhere).  A row with rep[i] > i or rep[rep[i]] != rep[i]
// is bad: counted in STAT_BAD_ROWS only, never used as an index.  copies is accumulator and
// output; shards: stats_shard_bytes() of scratch.  n < 2^32, n > 0.
size_t stats_shard_bytes();
hipError_t object_stats(const uint32_t* rep, const uint64_t* sizes, const uint8_t* state, uint64_t n,
                        uint32_t* copies, uint64_t* totals, uint64_t* shards, hipStream_t s);

// The top list's candidate selection.  A tile is TOP_TILE rows (one workgroup); the stable
// compaction keeps row order inside and across tiles.
constexpr uint32_t TOP_THREADS = 1024, TOP_ITEMS = 16;
constexpr uint64_t TOP_TILE = (uint64_t)TOP_THREADS * TOP_ITEMS;  // 16,384 (cas.py: TOP_TILE)
constexpr uint32_t TOP_BINS = 65;  // bin = waste ? 64 - clz(waste) : 0
constexpr int TOP_SEL_T = 0, TOP_SEL_TOP = 1, TOP_SEL_SETS = 2, TOP_SEL_M = 3, TOP_SEL_WORDS = 4;
size_t top_tiles(uint64_t n);
size_t top_scan_bytes(uint64_t n);
// hist[TOP_BINS] (u64) over the heads with copies >= 2; sel[TOP_SEL_T] = the highest bin t
// with sum_{b >= t} hist[b] >= k (0 when fewer than k sets), sel[TOP_SEL_TOP] = the highest
// non-empty bin, sel[TOP_SEL_SETS] = the number of sets; scan (top_scan_bytes(n)) = the
// tiles' counts and offsets among the heads with bin >= t, sel[TOP_SEL_M] = their number.
// k > 0, n > 0.
hipError_t top_select(const uint32_t* rep, const uint64_t* sizes, const uint32_t* copies, uint64_t n,
                      uint64_t k, uint64_t* hist, uint64_t* sel, uint32_t* scan, hipStream_t s);
// the candidates in row order: ckeys = ~waste, cvals = head (sel, scan as top_select left them)
hipError_t top_emit(const uint32_t* rep, const uint64_t* sizes, const uint32_t* copies, uint64_t n,
                    const uint64_t* sel, const uint32_t* scan, uint64_t* ckeys, uint32_t* cvals,
                    hipStream_t s);
// heads[j], waste[j] = (svals[j], ~skeys[j]) for j < found, (SD_LINKS_NO_OBJECT, 0) for
// found <= j < k
hipError_t top_write(const uint64_t* skeys, const uint32_t* svals, uint64_t found, uint64_t k,
                     uint32_t* heads, uint64_t* waste, hipStream_t s);

}  // namespace sdcas
