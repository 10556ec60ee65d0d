// sd_dup_runs.h — the index arithmetic of K1V's compare tasks (cas_hash.hip).  Plain arithmetic,
// host and device, so a host program checks it (tests/native/dup_runs_test.cpp).
//
// List C holds the candidates ordered by their original (cand[f]), so one original's copies are
// consecutive.  A compare task is a window of DUP_RUN_K consecutive entries of list C; inside it
// the entries of one original form a run, and the original's row is read once per run.  A row
// is DUP_SLICES slices of 8 KiB: a wave's 64 lanes hold DUP_SLICE_QUADS 16-B quads of one slice.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_RUNS_HD __host__ __device__
#else
#define SD_RUNS_HD
#endif

namespace sdcas {

// Entries per task.  A larger K re-reads fewer originals (at most F + G + D/K rows) and makes
// coarser tasks for filling the last hash round's drain.  Swept on the 30 %-duplicate bench
// (1,310,720 files, profiles/dup_groups/): K = 8 / 16 / 32 read 234,402 / 223,037 / 217,373
// reference rows for 211,767 groups and took 21.2 / 20.9 / 20.9 ms per step: 16 and 32 are
// equal within the spread, and 16 keeps the finer tasks.
#ifndef SD_DUP_RUN_K
#define SD_DUP_RUN_K 16
#endif
constexpr uint32_t DUP_RUN_K = SD_DUP_RUN_K;
static_assert(DUP_RUN_K >= 1 && DUP_RUN_K <= 32, "a task's entries are the bits of one u32");

constexpr uint32_t DUP_ROW_BYTES = 57344;     // a row's content bytes (SAMPLED_CONTENT_LEN)
constexpr uint32_t DUP_WAVE = 64;
constexpr uint32_t DUP_SLICE_QUADS = 8;       // 16-B quads per lane and slice
constexpr uint32_t DUP_SLICE_BYTES = DUP_WAVE * DUP_SLICE_QUADS * 16;  // 8 KiB
constexpr uint32_t DUP_SLICES = DUP_ROW_BYTES / DUP_SLICE_BYTES;       // 7
static_assert(DUP_SLICES * DUP_SLICE_BYTES == DUP_ROW_BYTES, "a row is whole slices");

// tasks over a list of n_cand entries
SD_RUNS_HD inline uint32_t dup_task_count(uint32_t n_cand) {
  return n_cand / DUP_RUN_K + (n_cand % DUP_RUN_K ? 1u : 0u);
}
// task t < dup_task_count(n_cand): its first entry, and how many (1..K; the last may be short)
SD_RUNS_HD inline uint32_t dup_task_first(uint32_t t) { return t * DUP_RUN_K; }  // (< 2^32: t < n / K + 1)
SD_RUNS_HD inline uint32_t dup_task_entries(uint32_t t, uint32_t n_cand) {
  const uint32_t left = n_cand - dup_task_first(t);
  return left < DUP_RUN_K ? left : DUP_RUN_K;
}

// The mixed kernel's grid is G workgroups: TH hash tiles and TC = G - TH compare tiles.  The last
// TT of them (the tail) take tasks until the queue is empty; the other TI = TC - TT lie evenly
// among the first GI = G - TT workgroups: workgroup b < GI is an interleaved compare tile where
// floor(b TI / GI) steps, and a hash tile otherwise.  c0 = interleaved tiles before b.
struct DupTile {
  bool compare, tail;
  uint32_t hash_tile;  // !compare: which tile of list H
};
SD_RUNS_HD inline DupTile dup_tile_of(uint32_t b, uint32_t G, uint32_t TH, uint32_t tail_tiles) {
  const uint32_t TC = G - TH;
  const uint32_t TT = TC < tail_tiles ? TC : tail_tiles;
  const uint32_t GI = G - TT, TI = TC - TT;
  if (b >= GI) return {true, true, 0u};
  const uint32_t c0 = (uint32_t)((uint64_t)b * TI / GI);
  const uint32_t c1 = (uint32_t)(((uint64_t)b + 1) * TI / GI);
  return {c0 != c1, false, b - c0};
}
// An interleaved tile's waves take at most this many tasks each, a tail tile's wave any number:
// one entry per lane of the tile, as a hash tile has one file per lane.
SD_RUNS_HD inline uint32_t dup_tile_wave_tasks(void) { return (DUP_WAVE + DUP_RUN_K - 1) / DUP_RUN_K; }

// byte offset in a row of lane `lane`'s quad u of slice s: consecutive lanes read consecutive
// quads (1 KiB per load instruction); the largest is 57,344 - 16
SD_RUNS_HD inline uint32_t dup_slice_quad_offset(uint32_t s, uint32_t u, uint32_t lane) {
  return s * DUP_SLICE_BYTES + (u * DUP_WAVE + lane) * 16u;
}

}  // namespace sdcas
