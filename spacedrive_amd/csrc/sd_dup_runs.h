// sd_dup_runs.h — the index arithmetic of K1V's compare tasks (dup_verify.hip).  Plain arithmetic,
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

// ---- roles taken at run time (SD_CAS_DUP_PLACEMENT=cu) --------------------------------------
// The grid is dup_role_grid(n) workgroups of DUP_ROLE_BLOCK lanes, so a compare workgroup is one
// wave on each SIMD of its CU.  Lane 0 of a workgroup decides its role when it starts:
//   compare  it takes dup_role_wave_tasks() tasks per wave and leaves (dup_compare_has_quota: any
//            number when the whole grid is resident at once).  Only while the task queue
//            still has tasks, its CU holds fewer than DUP_CU_LIMIT compare workgroups (a table of
//            DUP_CU_SLOTS counters indexed by dup_cu_slot), the compares are not ahead of the
//            hashing (dup_compares_not_ahead, from relaxed reads of the two queue counters) and
//            fewer than dup_compare_budget() workgroups have taken this role;
//   hash     otherwise: the next tile of list H from the hash queue;
//   drain    no hash tile is left: it takes tasks until the task queue is empty.
// Every hash tile is taken whatever the arrival order and whatever the relaxed reads return: at
// most G - TH workgroups leave without asking the hash queue, so at least TH ask it.  Every task is
// taken: if all G - TH compare workgroups ran, their quotas cover list C (TH + ceil(n_cand / B) <=
// G), and if fewer did, more than TH workgroups asked the hash queue and the ones past its end
// drain the task queue.  tests/native/dup_roles_test.cpp replays this for shuffled orders.
constexpr uint32_t DUP_ROLE_BLOCK = 256;
// Swept on the 30 %-duplicate bench (profiles/dup_roles/limit_quota_sweep.txt; the static map 20.8
// ms per call): LIMIT = 1 / 2 / none at a quota of one tile's worth 19.5 / 21.8 / 23.6 ms, at two
// tiles' worth 20.6 / 22.5 / 23.8.
#ifndef SD_DUP_CU_LIMIT
#define SD_DUP_CU_LIMIT 1  // compare workgroups per CU; 0: no per-CU limit (the progress rule alone)
#endif
#ifndef SD_DUP_QUOTA_MUL
#define SD_DUP_QUOTA_MUL 1  // a compare workgroup's quota in tiles' worth of entries
#endif
constexpr uint32_t DUP_CU_LIMIT = SD_DUP_CU_LIMIT;
constexpr uint32_t DUP_QUOTA_MUL = SD_DUP_QUOTA_MUL;
static_assert(DUP_QUOTA_MUL >= 1, "a compare workgroup covers at least one tile's worth of list C");

// XCC_ID is bits [3:0] of HW_REG_XCC_ID; SE_ID, SH_ID and CU_ID are bits [15:8] of HW_REG_HW_ID
constexpr uint32_t DUP_CU_SLOTS = 16u * 256u;
SD_RUNS_HD inline uint32_t dup_cu_slot(uint32_t xcc_id_reg, uint32_t hw_id_reg) {
  return ((xcc_id_reg & 15u) << 8) | ((hw_id_reg >> 8) & 255u);
}
SD_RUNS_HD inline uint32_t dup_role_grid(uint64_t n) {
  return (uint32_t)((n + DUP_ROLE_BLOCK - 1) / DUP_ROLE_BLOCK) + 1u;
}
SD_RUNS_HD inline uint32_t dup_role_hash_tiles(uint32_t n_hash) {
  return n_hash / DUP_ROLE_BLOCK + (n_hash % DUP_ROLE_BLOCK ? 1u : 0u);
}
SD_RUNS_HD inline uint32_t dup_role_wave_tasks(void) { return dup_tile_wave_tasks() * DUP_QUOTA_MUL; }
// A compare workgroup leaves after its quota so that the workgroup dispatched into its place can
// hash beside the CU's next compare workgroup.  When the chip holds the whole grid at once (G <=
// slots) nobody waits for its place, and fixed quotas would only leave the waves with the cheap
// tasks idle while the others finish: it then takes tasks until the queue is empty.
SD_RUNS_HD inline bool dup_compare_has_quota(uint32_t G, uint32_t slots) { return G > slots; }
// Which placement a grid of G workgroups takes by default, on a chip that holds `slots` of them at
// once.  The first `slots` workgroups all start within a microsecond and decide from counters that
// still read zero, so their roles fall as the arrival order has it, and a CU that draws more hash
// tiles than its neighbours sets the kernel's time (one hashing wave saturates its SIMD): the
// static map deals a resident grid evenly.  Swept from 1 to 20 quanta at 10 % and 30 % duplicates
// (profiles/dup_roles/size_sweep.txt): run-time roles take 1.4-1.8x the static map's time at 1-2
// quanta, 0.83-1.33x from 3 to 10, and 0.92-1.00x from 12 (three rounds of the chip) on.
constexpr uint32_t DUP_ROLES_MIN_ROUNDS = 3;
SD_RUNS_HD inline bool dup_roles_pay(uint32_t G, uint32_t slots) {
  return (uint64_t)G >= (uint64_t)DUP_ROLES_MIN_ROUNDS * slots;
}
// workgroups that may take the compare role (G >= TH: n_hash <= n)
SD_RUNS_HD inline uint32_t dup_compare_budget(uint32_t G, uint32_t TH) { return G - TH; }
// tasks_taken / tasks_total <= tiles_taken / tiles_total, cross-multiplied (both products < 2^64)
SD_RUNS_HD inline bool dup_compares_not_ahead(uint32_t tasks_taken, uint32_t tasks_total,
                                              uint32_t tiles_taken, uint32_t tiles_total) {
  return (uint64_t)tasks_taken * tiles_total <= (uint64_t)tiles_taken * tasks_total;
}
// Does a starting workgroup ask for the compare role?  task_queue and hash_queue are the queue
// counters as read (they run past their totals once the queues are empty).
SD_RUNS_HD inline bool dup_wants_compare(uint32_t task_queue, uint32_t tasks_total, uint32_t hash_queue,
                                         uint32_t tiles_total) {
  if (task_queue >= tasks_total) return false;
  const uint32_t tiles_taken = hash_queue < tiles_total ? hash_queue : tiles_total;
  return dup_compares_not_ahead(task_queue, tasks_total, tiles_taken, tiles_total);
}
// cu_compare: the CU's counter before the workgroup's own increment
SD_RUNS_HD inline bool dup_cu_has_room(uint32_t cu_compare) { return DUP_CU_LIMIT == 0 || cu_compare < DUP_CU_LIMIT; }
// a workgroup's role as one word (broadcast through LDS): a hash tile, or one of the two below
constexpr uint32_t DUP_ROLE_COMPARE = 0x80000000u, DUP_ROLE_DRAIN = 0xC0000000u;

// byte offset in a row of lane `lane`'s quad u of slice s: consecutive lanes read consecutive
// quads (1 KiB per load instruction); the largest is 57,344 - 16
SD_RUNS_HD inline uint32_t dup_slice_quad_offset(uint32_t s, uint32_t u, uint32_t lane) {
  return s * DUP_SLICE_BYTES + (u * DUP_WAVE + lane) * 16u;
}

}  // namespace sdcas
