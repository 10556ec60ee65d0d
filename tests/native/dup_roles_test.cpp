// Host test of the run-time roles of sd_dup_runs.h (a stand-alone program; tests/test_dup_roles_cpu.py
// builds it plain and with -fsanitize=address,undefined, for every per-CU limit and quota the kernel
// was swept at).  It replays the main kernel's role decisions on the CPU with the header's own
// functions: workgroups start on a chip of a few CUs in shuffled order, read the two queue counters
// late (any earlier value, as a relaxed read may return), and run their waves interleaved.  The
// hash-tile and task ledgers are heap arrays of exactly TH and n_tasks entries and the CU table a
// heap array of exactly DUP_CU_SLOTS words, so an index past either is a heap overflow the
// sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sd_dup_runs.h"

using namespace sdcas;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // uniform in [0, n), n >= 1
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((rng_state >> 33) % n);
}

struct Wg {
  uint32_t role;     // a hash tile, DUP_ROLE_COMPARE or DUP_ROLE_DRAIN
  uint32_t slot;     // its CU's slot in the table
  uint32_t cu;       // the simulated CU it holds a workgroup slot of
  uint32_t left[4];  // a compare workgroup's waves: tasks still allowed; a hash workgroup: steps left in [0]
  bool done[4];
};

// n files of which n_hash are hashed, on `cus` CUs of four workgroups each.  stale: a starting
// workgroup reads the queue counters as they were up to `stale` events ago.
static void simulate(uint32_t n, uint32_t n_hash, uint32_t cus, uint32_t stale) {
  const uint32_t n_cand = n - n_hash;
  const uint32_t G = dup_role_grid(n), TH = dup_role_hash_tiles(n_hash), n_tasks = dup_task_count(n_cand);
  CHECK(G >= TH + 1);
  CHECK((uint64_t)dup_compare_budget(G, TH) * dup_role_wave_tasks() * 4 * DUP_RUN_K >= n_cand);
  uint8_t* tile_seen = (uint8_t*)calloc(TH ? TH : 1, 1);
  uint8_t* task_seen = (uint8_t*)calloc(n_tasks ? n_tasks : 1, 1);
  uint32_t* cu = (uint32_t*)calloc(DUP_CU_SLOTS, sizeof(uint32_t));
  uint32_t task_queue = 0, hash_queue = 0, compare_wgs = 0, tasks_done = 0, tiles_done = 0;
  std::vector<uint32_t> hist_t, hist_h;  // the queue counters after every event
  std::vector<Wg> resident;
  // a CU's hardware ids: any XCC, SE, SH and CU field, other bits of both registers set at random
  std::vector<uint32_t> cu_xcc(cus), cu_hw(cus);
  for (uint32_t c = 0; c < cus; ++c) {
    cu_xcc[c] = (c & 7u) | (rnd(1u << 20) << 4);
    cu_hw[c] = (((c >> 3) & 255u) << 8) | rnd(256) | (rnd(1u << 16) << 16);
  }
  std::vector<uint32_t> free_cu;  // one entry per free workgroup slot
  for (uint32_t c = 0; c < cus; ++c)
    for (int k = 0; k < 4; ++k) free_cu.push_back(c);
  uint32_t started = 0, drains = 0, compares = 0;
  while (started < G || !resident.empty()) {
    const bool can_start = started < G && !free_cu.empty();
    if (can_start && (resident.empty() || rnd(3) == 0)) {  // the dispatcher starts a workgroup
      const uint32_t pick = rnd((uint32_t)free_cu.size());
      const uint32_t c = free_cu[pick];
      free_cu[pick] = free_cu.back();
      free_cu.pop_back();
      ++started;
      Wg w{};
      w.cu = c;
      w.slot = dup_cu_slot(cu_xcc[c], cu_hw[c]);
      CHECK(w.slot < DUP_CU_SLOTS);
      const uint32_t lag = hist_t.empty() ? 0 : rnd(stale + 1);
      const uint32_t at = hist_t.size() > lag ? (uint32_t)hist_t.size() - 1 - lag : 0;
      const uint32_t seen_t = hist_t.empty() ? 0 : hist_t[at], seen_h = hist_h.empty() ? 0 : hist_h[at];
      bool compare = dup_wants_compare(seen_t, n_tasks, seen_h, TH);
      if (compare) {  // the kernel's order: the CU's counter, then the budget, undone on a refusal
        compare = dup_cu_has_room(cu[w.slot]++) && compare_wgs++ < dup_compare_budget(G, TH);
        if (!compare) --cu[w.slot];
      }
      if (compare) {
        w.role = DUP_ROLE_COMPARE;
        ++compares;
        if (DUP_CU_LIMIT) CHECK(cu[w.slot] <= DUP_CU_LIMIT);
        for (int k = 0; k < 4; ++k) w.left[k] = dup_compare_has_quota(G, 4 * cus) ? dup_role_wave_tasks() : 0xFFFFFFFFu;
      } else {
        w.role = hash_queue++;
        if (w.role >= TH) {
          w.role = DUP_ROLE_DRAIN;
          ++drains;
          for (int k = 0; k < 4; ++k) w.left[k] = 0xFFFFFFFFu;
        } else {
          CHECK(!tile_seen[w.role]);  // every hash tile to exactly one workgroup
          tile_seen[w.role] = 1;
          w.left[0] = 1 + rnd(40);  // a hash tile is long
        }
      }
      CHECK((w.role >= DUP_ROLE_COMPARE) == (w.role == DUP_ROLE_COMPARE || w.role == DUP_ROLE_DRAIN));
      resident.push_back(w);
    } else if (!resident.empty()) {  // a resident workgroup advances by one step
      const uint32_t i = rnd((uint32_t)resident.size());
      Wg& w = resident[i];
      bool leaves = false;
      if (w.role < DUP_ROLE_COMPARE) {
        if (--w.left[0] == 0) {
          ++tiles_done;
          leaves = true;
        }
      } else {
        const uint32_t k = rnd(4);
        if (!w.done[k]) {
          if (w.left[k] == 0) {
            w.done[k] = true;
          } else {
            const uint32_t t = task_queue++;  // the wave's atomicAdd
            if (t >= n_tasks) {
              w.done[k] = true;
            } else {
              CHECK(!task_seen[t]);  // every task to exactly one wave
              task_seen[t] = 1;
              ++tasks_done;
              if (w.left[k] != 0xFFFFFFFFu) --w.left[k];
            }
          }
        }
        leaves = w.done[0] && w.done[1] && w.done[2] && w.done[3];
        if (leaves && w.role == DUP_ROLE_COMPARE) {
          CHECK(cu[w.slot] >= 1);
          --cu[w.slot];
        }
      }
      if (leaves) {
        free_cu.push_back(w.cu);
        resident[i] = resident.back();
        resident.pop_back();
      }
    }
    hist_t.push_back(task_queue);
    hist_h.push_back(hash_queue);
  }
  CHECK(tiles_done == TH && tasks_done == n_tasks);
  for (uint32_t t = 0; t < TH; ++t) CHECK(tile_seen[t]);
  for (uint32_t t = 0; t < n_tasks; ++t) CHECK(task_seen[t]);
  for (uint32_t s = 0; s < DUP_CU_SLOTS; ++s) CHECK(cu[s] == 0);
  CHECK(compares <= dup_compare_budget(G, TH));
  CHECK(compares + drains + TH == G);
  free(tile_seen);
  free(task_seen);
  free(cu);
}

int main() {
  // the progress rule: "compares are not ahead" is tasks_taken / tasks_total <= tiles_taken / tiles_total
  CHECK(dup_compares_not_ahead(0, 0, 0, 0));
  CHECK(dup_compares_not_ahead(0, 0, 5, 9));      // no tasks at all: never ahead ...
  CHECK(!dup_wants_compare(0, 0, 5, 9));          // ... and never wanted: the queue is empty
  CHECK(dup_compares_not_ahead(0, 10, 0, 0));     // no hash tiles: nothing to be ahead of
  CHECK(dup_wants_compare(3, 10, 0, 0) && dup_wants_compare(3, 10, 7, 0));
  CHECK(dup_wants_compare(0, 10, 0, 9));          // the first workgroups, both queues untouched
  CHECK(!dup_wants_compare(1, 10, 0, 9));         // one task taken, no tile yet: ahead
  CHECK(dup_wants_compare(5, 10, 5, 10) && !dup_wants_compare(6, 10, 5, 10) && dup_wants_compare(4, 10, 5, 10));
  CHECK(!dup_wants_compare(10, 10, 10, 10) && !dup_wants_compare(11, 10, 3, 10));  // the queue is empty
  CHECK(dup_wants_compare(9, 10, 4000000000u, 10));  // a hash queue past its end counts as all tiles
  // products near and past 2^32 and up to 2^64: 64-bit cross-multiplication
  CHECK(dup_compares_not_ahead(65536, 65537, 65536, 65537));
  CHECK(!dup_compares_not_ahead(65537, 131072, 32768, 65537));  // 65537^2 > 2^32 + 2^16: not truncated
  CHECK(dup_compares_not_ahead(65536, 131072, 32768, 65536) && !dup_compares_not_ahead(65537, 131072, 32768, 65536));
  CHECK(dup_compares_not_ahead(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu));
  CHECK(!dup_compares_not_ahead(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu));
  CHECK(dup_compares_not_ahead(0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu));
  CHECK(dup_compares_not_ahead(0x80000000u, 0xFFFFFFFFu, 0x80000001u, 0xFFFFFFFFu));
  CHECK(!dup_compares_not_ahead(1, 0xFFFFFFFFu, 0, 0xFFFFFFFFu));

  // the CU slot: any value of the two registers stays in the table, and the CUs of a chip (XCC
  // 0-7, SE, SH and CU fields in HW_ID[15:8]) get different slots whatever the other bits hold
  for (uint32_t i = 0; i < 200000; ++i) {
    const uint32_t x = rnd(0xFFFFFFFFu) ^ (rnd(2) << 31), h = rnd(0xFFFFFFFFu) ^ (rnd(2) << 31);
    CHECK(dup_cu_slot(x, h) < DUP_CU_SLOTS);
  }
  CHECK(dup_cu_slot(0xFFFFFFFFu, 0xFFFFFFFFu) == DUP_CU_SLOTS - 1 && dup_cu_slot(0, 0) == 0);
  {
    std::vector<uint8_t> used(DUP_CU_SLOTS, 0);
    for (uint32_t xcc = 0; xcc < 8; ++xcc)
      for (uint32_t id = 0; id < 256; ++id) {
        const uint32_t s = dup_cu_slot(xcc | 0xABCDEF00u, (id << 8) | 0x5A | 0x12340000u);
        CHECK(!used[s]);
        used[s] = 1;
      }
  }

  // grid and budget: one spare workgroup is enough for any split of n into hashed and candidate files
  const uint32_t ns[] = {1, 2, 255, 256, 257, 511, 512, 513, 65536, 196608, 1310720};
  for (uint32_t n : ns) {
    const uint32_t hs[] = {1, 2, 255, 256, 257, n / 3, n / 2 + 1, n - 257, n - 256, n - 255, n - 1, n};
    for (uint32_t n_hash : hs) {
      if (n_hash < 1 || n_hash > n) continue;
      const uint32_t G = dup_role_grid(n), TH = dup_role_hash_tiles(n_hash);
      CHECK(TH * DUP_ROLE_BLOCK >= n_hash && (TH - 1) * DUP_ROLE_BLOCK < n_hash);
      CHECK(G > TH);
      CHECK((uint64_t)dup_compare_budget(G, TH) * DUP_ROLE_BLOCK >= n - n_hash);
    }
  }
  CHECK(dup_role_wave_tasks() * 4 * DUP_RUN_K >= DUP_ROLE_BLOCK * DUP_QUOTA_MUL);
  // quotas only where workgroups wait for a place: a grid of more workgroups than the chip holds
  CHECK(!dup_compare_has_quota(1024, 1024) && dup_compare_has_quota(1025, 1024) && !dup_compare_has_quota(1, 1024));

  // the default placement: run-time roles from three rounds of the chip's slots on (12 quanta of
  // 256 files per CU, plus the spare workgroup)
  CHECK(!dup_roles_pay(dup_role_grid(11 * 65536), 1024) && dup_roles_pay(dup_role_grid(12 * 65536), 1024));
  CHECK(!dup_roles_pay(3071, 1024) && dup_roles_pay(3072, 1024) && dup_roles_pay(0xFFFFFFFFu, 0xFFFFFFFFu / 3));
  CHECK(!dup_roles_pay(0xFFFFFFFFu, 0xFFFFFFFFu));  // (no 32-bit wrap of rounds x slots)

  // arrival orders: every hash tile and every task exactly once, the CU table back at zero
  const uint32_t shapes[][2] = {{65536, 45883}, {65536, 1}, {65536, 65536}, {65536, 65530}, {4096, 2000},
                                {4096, 257}, {300, 1}, {300, 299}, {257, 256}, {1, 1}, {20000, 255}, {20000, 19744}};
  for (const auto& sh : shapes)
    for (uint32_t cus : {1u, 2u, 8u, 64u})
      for (uint32_t stale : {0u, 3u, 1000000u}) simulate(sh[0], sh[1], cus, stale);
  if (fails) return 1;
  printf("dup_roles ok LIMIT=%u QUOTA=%u K=%u\n", DUP_CU_LIMIT, DUP_QUOTA_MUL, DUP_RUN_K);
  return 0;
}
