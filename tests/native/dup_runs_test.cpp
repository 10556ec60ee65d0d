// Host test of sd_dup_runs.h (a stand-alone program; tests/test_dup_groups_cpu.py builds it plain
// and with -fsanitize=address,undefined).  It replays K1V's compare tasks on the CPU: list C is a
// heap array of exactly n_cand entries and a row a heap block of exactly 57,344 B, so an index
// past the list's end or a quad past the row's end is a heap overflow the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sd_dup_runs.h"

using namespace sdcas;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

constexpr uint32_t K = DUP_RUN_K;

// groups: the copies of each original, in list C's order.  Walks every task's window as the
// kernel does and returns the reference rows read (one per run of a window).
static uint32_t replay(const std::vector<uint32_t>& groups, uint32_t* tasks_out) {
  uint32_t n_cand = 0;
  for (uint32_t g : groups) n_cand += g;
  uint32_t* orig = (uint32_t*)malloc(n_cand ? n_cand * sizeof(uint32_t) : 1);  // orig[i] of entry i
  uint32_t* first = (uint32_t*)malloc(groups.size() ? groups.size() * sizeof(uint32_t) : 1);
  uint8_t* seen = (uint8_t*)calloc(n_cand ? n_cand : 1, 1);
  uint32_t p = 0;
  for (uint32_t g = 0; g < groups.size(); ++g) {
    first[g] = p;
    for (uint32_t i = 0; i < groups[g]; ++i) orig[p++] = g;
  }
  const uint32_t tasks = dup_task_count(n_cand);
  CHECK(tasks == (n_cand + K - 1) / K);
  uint32_t refs = 0;
  for (uint32_t t = 0; t < tasks; ++t) {
    const uint32_t a = dup_task_first(t), m = dup_task_entries(t, n_cand);
    CHECK(m >= 1 && m <= K && a + m <= n_cand);
    CHECK(t + 1 == tasks ? a + m == n_cand : m == K);  // only the last window is short
    for (uint32_t e = 0; e < m; ++e) {
      CHECK(!seen[a + e]);  // every entry in exactly one task
      seen[a + e] = 1;
      // the kernel's rule for a run's head: the window's first entry, or a group's first slot
      const bool head = e == 0 || first[orig[a + e]] == a + e;
      CHECK(head == (e == 0 || orig[a + e] != orig[a + e - 1]));
      refs += head;
    }
  }
  for (uint32_t i = 0; i < n_cand; ++i) CHECK(seen[i]);
  free(orig);
  free(first);
  free(seen);
  *tasks_out = tasks;
  return refs;
}

int main() {
  static_assert(DUP_SLICES == 7 && DUP_SLICE_BYTES == 8192, "a row is seven 8-KiB slices");
  uint32_t tasks = 0;
  // zero candidates: no task, no reference
  CHECK(dup_task_count(0) == 0);
  CHECK(replay({}, &tasks) == 0 && tasks == 0);
  // one group of K - 1, K, K + 1, 2K + 1 entries: a reference per window it spans
  const uint32_t lens[] = {1, K - 1, K, K + 1, 2 * K, 2 * K + 1};
  for (uint32_t len : lens) {
    if (!len) continue;
    const uint32_t refs = replay({len}, &tasks);
    CHECK(tasks == (len + K - 1) / K);
    CHECK(refs == tasks);
    CHECK(dup_task_entries(tasks - 1, len) == (len % K ? len % K : K));  // the window at the list's end
  }
  // a group ending exactly at a window's edge: the next group's head is the next window's first
  // entry and costs no extra reference
  CHECK(replay({K, 3}, &tasks) == 2 && tasks == 2);
  CHECK(replay({K - 1, 1, K, 1}, &tasks) == 4 && tasks == 3);
  // a group cut by a window's edge costs one extra reference
  CHECK(replay({K - 1, 2}, &tasks) == 3 && tasks == 2);
  // singles: a reference per entry, whatever the windows
  CHECK(replay(std::vector<uint32_t>(3 * K + 1, 1), &tasks) == 3 * K + 1 && tasks == 4);
  // references are groups + cut groups, at most groups + tasks
  {
    std::vector<uint32_t> g;
    uint64_t x = 12345;
    uint32_t n = 0;
    for (int i = 0; i < 500; ++i) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      g.push_back(1 + (uint32_t)(x >> 59) * (uint32_t)((x >> 40) & 3));
      n += g.back();
    }
    const uint32_t refs = replay(g, &tasks);
    CHECK(refs >= g.size() && refs <= g.size() + tasks - 1);
    CHECK(tasks == dup_task_count(n));
  }

  // interleaved tile -> hash tile or compare tile: every hash tile once, in order; TC compare
  // tiles, the last min(TC, tail) of them the tail
  const uint32_t shapes[][3] = {{2561, 1793, 366}, {257, 180, 731}, {257, 256, 731}, {129, 1, 183},
                                {2, 1, 1}, {2, 0, 7}, {9, 8, 1}, {100, 37, 1}, {100, 37, 50}};
  for (const auto& sh : shapes) {
    const uint32_t G = sh[0], TH = sh[1], tail = sh[2], TC = G - TH;
    const uint32_t TT = TC < tail ? TC : tail;
    uint32_t hash = 0, cmp = 0, tails = 0;
    for (uint32_t b = 0; b < G; ++b) {
      const DupTile t = dup_tile_of(b, G, TH, tail);
      if (!t.compare) {
        CHECK(!t.tail);
        CHECK(t.hash_tile == hash);
        ++hash;
      } else {
        ++cmp;
        tails += t.tail;
        CHECK(t.tail == (b >= G - TT));
      }
    }
    CHECK(hash == TH && cmp == TC && tails == TT);
    CHECK(TT >= 1);  // some tile always drains the queue
  }
  CHECK(dup_tile_wave_tasks() * K >= DUP_WAVE && (dup_tile_wave_tasks() - 1) * K < DUP_WAVE);

  // slice -> quads: a wave's 7 x 8 loads of 64 quads cover the row's 3,584 quads once each, and
  // nothing else (the row is a heap block of exactly 57,344 B)
  uint8_t* row = (uint8_t*)aligned_alloc(16, DUP_ROW_BYTES);
  if (!row) return 2;
  memset(row, 0, DUP_ROW_BYTES);
  for (uint32_t s = 0; s < DUP_SLICES; ++s)
    for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u)
      for (uint32_t lane = 0; lane < DUP_WAVE; ++lane) {
        const uint32_t off = dup_slice_quad_offset(s, u, lane);
        CHECK(off % 16 == 0);
        CHECK(off == dup_slice_quad_offset(s, u, 0) + dup_slice_quad_offset(0, 0, lane));  // scalar + lane part
        for (uint32_t i = 0; i < 16; ++i) row[off + i]++;
      }
  for (uint32_t i = 0; i < DUP_ROW_BYTES; ++i)
    if (row[i] != 1) { CHECK(row[i] == 1); break; }
  CHECK(dup_slice_quad_offset(DUP_SLICES - 1, DUP_SLICE_QUADS - 1, DUP_WAVE - 1) + 16 == DUP_ROW_BYTES);
  free(row);
  if (fails) return 1;
  printf("dup_runs ok K=%u\n", K);
  return 0;
}
