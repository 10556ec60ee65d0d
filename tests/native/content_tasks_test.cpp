// content_tasks_test.cpp — a host program over spacedrive_amd/csrc/sd_content_tasks.h, the index
// arithmetic of the whole-content compare (tests/test_exact_compare_cpu.py builds it plain and
// with -fsanitize=address,undefined).  Prints "content_tasks ok" and the constants.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "sd_content_tasks.h"

using namespace sdcas;

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

static void pieces() {
  const uint64_t P = CT_PIECE_BYTES, S = CT_SLICE_BYTES;
  CHECK(P % S == 0 && S == 8192 && CT_RUN_K <= 32 && CT_RUN_K >= 1);
  CHECK(ct_pieces(0) == 0 && ct_pieces(1) == 1 && ct_pieces(P - 1) == 1 && ct_pieces(P) == 1 &&
        ct_pieces(P + 1) == 2);
  const uint64_t G = 1ull << 32;
  CHECK(ct_pieces(G - 1) == G / P && ct_pieces(G) == G / P && ct_pieces(G + 1) == G / P + 1);
  CHECK(ct_pieces(CT_MAX_LEN) == CT_MAX_LEN / P && CT_MAX_LEN / P == (1u << 20));
  // the pieces of a length tile it; the slices of a piece tile the piece; the limits end at the
  // 16-B round-up
  const uint64_t lens[] = {1, 15, 16, 17, S - 1, S, S + 1, P - 1, P, P + 1, 2 * P + 17, G - 1, G + 1, CT_MAX_LEN};
  for (uint64_t len : lens) {
    uint64_t covered = 0;
    const uint32_t np = ct_pieces(len);
    for (uint32_t p : std::set<uint32_t>{0u, 1u, np / 2, np - 2, np - 1}) {
      if (p >= np) continue;
      const uint32_t b = ct_piece_bytes(len, p);
      CHECK(b >= 1 && b <= P && (uint64_t)p * P + b <= len && (p + 1 < np ? b == P : (uint64_t)p * P + b == len));
      const uint32_t ns = ct_slices(b);
      CHECK(ns >= 1 && ns <= CT_PIECE_SLICES && (uint64_t)(ns - 1) * S < b && b <= (uint64_t)ns * S);
      for (uint32_t s = 0; s < ns; ++s) {
        const uint64_t from = (uint64_t)p * P + (uint64_t)s * S;
        CHECK(from < len);
        const uint32_t lim = ct_slice_limit(len, from);
        CHECK(lim % 16 == 0 && lim >= 16 && lim <= S && from + lim <= ((len + 15) & ~15ull));
        if (from + S >= len) {  // the content's last slice
          CHECK(from + lim == ((len + 15) & ~15ull));
          const uint32_t q = ct_last_quad(len, from);
          CHECK((uint64_t)q * 16 + 16 == lim && from + (uint64_t)q * 16 < len && len <= from + (uint64_t)q * 16 + 16);
        } else {
          CHECK(lim == S);
        }
      }
      covered += b;
    }
    if (np <= 3) CHECK(covered == len);
  }
  CHECK(ct_piece_bytes(CT_MAX_LEN, (1u << 20) - 1) == P && ct_piece_bytes(G + 1, (uint32_t)(G / P)) == 1);
}

static void masks() {
  for (uint32_t r = 0; r < 16; ++r) {
    const uint64_t len = 4096 + r + (r == 0 ? 16 : 0);
    uint8_t m[16];
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t w = ct_last_quad_mask(len, k);
      for (uint32_t b = 0; b < 4; ++b) m[4 * k + b] = (uint8_t)(w >> (8 * b));
    }
    const uint32_t keep = r ? r : 16;
    for (uint32_t b = 0; b < 16; ++b) CHECK(m[b] == (b < keep ? 0xFF : 0x00));
  }
}

static void windows(const std::vector<uint64_t>& lens) {
  const uint32_t n = (uint32_t)lens.size(), nw = ct_window_count(n);
  CHECK(nw == (n + CT_RUN_K - 1) / CT_RUN_K);
  std::vector<uint32_t> wstart(nw);
  uint64_t total = 0;
  uint32_t entries = 0;
  for (uint32_t w = 0; w < nw; ++w) {
    wstart[w] = (uint32_t)total;
    total += ct_window_pieces(lens.data(), w, n);
    CHECK(ct_window_first(w) == entries);
    const uint32_t m = ct_window_entries(w, n);
    CHECK(m >= 1 && m <= CT_RUN_K && (w + 1 < nw ? m == CT_RUN_K : entries + m == n));
    entries += m;
  }
  CHECK(entries == n && total == ct_task_count(lens.data(), n));
  // every task once, no (entry, piece) twice, and every (entry, piece) of the list in some task
  std::set<std::pair<uint32_t, uint32_t>> tasks, seen;
  for (uint32_t t = 0; t < total; ++t) {
    const CtTask k = ct_task_of(wstart.data(), nw, t);
    CHECK(k.window < nw && k.piece < ct_window_pieces(lens.data(), k.window, n));
    CHECK(tasks.insert({k.window, k.piece}).second);
    const uint32_t first = ct_window_first(k.window), m = ct_window_entries(k.window, n);
    for (uint32_t e = 0; e < m; ++e)
      if (ct_entry_in_piece(lens[first + e], k.piece)) CHECK(seen.insert({first + e, k.piece}).second);
  }
  uint64_t want = 0;
  for (uint64_t len : lens) want += ct_pieces(len);
  CHECK(seen.size() == want);
}

static void runs() {
  // pivots of a window's entries -> heads and runs
  const uint32_t piv[] = {7, 7, 7, 9, 9, 12, 40, 40};
  uint32_t heads = 0;
  for (uint32_t e = 0; e < 8; ++e)
    if (ct_run_starts(e, piv[e], e ? piv[e - 1] : 0)) heads |= 1u << e;
  CHECK(heads == ((1u << 0) | (1u << 3) | (1u << 5) | (1u << 6)));
  const uint32_t want[] = {1, 1, 1, 2, 2, 3, 4, 4};
  for (uint32_t e = 0; e < 8; ++e) CHECK(ct_run_of(heads, e) == want[e]);
  CHECK(ct_run_starts(0, 0, 0));  // a window's first entry starts a run whatever came before it
  CHECK(ct_run_of(0xFFFFFFFFu, 31) == 32 && ct_run_of(1u, 31) == 1);
}

int main() {
  pieces();
  masks();
  runs();
  const uint64_t P = CT_PIECE_BYTES, S = CT_SLICE_BYTES;
  const uint64_t mix[] = {0, 1, S - 1, S, S + 1, P - 1, P, P + 1, 2 * P + 17, 5 * P, 0, 3 * P + 1, 17};
  for (uint32_t n : {1u, CT_RUN_K - 1, CT_RUN_K, CT_RUN_K + 1, 2 * CT_RUN_K + 1}) {
    if (n == 0) continue;
    for (uint32_t shift = 0; shift < 13; ++shift) {
      std::vector<uint64_t> lens(n);
      for (uint32_t e = 0; e < n; ++e) lens[e] = mix[(e * 5 + shift) % 13];
      windows(lens);
    }
    windows(std::vector<uint64_t>(n, 0));  // no task at all
  }
  // windows without a task between windows with one
  {
    std::vector<uint64_t> lens(4 * CT_RUN_K, 0);
    lens[0] = 3 * P;
    lens[3 * CT_RUN_K + 1] = 2 * P + 1;
    windows(lens);
  }
  printf("content_tasks ok slice=%u piece=%u run_k=%u\n", CT_SLICE_BYTES, CT_PIECE_BYTES, CT_RUN_K);
  return 0;
}
