// Runs blake3_tree.hpp's level code on the CPU over simulated lanes: the in-LDS phases
// (level_read for every lane, then level_write for every lane, on a heap array that stands for
// LDS and holds exactly `count` CVs, so a slot read or written past it is an AddressSanitizer
// report) and the stride form (an array of per-lane CVs, "lane above" an index).  No HIP
// runtime call.  Expected values: the recursive left-balanced definition below (left subtree
// = the largest power of two strictly below n leaves) over pseudo-random leaf CVs.  Output:
//   <family> <cases> <mismatches>       one line per family of cases
//   o <count> <64 hex digits>           the root of a message of `count` chunks, the last 1 byte
//                                       long, its leaves from blake3_lane.hpp's PLAIN chunk
//                                       routines (tests/test_tree_reduce_cpu.py: vs the oracle)
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "blake3_lane.hpp"
#include "blake3_tree.hpp"

using namespace sdcas;
typedef uint32_t Cv[8];

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static void expected(const Cv* leaf, uint32_t n, bool root, Cv& out) {
  if (n == 1) { memcpy(out, leaf[0], sizeof(Cv)); return; }
  uint32_t split = 1;
  while (2 * split < n) split *= 2;
  Cv l, r;
  expected(leaf, split, false, l);
  expected(leaf + split, n - split, false, r);
  parent(out, l, r, root ? (uint32_t)ROOT : 0u);
}

// One wave or workgroup of `slices` scopes side by side, `lanes` lanes and counts[s] CVs each,
// slice s at lds + s * lanes: the device loop's phases with the sync left out.  `trips`: the
// count that governs the number of levels (the scope's own, or `lanes` for 16-lane slices).
template <int PER>
static void lds_reduce_sim(Cv* lds, uint32_t lanes, uint32_t slices, const uint32_t* counts,
                           uint32_t trips, bool root_last) {
  Cv(*out)[PER] = (Cv(*)[PER])malloc(sizeof(Cv) * PER * lanes * slices);
  TreeLevel lv[4];
  for (uint32_t s = 0; s < slices; ++s) lv[s] = TreeLevel{counts[s]};
  for (TreeLevel trip{trips}; trip.count > 1u; trip = trip.next()) {
    for (uint32_t t = 0; t < lanes * slices; ++t)
      for (int k = 0; k < PER; ++k)
        level_read(lv[t / lanes], lds + t / lanes * lanes, t % lanes + k * lanes, root_last, out[t][k]);
    for (uint32_t t = 0; t < lanes * slices; ++t)
      for (int k = 0; k < PER; ++k)
        level_write(lv[t / lanes], lds + t / lanes * lanes, t % lanes + k * lanes, out[t][k]);
    for (uint32_t s = 0; s < slices; ++s) lv[s] = lv[s].next();
  }
  free(out);
}

// `count` leaves through one scope of `lanes` lanes; the LDS array holds exactly count CVs
template <int PER>
static void lds_root(const Cv* leaf, uint32_t lanes, uint32_t count, bool root_last, Cv& got) {
  Cv* lds = (Cv*)malloc(sizeof(Cv) * count);
  memcpy(lds, leaf, sizeof(Cv) * count);
  lds_reduce_sim<PER>(lds, lanes, 1, &count, count, root_last);
  memcpy(got, lds[0], sizeof(Cv));
  free(lds);
}

// segment_merge<SEG, 1> with from_lane_above as an index (a lane past the segment reads 0)
static void stride_root(const Cv* leaf, uint32_t seg, uint32_t count, Cv& got) {
  Cv cv[64], r[64];
  for (uint32_t l = 0; l < seg; ++l)
    for (int w = 0; w < 8; ++w) cv[l][w] = l < count ? leaf[l][w] : 0xDEAD0000u + l;  // never read
  for (uint32_t S = 1; S < seg; S *= 2) {
    for (uint32_t l = 0; l < seg; ++l)
      for (int w = 0; w < 8; ++w) r[l][w] = l + S < seg ? cv[l + S][w] : 0u;
    for (uint32_t l = 0; l < seg; ++l) stride_level(TreeLevel{count}, cv[l], r[l], l, S);
    count = TreeLevel{count}.next().count;
  }
  if (count != 1) exit(3);
  memcpy(got, cv[0], sizeof(Cv));
}

static uint8_t content_byte(uint32_t len, uint32_t i) {  // lane_walker_test.cpp's
  return (uint8_t)(((i + 1u) * 2654435761u + len * 0x9E3779B1u) >> 11);
}

// the true chunk CVs of a message of `count` chunks whose last chunk is 1 byte long
static void chunk_leaves(uint32_t count, Cv* leaf) {
  const uint32_t len = (count - 1u) * 1024u + 1u;
  const size_t alloc = ((size_t)len + 15u) / 16u * 16u;
  uint8_t* buf = (uint8_t*)malloc(alloc);
  memset(buf, 0xFF, alloc);
  for (uint32_t i = 0; i < len; ++i) buf[i] = content_byte(len, i);
  const uint4* q = reinterpret_cast<const uint4*>(buf);
  for (uint32_t c = 0; c < count; ++c) {
    uint4 A[8], B[8];
    uint32_t c0 = 0, c1 = 0;
    line_clamped(q, 8u * c, len, A);
    if (c + 1 < count) full_chunk<PLAIN>(q, len, c, leaf[c], A, B, c0, c1);
    else last_chunk<PLAIN>(q, len, c, 1u, count == 1, leaf[c], A, B, c0, c1);
  }
  free(buf);
}

int main() {
  static Cv leaf[1024];
  for (auto& cv : leaf)
    for (auto& w : cv) w = rnd();
  uint32_t bad_total = 0;
  auto report = [&](const char* family, uint32_t cases, uint32_t bad) {
    printf("%s %" PRIu32 " %" PRIu32 "\n", family, cases, bad);
    bad_total += bad;
  };
  auto differs = [](const Cv& a, const Cv& b) { return memcmp(a, b, sizeof(Cv)) != 0 ? 1u : 0u; };
  Cv want, got;
  for (int root = 0; root < 2; ++root) {
    uint32_t bad[4] = {0, 0, 0, 0};
    for (uint32_t n = 1; n <= 1024; ++n) {
      expected(leaf, n, root, want);
      if (n <= 256) { lds_root<1>(leaf, 256, n, root, got); bad[0] += differs(got, want); }
      lds_root<2>(leaf, 256, n, root, got); bad[1] += differs(got, want);
      if (n <= 64) { lds_root<1>(leaf, 64, n, root, got); bad[2] += differs(got, want); }
    }
    // four 16-lane slices of one wave, different counts, log2(16) levels in step; slice 0
    // takes every count, and every slice's slots past its count are poisoned
    for (uint32_t n = 1; n <= 16; ++n) {
      const uint32_t counts[4] = {n, 17u - n, (n + 6u) % 16u + 1u, (5u * n) % 16u + 1u};
      Cv lds[64];
      memset(lds, 0xA5, sizeof lds);
      for (uint32_t s = 0; s < 4; ++s) memcpy(lds + 16 * s, leaf + 100 * s, sizeof(Cv) * counts[s]);
      lds_reduce_sim<1>(lds, 16, 4, counts, 16, root);
      for (uint32_t s = 0; s < 4; ++s) {
        expected(leaf + 100 * s, counts[s], root, want);
        bad[3] += differs(lds[16 * s], want);
      }
    }
    const char* names[2][4] = {{"lds256x1", "lds256x2", "lds64", "slices16"},
                               {"lds256x1_root", "lds256x2_root", "lds64_root", "slices16_root"}};
    const uint32_t cases[4] = {256, 1024, 64, 64};
    for (int k = 0; k < 4; ++k) report(names[root][k], cases[k], bad[k]);
  }
  for (uint32_t seg = 16; seg <= 64; seg *= 4) {
    uint32_t bad = 0;
    for (uint32_t n = 1; n <= seg; ++n) {
      expected(leaf, n, true, want);
      stride_root(leaf, seg, n, got);
      bad += differs(got, want);
    }
    report(seg == 16 ? "stride16" : "stride64", seg, bad);
  }
  // the oracle tie: every form that holds the count must give the same root
  const uint32_t big[5] = {255, 256, 257, 1023, 1024};
  for (uint32_t i = 0; i < 64 + 5; ++i) {
    const uint32_t n = i < 64 ? i + 1 : big[i - 64];
    chunk_leaves(n, leaf);
    lds_root<2>(leaf, 256, n, true, want);
    uint32_t bad = 0;
    if (n <= 512) { lds_root<1>(leaf, 256, n, true, got); bad += differs(got, want); }
    if (n <= 64) {
      lds_root<1>(leaf, 64, n, true, got); bad += differs(got, want);
      stride_root(leaf, 64, n, got); bad += differs(got, want);
    }
    if (n <= 16) { stride_root(leaf, 16, n, got); bad += differs(got, want); }
    bad_total += bad;
    printf("o %" PRIu32 " ", n);
    for (int w = 0; w < 8; ++w)
      for (int b = 0; b < 4; ++b) printf("%02x", (want[w] >> (8 * b)) & 0xFFu);
    printf("%s\n", bad ? " FORMS-DISAGREE" : "");
  }
  return bad_total ? 1 : 0;
}
