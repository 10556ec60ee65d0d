// Host test of sd_dup_probe.h (a stand-alone program; tests/test_dup_probe_cpu.py builds it with
// -fsanitize=address,undefined).  The row is a heap block of exactly 57,344 B, 16-B aligned, so
// a read before row offset 0 or past 57,312 + 32 is a heap overflow the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sd_dup_probe.h"

using namespace sdcas;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  static_assert(DUP_PROBE_TAIL == 57312 && DUP_PROBE_TAIL + DUP_PROBE_EDGE == DUP_PROBE_ROW, "edges");
  uint8_t* row = (uint8_t*)aligned_alloc(16, DUP_PROBE_ROW);  // nothing after the row
  uint8_t* twin = (uint8_t*)aligned_alloc(16, DUP_PROBE_ROW);
  if (!row || !twin) return 2;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (uint32_t i = 0; i < DUP_PROBE_ROW; ++i) {
    x = dup_probe_mix(x + i);
    row[i] = (uint8_t)x;
  }
  memcpy(twin, row, DUP_PROBE_ROW);
  const uint64_t size = 123456789;
  const uint64_t p = dup_probe(size, row);
  // determinism: the same bytes at another address, and the same call again
  CHECK(dup_probe(size, row) == p);
  CHECK(dup_probe(size, twin) == p);
  // the size and every byte of both edges count: [0, 32) and [57,312, 57,344)
  CHECK(dup_probe(size + 1, row) != p);
  for (uint32_t i = 0; i < DUP_PROBE_EDGE; ++i) {
    twin[i] ^= 1;
    CHECK(dup_probe(size, twin) != p);
    twin[i] ^= 1;
    twin[DUP_PROBE_TAIL + i] ^= 0x80;
    CHECK(dup_probe(size, twin) != p);
    twin[DUP_PROBE_TAIL + i] ^= 0x80;
  }
  // nothing between the edges does (those bytes are the comparison's business)
  const uint32_t inner[] = {32, 33, 28671, 28672, 57310, 57311};
  for (uint32_t off : inner) {
    twin[off] ^= 0xFF;
    CHECK(dup_probe(size, twin) == p);
    twin[off] ^= 0xFF;
  }
  // swapping the edges is another probe (the words are chained, not summed)
  memcpy(twin, row + DUP_PROBE_TAIL, DUP_PROBE_EDGE);
  memcpy(twin + DUP_PROBE_TAIL, row, DUP_PROBE_EDGE);
  CHECK(dup_probe(size, twin) != p);
  free(row);
  free(twin);
  if (fails) return 1;
  printf("dup_probe ok %016llx\n", (unsigned long long)p);
  return 0;
}
