// ws_carve_test.cpp — sd_ws.h alone (plain C++, no HIP): measuring from a null base and
// carving from a real one are the same walk.  Exits non-zero at the first violated property.
#include <stdio.h>
#include <stdlib.h>

#include "sd_ws.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

// one walk used for both the measure and the carve: u64[a] | u32[b] | 256 B | u8[c] | u64[0] | u16[d]
struct Walk {
  uintptr_t p[5];
  size_t bytes;
};
static Walk walk(void* base, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  WsCarve w(base);
  Walk r;
  r.p[0] = (uintptr_t)w.take<uint64_t>(a);
  r.p[1] = (uintptr_t)w.take<uint32_t>(b);
  w.skip(256);
  r.p[2] = (uintptr_t)w.take<uint8_t>(c);
  r.p[3] = (uintptr_t)w.take<uint64_t>(0);
  r.p[4] = (uintptr_t)w.take<uint16_t>(d);
  r.bytes = w.bytes();
  return r;
}

int main() {
  CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512);
  CHECK(up128(1) == 128 && up128(128) == 128 && up16(17) == 32);
  CHECK(up256(((size_t)1 << 32) + 1) == ((size_t)1 << 32) + 256);

  const uint64_t shapes[][4] = {{1, 1, 1, 1}, {31, 33, 255, 129}, {32, 64, 256, 128}, {33, 65, 257, 127},
                                {0, 0, 0, 0}, {4097, 0, 100000, 3}};
  for (const auto& s : shapes) {
    const Walk m = walk(nullptr, s[0], s[1], s[2], s[3]);
    void* raw = malloc(m.bytes + 256);
    CHECK(raw);
    char* base = (char*)(((uintptr_t)raw + 255) & ~(uintptr_t)255);
    const Walk c = walk(base, s[0], s[1], s[2], s[3]);
    CHECK(c.bytes == m.bytes);
    const size_t want[5] = {(size_t)s[0] * 8, (size_t)s[1] * 4, (size_t)s[2], 0, (size_t)s[3] * 2};
    uintptr_t end = (uintptr_t)base;  // end of the previous take (+ the skip)
    for (int k = 0; k < 5; k++) {
      CHECK(c.p[k] % 256 == 0);
      CHECK(c.p[k] == end + (k == 2 ? 256 : 0));                // disjoint and gap-free
      CHECK(c.p[k] - (uintptr_t)base == m.p[k]);                // measuring sees the same offsets
      end = c.p[k] + up256(want[k]);
    }
    CHECK(c.p[3] == c.p[4]);  // a take of 0 elements advances by 0
    CHECK(end - (uintptr_t)base == c.bytes);
    // every byte handed out is inside the allocation
    for (int k = 0; k < 5; k++)
      if (want[k]) { ((volatile char*)c.p[k])[0] = 1; ((volatile char*)c.p[k])[want[k] - 1] = 1; }
    free(raw);
  }

  // take<uint64_t>(n) advances by up256(8 n), with no 32-bit wrap (measured: no allocation)
  const uint64_t ns[] = {1, 31, 32, 33, ((uint64_t)1 << 32) + 1};
  for (uint64_t n : ns) {
    WsCarve w(nullptr);
    CHECK(w.take<uint64_t>(n) == nullptr && w.bytes() == up256((size_t)n * 8));
    CHECK((uintptr_t)w.rest() == w.bytes());
    const size_t before = w.bytes();
    w.take<uint64_t>(n);
    CHECK(w.bytes() - before == up256((size_t)n * 8));
  }
  {
    WsCarve w(nullptr);
    w.take<uint64_t>(((uint64_t)1 << 32) + 1);
    CHECK(w.bytes() == ((size_t)8 << 32) + 256);
  }
  printf("ws_carve ok\n");
  return 0;
}
