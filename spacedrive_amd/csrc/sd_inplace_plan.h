// sd_inplace_plan.h — where the sampled cas message of a file lies INSIDE the file (K1P,
// cas_inplace.hip).  Plain arithmetic, host and device, so the CPU suite checks it against
// the oracle's literal simulation of cas.rs:35-58 (tests/test_inplace_cpu.py).
//
// For len > MINIMUM_FILE_SIZE the gathered content is six segments of the file:
//   header F[0, 8192), samples F[8192 + k*j, +10240) for k = 0..3 with j = (len - 16384) / 4,
//   footer F[len - 8192, len)
// laid back to back (57,344 B).  Every segment boundary of the gathered content is a
// multiple of 1,024, and the message M = le64(len) || gathered shifts the content by 8 bytes,
// so BLAKE3 chunk c >= 1 of M is the 8 bytes BEFORE gathered offset 1024 c (the "carry": the
// previous segment's tail at a segment boundary) followed by the 1,016 bytes FROM it, which
// lie in one segment.  Chunk 56 is the carry alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_PLAN_HD __host__ __device__
#else
#define SD_PLAN_HD
#endif

namespace sdcas {

constexpr uint32_t INPLACE_SEGMENTS = 6;
constexpr uint32_t INPLACE_CHUNKS = 57;  // (8 + 57,344) / 1024 rounded up
constexpr uint64_t INPLACE_HEAD = 8192, INPLACE_SAMPLE = 10240, INPLACE_SAMPLES = 4;

// gathered offset at which segment s starts, in 1 KiB units: 0, 8, 18, 28, 38, 48 (56 = end)
SD_PLAN_HD inline uint32_t inplace_seg_g0_kib(uint32_t s) { return s == 0 ? 0u : 10u * s - 2u; }

// file offset and length of segment s (0 header, 1..4 samples, 5 footer); len > 102,400
SD_PLAN_HD inline uint64_t inplace_seg_start(uint64_t len, uint32_t s) {
  const uint64_t j = (len - 2 * INPLACE_HEAD) / INPLACE_SAMPLES;
  return s == 0 ? 0 : s == 5 ? len - INPLACE_HEAD : INPLACE_HEAD + (uint64_t)(s - 1) * j;
}
SD_PLAN_HD inline uint64_t inplace_seg_len(uint32_t s) {
  return s == 0 || s == 5 ? INPLACE_HEAD : INPLACE_SAMPLE;
}

// the segment holding gathered offset 1024 c, c < 56
SD_PLAN_HD inline uint32_t inplace_seg_of_chunk(uint32_t c) { return c < 8u ? 0u : (c + 2u) / 10u; }

// file offset of gathered offset 1024 c (the body of message chunk c, c < 56)
SD_PLAN_HD inline uint64_t inplace_body_off(uint64_t len, uint32_t c) {
  const uint32_t s = inplace_seg_of_chunk(c);
  return inplace_seg_start(len, s) + 1024ull * (c - inplace_seg_g0_kib(s));
}

// file offset of the 8 bytes before gathered offset 1024 c (1 <= c <= 56): message words
// 256 c and 256 c + 1
SD_PLAN_HD inline uint64_t inplace_carry_off(uint64_t len, uint32_t c) {
  if (c == INPLACE_CHUNKS - 1) return len - 8;
  const uint32_t s = inplace_seg_of_chunk(c);
  if (c != inplace_seg_g0_kib(s)) return inplace_body_off(len, c) - 8;
  return inplace_seg_start(len, s - 1) + inplace_seg_len(s - 1) - 8;  // the previous segment's tail
}

}  // namespace sdcas
