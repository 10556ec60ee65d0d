// sd_dup_probe.h — the 64-bit probe that nominates duplicate candidates for the fused chain's
// verify-by-comparison (dup_verify.hip, K1V).  Plain arithmetic, host and device, so a host
// program checks its bounds under a sanitizer (tests/native/dup_probe_test.cpp).
//
// Two sampled files have the same cas key when their sizes and their 57,344 content bytes are
// equal.  The probe mixes the size with the first and the last 32 content bytes: equal files
// have equal probes, and files with equal probes are only CANDIDATES — the comparison of all
// 57,344 bytes decides, so a probe collision costs time and never a wrong key.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SD_PROBE_HD __host__ __device__
#else
#define SD_PROBE_HD
#endif

namespace sdcas {

constexpr uint32_t DUP_PROBE_ROW = 57344;  // a row's content bytes (SAMPLED_CONTENT_LEN)
constexpr uint32_t DUP_PROBE_EDGE = 32;    // bytes read at each end of the row
constexpr uint32_t DUP_PROBE_TAIL = DUP_PROBE_ROW - DUP_PROBE_EDGE;  // 57,312

// splitmix64 finalizer (sd_mix.h's mix64, which is device only)
SD_PROBE_HD inline uint64_t dup_probe_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// row: the file's 57,344 content bytes, 16-B aligned (the sampled layout's contract).  Reads
// row[0, 32) and row[57,312, 57,344) and nothing else: never the stride padding after a row.
SD_PROBE_HD inline uint64_t dup_probe(uint64_t size, const void* row) {
  const uint8_t* p = (const uint8_t*)__builtin_assume_aligned(row, 16);
  uint64_t w[8];
  memcpy(w, p, DUP_PROBE_EDGE);
  memcpy(w + 4, p + DUP_PROBE_TAIL, DUP_PROBE_EDGE);
  uint64_t h = dup_probe_mix(size ^ 0x5344445550564552ull);
  for (int i = 0; i < 8; ++i) h = dup_probe_mix(h ^ w[i]);
  return h;
}

}  // namespace sdcas
