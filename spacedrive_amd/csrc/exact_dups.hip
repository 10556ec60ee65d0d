// exact_dups.hip — split a grouping by whole-content checksum, on gfx950.
//
// A cas_id is a sampled hash (cas.rs:31-58): two files of one size that agree in the header,
// the four samples and the footer share it whatever the rest holds.  The library also has the
// BLAKE3 of every file's whole content (file_checksum, validation/hash.rs:11-25); joining the
// two columns gives the sets that really are byte-identical:
//   rep_exact[i] = min{ j : rep[j] == rep[i] && digest[j] == digest[i] }
// Fast path: one u64 key per row from (rep, digest bytes 0..8), the context's grouping over
// those keys, then a check of every non-head row's full (rep, 32-byte digest) against its
// head's.  No mismatch = the grouping is exact: equal pairs have equal keys, and every member
// equals its head.  Any mismatch: the word-wise path (reports_host.cpp) regroups by one digest
// word at a time, which is exact by construction.  Elementwise integer passes bound by HBM;
// digests are read as 16-byte vector loads, every write is a plain vector store or an atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_debug.h"
#include "sd_exact_dups.h"

namespace sdcas {

constexpr int EX_THREADS = 256;

extern "C" __global__ void __launch_bounds__(EX_THREADS)
sd_exact_keys(const uint32_t* __restrict__ rep, const uint4* __restrict__ dig, uint64_t n,
              uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4 a = dig[2 * i];
  const uint64_t w0 = ((uint64_t)a.y << 32) | a.x;
  keys[i] = w0 ^ (rep ? (uint64_t)rep[i] * EXACT_KEY_MUL : 0ull);
}

// The gather through head[] is uncoalesced by nature (68 B per non-head row: its head's rep
// and digest); a set's members share their head's lines, so duplicates mostly hit L2.  The
// count is reduced per wave with one ballot and leaves as at most one atomic per wave — none
// at all on the expected input, where nothing mismatches.
extern "C" __global__ void __launch_bounds__(EX_THREADS)
sd_exact_verify(const uint32_t* __restrict__ rep, const uint4* __restrict__ dig,
                const uint32_t* __restrict__ head, uint64_t n, uint32_t* __restrict__ mismatched,
                int after_words) {
  const uint64_t i = (uint64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const uint32_t h = head[i];
    if (h != (uint32_t)i) {
      if (h > i) {
        bad = true;  // not a grouping's output: counted, never indexed
      } else {
        const uint4 a0 = dig[2 * i], a1 = dig[2 * i + 1];
        const uint4 b0 = dig[2 * (uint64_t)h], b1 = dig[2 * (uint64_t)h + 1];
        const uint32_t d = (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) |
                           (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w);
        bad = d != 0u || (rep && rep[i] != rep[h]);
      }
      if (after_words)
        SD_DBG_CHECK(!bad, "group_exact: row %llu differs from its head %u after the word-wise path",
                     (unsigned long long)i, h);
    }
  }
  const uint64_t m = __ballot(bad);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(mismatched, (uint32_t)__popcll(m));
}

extern "C" __global__ void __launch_bounds__(EX_THREADS)
sd_exact_word_keys(const uint4* __restrict__ dig, uint32_t w, uint64_t n, uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4 a = dig[2 * i + (w >> 1)];
  keys[i] = (w & 1u) ? (((uint64_t)a.w << 32) | a.z) : (((uint64_t)a.y << 32) | a.x);
}

extern "C" __global__ void __launch_bounds__(EX_THREADS)
sd_exact_pair_keys(const uint32_t* __restrict__ cls, const uint32_t* __restrict__ ids, uint64_t n,
                   uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i >= n) return;
  keys[i] = ((uint64_t)(cls ? cls[i] : 0u) << 32) | ids[i];
}

extern "C" __global__ void __launch_bounds__(EX_THREADS)
sd_exact_scatter(const uint32_t* __restrict__ rep_c, const uint32_t* __restrict__ rows, uint64_t m,
                 uint32_t* __restrict__ full) {
  const uint64_t j = (uint64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  if (j >= m) return;
  const uint32_t r = rep_c[j];
  full[rows[j]] = rows[r <= j ? r : j];
}

// ---- launchers -------------------------------------------------------------------------
static inline uint32_t ex_grid(uint64_t n) { return (uint32_t)((n + EX_THREADS - 1) / EX_THREADS); }
static inline bool ex_ok(uint64_t n) { return n > 0 && n < (1ull << 32); }

hipError_t exact_keys(const uint32_t* rep, const uint8_t* digests, uint64_t n, uint64_t* keys,
                      hipStream_t s) {
  if (!ex_ok(n)) return hipErrorInvalidValue;
  sd_exact_keys<<<ex_grid(n), EX_THREADS, 0, s>>>(rep, (const uint4*)digests, n, keys);
  return hipGetLastError();
}

hipError_t exact_verify(const uint32_t* rep, const uint8_t* digests, const uint32_t* head, uint64_t n,
                        uint32_t* mismatched, bool after_words, hipStream_t s) {
  if (!ex_ok(n)) return hipErrorInvalidValue;
  sd_exact_verify<<<ex_grid(n), EX_THREADS, 0, s>>>(rep, (const uint4*)digests, head, n, mismatched,
                                                    after_words ? 1 : 0);
  return hipGetLastError();
}

hipError_t exact_word_keys(const uint8_t* digests, uint32_t w, uint64_t n, uint64_t* keys, hipStream_t s) {
  if (!ex_ok(n) || w > 3) return hipErrorInvalidValue;
  sd_exact_word_keys<<<ex_grid(n), EX_THREADS, 0, s>>>((const uint4*)digests, w, n, keys);
  return hipGetLastError();
}

hipError_t exact_pair_keys(const uint32_t* cls, const uint32_t* ids, uint64_t n, uint64_t* keys,
                           hipStream_t s) {
  if (!ex_ok(n)) return hipErrorInvalidValue;
  sd_exact_pair_keys<<<ex_grid(n), EX_THREADS, 0, s>>>(cls, ids, n, keys);
  return hipGetLastError();
}

hipError_t exact_scatter(const uint32_t* rep_c, const uint32_t* rows, uint64_t m, uint32_t* full,
                         hipStream_t s) {
  if (!ex_ok(m)) return hipErrorInvalidValue;
  sd_exact_scatter<<<ex_grid(m), EX_THREADS, 0, s>>>(rep_c, rows, m, full);
  return hipGetLastError();
}

SD_DBG_ACCESSOR(sd_dbg_violations_exact_dups)

}  // namespace sdcas
