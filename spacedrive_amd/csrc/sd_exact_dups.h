// sd_exact_dups.h — launchers of the exact duplicate grouping's kernels (exact_dups.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdcas {

// The fast key of a row, restated for hosts and tests:
//   key[i] = le64(digest[i][0..8]) ^ (rep ? rep[i] * EXACT_KEY_MUL : 0)
// Equal (rep, digest) pairs give equal keys.  Only digest bytes 0..8 take part, so two rows of
// one rep whose digests differ in bytes 8..32 alone always collide (constructible in tests;
// BLAKE3 output is uniform there, so real rows collide with probability ~n^2 / 2^65).
constexpr uint64_t EXACT_KEY_MUL = 0x9E3779B97F4A7C15ull;

// keys[i] as above.  digests: 32 B per row, 16-B aligned.  rep may be NULL.  n > 0.
hipError_t exact_keys(const uint32_t* rep, const uint8_t* digests, uint64_t n, uint64_t* keys,
                      hipStream_t s);
// *mismatched += the rows i with head[i] != i whose (rep, digest) differs from row head[i]'s
// (a head[i] > i counts too and is never used as an index).  after_words: the debug build
// reports every such row as an invariant violation.  n > 0.
hipError_t exact_verify(const uint32_t* rep, const uint8_t* digests, const uint32_t* head, uint64_t n,
                        uint32_t* mismatched, bool after_words, hipStream_t s);
// the word-wise path: keys[i] = le64(digest[i][8 w .. 8 w + 8)), w in 0..3
hipError_t exact_word_keys(const uint8_t* digests, uint32_t w, uint64_t n, uint64_t* keys, hipStream_t s);
// keys[i] = (cls ? cls[i] : 0) << 32 | ids[i]
hipError_t exact_pair_keys(const uint32_t* cls, const uint32_t* ids, uint64_t n, uint64_t* keys,
                           hipStream_t s);
// the host report: full[rows[j]] = rows[rep_c[j]] for j < m (rep_c[j] <= j < m)
hipError_t exact_scatter(const uint32_t* rep_c, const uint32_t* rows, uint64_t m, uint32_t* full,
                         hipStream_t s);

}  // namespace sdcas
