// sd_object_index.h — launchers of the library-resident Object index kernels (object_index.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdcas {

// One slot of the open-addressing table.  A cleared slot is all ones: key word INDEX_EMPTY and id
// 0xFFFFFFFF, so an insert's minimum needs no ordering against the claim of the key word.
struct IndexSlot { uint64_t key; uint32_t id; uint32_t pad; };
static_assert(sizeof(IndexSlot) == 16, "slot");
// The two key words that are not keys.  The real keys of these values live in the two side ids
// of the counter block instead of the table, so no u64 is refused.
constexpr uint64_t INDEX_EMPTY = ~0ull;
constexpr uint64_t INDEX_TOMB = ~0ull - 1;
constexpr uint32_t INDEX_NO_ID = 0xFFFFFFFFu;

// An index's counter block (u64 words, device): live entries (side keys included), tombstones,
// the longest probe sequence as op << 32 | slots examined (a later op's word is larger, so no
// call zeroes it), a flag set by a probe that ran round the whole table (the host's load bound
// keeps that from happening), export's cursor, insert's bad-id count, and the side ids (two u32:
// the id of key INDEX_EMPTY, the id of key INDEX_TOMB; INDEX_NO_ID = absent).
enum : uint32_t {
  INDEX_CTR_ENTRIES = 0, INDEX_CTR_TOMBS = 1, INDEX_CTR_PROBE = 2, INDEX_CTR_FULL = 3,
  INDEX_CTR_EXPORT = 4, INDEX_CTR_BAD = 5, INDEX_CTR_SIDE = 6, INDEX_CTR_WORDS = 8
};

struct IndexTable {
  IndexSlot* slots;
  uint64_t* ctr;
  uint32_t log2_slots;  // home(key) = mix64(key) >> (64 - log2_slots)
};

// table[key] = min(table[key], id) for every pair; new keys claim the first empty slot of their
// probe sequence (tombstones are never reused: keys stay unique)
hipError_t index_insert(IndexTable t, const uint64_t* keys, const uint32_t* ids, uint64_t n, uint32_t op,
                        hipStream_t s);
// out[i] = the id of keys[i] or INDEX_NO_ID; min_into: out[i] = min(out[i], that)
hipError_t index_lookup(IndexTable t, const uint64_t* keys, uint64_t n, uint32_t* out, bool min_into,
                        uint32_t op, hipStream_t s);
// the keys' slots become tombstones
hipError_t index_erase(IndexTable t, const uint64_t* keys, uint64_t n, uint32_t op, hipStream_t s);
// every live slot of `from` into `to` (cleared, with room: same counter block)
hipError_t index_rehash(IndexTable from, IndexTable to, hipStream_t s);
// the live pairs, side keys included, in any order; ctr[INDEX_CTR_EXPORT] (zeroed by the caller)
// counts them, and a pair whose position is not below cap is not written
hipError_t index_export(IndexTable t, uint64_t* keys, uint32_t* ids, uint64_t cap, hipStream_t s);

}  // namespace sdcas
