// sd_object_index_plan.h — the size decisions of the library-resident Object index
// (object_index.hip, object_index_host.cpp): how many slots a table gets, when an insert has to
// look at the exact device counts, and whether it then grows the table, compacts it at its size
// or goes on.  Host only, no HIP include (tests/native/object_index_plan_test.cpp).
#pragma once
#include <stdint.h>

namespace sdcas {

constexpr uint64_t INDEX_MIN_SLOTS = 1024;  // expected_entries == 0
constexpr uint64_t INDEX_MAX_SLOTS = 1ull << 36;  // 1 TiB of slots; one lane per slot fits a grid
// maximum load (live keys + tombstones over slots), in percent.  Measured at 10 M keys
// (profiles/object_index/README.md): 30 and 50 choose the same 512-MiB table, lookup 1.83 ms; 70
// halves it for 1.85 ms.  The best lookup time under 1 GiB, and no larger a table than it needs.
constexpr uint32_t INDEX_LOAD_PERCENT = 50;

// the slots an insert may use (live + tombstones) before the table is rehashed
inline uint64_t index_capacity(uint64_t slots, uint32_t percent) { return slots / 100 * percent + slots % 100 * percent / 100; }

// the smallest power-of-two table, at least INDEX_MIN_SLOTS, that holds `entries` under the load;
// 0 when none up to INDEX_MAX_SLOTS does
inline uint64_t index_slots_for(uint64_t entries, uint32_t percent) {
  for (uint64_t s = INDEX_MIN_SLOTS; s <= INDEX_MAX_SLOTS; s <<= 1)
    if (index_capacity(s, percent) >= entries) return s;
  return 0;
}
inline uint32_t index_log2(uint64_t slots) {
  uint32_t l = 0;
  while ((1ull << l) < slots) ++l;
  return l;
}

// The host keeps an upper bound of the used slots (every key ever handed to insert since the last
// exact count, repeats and keys already present included), so that an insert reads nothing back
// while the bound stays under the load.
inline bool index_bound_trips(uint64_t slots, uint64_t used_bound, uint64_t n, uint32_t percent) {
  return used_bound + n > index_capacity(slots, percent);
}
// The bound tripped and the exact counts were read: the table size to rehash into, or 0 to go on
// with the table as it is (the bound was loose).  live + n past the load: grow; live + tombstones
// + n past it: tombstones are what filled the table, same size; ~0 when no table can hold it.
inline uint64_t index_rehash_slots(uint64_t slots, uint64_t live, uint64_t tombstones, uint64_t n,
                                   uint32_t percent) {
  const uint64_t cap = index_capacity(slots, percent);
  if (live + n > cap) {
    const uint64_t s = index_slots_for(live + n, percent);
    return s ? s : ~0ull;
  }
  return live + tombstones + n > cap ? slots : 0;
}

}  // namespace sdcas
