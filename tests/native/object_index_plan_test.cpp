// object_index_plan_test.cpp — the Object index's size decisions (sd_object_index_plan.h) as pure
// functions: table sizes, when the host's bound trips, and what the exact counts then decide.
// Stand-alone host program (tests/test_index_cases_cpu.py compiles and runs it).
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "sd_object_index_plan.h"

using namespace sdcas;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// the insert path of object_index_host.cpp over counts alone
struct Sim {
  uint64_t slots, live = 0, tombs = 0, bound = 0, rehashes = 0, reads = 0;
  uint32_t pct;
  Sim(uint64_t expected, uint32_t p) : slots(index_slots_for(expected, p)), pct(p) {}
  // n keys of which `fresh` are new
  void insert(uint64_t n, uint64_t fresh) {
    if (index_bound_trips(slots, bound, n, pct)) {
      ++reads;
      const uint64_t t = index_rehash_slots(slots, live, tombs, n, pct);
      CHECK(t != ~0ull);
      if (t) {
        CHECK(t >= slots && (t & (t - 1)) == 0);
        slots = t;  tombs = 0;  bound = live;  ++rehashes;
      } else {
        bound = live + tombs;
      }
    }
    bound += n;
    live += fresh;
    CHECK(live + tombs <= bound);                        // the bound is one
    CHECK(bound <= index_capacity(slots, pct));          // and an insert never passes the load
    CHECK(live + tombs < slots);                         // so a probe always meets an empty slot
  }
  void erase(uint64_t gone) { live -= gone;  tombs += gone; }
};

int main() {
  for (uint32_t pct : {30u, 50u, 70u, INDEX_LOAD_PERCENT}) {
    CHECK(index_slots_for(0, pct) == INDEX_MIN_SLOTS);
    CHECK(index_capacity(INDEX_MIN_SLOTS, pct) == INDEX_MIN_SLOTS * pct / 100);
    for (uint64_t e : {1ull, 307ull, 308ull, 512ull, 513ull, 717ull, 10000000ull, 1ull << 33}) {
      const uint64_t s = index_slots_for(e, pct);
      CHECK(s >= INDEX_MIN_SLOTS && (s & (s - 1)) == 0 && index_capacity(s, pct) >= e);
      CHECK(s == INDEX_MIN_SLOTS || index_capacity(s / 2, pct) < e);
      CHECK((1ull << index_log2(s)) == s);
    }
    CHECK(index_slots_for(~0ull, pct) == 0);
    CHECK(index_rehash_slots(INDEX_MIN_SLOTS, 0, 0, ~0ull >> 1, pct) == ~0ull);

    // growth: 5,000 distinct keys in batches of 1, 63, 64, 65 and 1,000
    Sim g(0, pct);
    const uint64_t batch[5] = {1, 63, 64, 65, 1000};
    for (uint64_t done = 0, k = 0; done < 5000; ++k) {
      const uint64_t n = batch[k % 5] < 5000 - done ? batch[k % 5] : 5000 - done;
      g.insert(n, n);
      done += n;
    }
    CHECK(g.live == 5000 && g.rehashes >= 3 && g.slots == index_slots_for(5000, pct));
    CHECK(g.reads == g.rehashes);  // distinct keys: the bound is exact, every read rehashes

    // keys already present make the bound loose: a read, no rehash
    Sim d(0, pct);
    const uint64_t cap = index_capacity(d.slots, pct);
    d.insert(cap / 2, cap / 2);
    d.insert(cap / 2, 0);
    d.insert(cap / 2, 0);
    CHECK(d.reads == 1 && d.rehashes == 0 && d.slots == INDEX_MIN_SLOTS);
    // ... and a batch that trips the bound while carrying present keys grows for all of it
    d.insert(cap, cap / 4);
    CHECK(d.rehashes == 1 && d.slots == 2 * INDEX_MIN_SLOTS);

    // compaction: ten cycles of insert 600 / erase 600 end no larger than the first cycle left it
    Sim c(0, pct);
    c.insert(600, 600);
    const uint64_t after_first = c.slots;
    c.erase(600);
    for (int k = 1; k < 10; ++k) {
      c.insert(600, 600);
      c.erase(600);
    }
    CHECK(c.slots == after_first && c.slots <= 2 * INDEX_MIN_SLOTS && c.live == 0);
    CHECK(c.rehashes >= 2);
  }
  printf("object_index_plan ok\n");
  return 0;
}
