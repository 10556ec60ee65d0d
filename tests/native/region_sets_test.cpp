// Host test of sd_region_sets.h (a stand-alone program; tests/test_region_sets_cpu.py builds it
// plain and with -fsanitize=address,undefined).  The fused chain's three entry points are replayed
// as pure transitions: Chain performs each decision on a model of what the device holds (are a
// set's cursors clean, which count lies in a set's counter and which in d_scalar) and logs the
// waits, in the order group_host.cpp performs them.  The call sequences are those of the GPU tests
// test_hash_regions_split_pipelined, test_hash_regions_streams_and_ungrouped and
// test_alternating_region_sets_then_group_regions.
#include <stdint.h>
#include <stdio.h>

#include "sd_region_sets.h"

using sdcas::RegionSets;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Chain {
  RegionSets sets;
  bool dirty[2] = {false, false};  // set k's cursors and spill count are counted (not zero)
  uint64_t counter[2] = {0, 0};    // set k's Object counter
  uint64_t scalar = 0;             // d_scalar[0]
  uint64_t keys[4] = {0, 0, 0, 0};
  RegionSets::Refill last{};       // the decisions of the last hash_regions call
  int rescues = 0;

  // sd_cas_hash_regions_sampled_dev; k1g_ok = false: the enqueue fails
  bool hash_regions(uint64_t n, bool k1g_ok = true) {
    const RegionSets::Refill f = last = sets.next_refill();
    const int k = f.set;
    if (f.wait_hashed) dirty[k] = false;  // wait for `hashed`, clear
    if (f.rescue) {
      scalar = counter[k];
      sets.objects_in_scalar();
      ++rescues;
    }
    CHECK(!dirty[k]);  // K1G starts on clean cursors
    if (!k1g_ok) return false;  // (the entry point clears the cursors again: they are clean)
    dirty[k] = true;
    counter[k] = 0;  // K1G zeroes the counter
    sets.hashed(k, n, keys);
    return true;
  }
  // sd_cas_group_regions_dev; objects: what the tables count
  bool group_regions(uint64_t n, uint64_t objects) {
    if (!sets.can_group(n)) return false;
    const int k = sets.cur;
    CHECK(dirty[k] && sets.keys[k] == keys);
    dirty[k] = false;  // the tables re-zero
    counter[k] = objects;
    sets.tables_enqueued();
    return true;
  }
  // a standalone grouping (sd_cas_group_dev and the others)
  void group(uint64_t objects) {
    scalar = objects;
    sets.objects_in_scalar();
  }
  // sd_cas_copy_objects_dev
  uint64_t copy_objects() const { return sets.objects_set >= 0 ? counter[sets.objects_set] : scalar; }
};

static bool waits(const RegionSets::Refill& f, int set, bool done, bool hashed, bool rescue) {
  return f.set == set && f.wait_done == done && f.wait_hashed == hashed && f.rescue == rescue;
}
static bool same(const RegionSets::Refill& a, const RegionSets::Refill& b) {
  return waits(a, b.set, b.wait_done, b.wait_hashed, b.rescue);
}

// batch j of 4 on the main stream, its tables and copy_objects on a side stream; batch 1 is
// hashed and never grouped
static void split_pipelined() {
  Chain c;
  const uint64_t n = 2 * 65536;
  CHECK(!c.group_regions(n, 1));  // before any batch
  CHECK(c.hash_regions(n) && waits(c.last, 0, false, false, false));  // a fresh context: no waits
  CHECK(c.group_regions(n, 100) && c.sets.objects_set == 0 && c.copy_objects() == 100);
  CHECK(c.hash_regions(n) && waits(c.last, 1, false, false, false));
  // set 0's tables were enqueued: only after `done`; it holds batch 0's count: rescued
  CHECK(c.hash_regions(n) && waits(c.last, 0, true, false, true));
  CHECK(c.sets.objects_set == -1 && c.copy_objects() == 100 && c.rescues == 1);
  CHECK(c.group_regions(n, 102) && c.sets.objects_set == 0 && c.copy_objects() == 102);
  // set 1 was hashed, never grouped: after its own K1G and a clear; it never ran tables
  CHECK(c.hash_regions(n) && waits(c.last, 1, false, true, false));
  CHECK(c.dirty[1] && c.rescues == 1);
  CHECK(c.group_regions(n, 103) && c.sets.objects_set == 1 && c.copy_objects() == 103);
  CHECK(!c.group_regions(n, 103));  // the last batch is grouped already
  CHECK(!c.dirty[0] && !c.dirty[1]);
  c.group(7);  // any standalone grouping: the count is d_scalar's
  CHECK(c.sets.objects_set == -1 && c.copy_objects() == 7);
  CHECK(!c.group_regions(n, 103));
}

// five batches, grouped T F T T T, then further refills that are never grouped: the last
// grouping's count survives the refill of its set
static void streams_and_ungrouped() {
  Chain c;
  const uint64_t n = 65536;
  CHECK(c.hash_regions(n) && waits(c.last, 0, false, false, false) && c.group_regions(n, 200));
  CHECK(c.hash_regions(n) && waits(c.last, 1, false, false, false));  // never grouped
  CHECK(c.hash_regions(n) && waits(c.last, 0, true, false, true) && c.copy_objects() == 200);
  CHECK(c.group_regions(n, 202) && c.copy_objects() == 202);
  CHECK(c.hash_regions(n) && waits(c.last, 1, false, true, false));  // batch 1's K1G may still run
  CHECK(c.sets.objects_set == 0 && c.group_regions(n, 203) && c.sets.objects_set == 1);
  CHECK(c.hash_regions(n) && waits(c.last, 0, true, false, false));  // the count is set 1's
  CHECK(c.group_regions(n, 204) && c.sets.objects_set == 0 && c.copy_objects() == 204);
  const int before = c.rescues;
  CHECK(c.hash_regions(n) && waits(c.last, 1, true, false, false) && c.sets.objects_set == 0);
  CHECK(c.hash_regions(n) && waits(c.last, 0, true, false, true));  // batch 4's set: the rescue
  CHECK(c.sets.objects_set == -1 && c.copy_objects() == 204);
  // two further ungrouped refills leave it in d_scalar; each waits for the K1G it replaces
  CHECK(c.hash_regions(n) && waits(c.last, 1, true, true, false));
  CHECK(c.hash_regions(n) && waits(c.last, 0, true, true, false));
  CHECK(c.rescues == before + 1 && c.sets.objects_set == -1 && c.copy_objects() == 204);
  CHECK(!c.group_regions(2 * n, 1));  // another n
  CHECK(c.group_regions(n, 209) && c.copy_objects() == 209);
}

// set A, set B on another stream (A dropped ungrouped), B's tables, A again and its tables
static void alternating_then_group() {
  Chain c;
  const uint64_t n = 65536;
  CHECK(c.hash_regions(n) && waits(c.last, 0, false, false, false));
  CHECK(c.hash_regions(n) && waits(c.last, 1, false, false, false));
  CHECK(c.group_regions(n, 301) && c.sets.objects_set == 1);
  CHECK(!c.group_regions(n, 301));  // twice for the same batch
  CHECK(c.hash_regions(n) && waits(c.last, 0, false, true, false) && c.copy_objects() == 301);
  CHECK(c.group_regions(n, 300) && c.sets.objects_set == 0 && c.copy_objects() == 300);
}

// a K1G enqueue that fails: every decision afterwards is the one from before the call (the Object
// count, if the refill rescued it, has moved to d_scalar with its value)
static void failed_refill() {
  for (int rescue = 0; rescue < 2; ++rescue)
    for (int ungrouped = 0; ungrouped < 2; ++ungrouped) {
      Chain c;
      const uint64_t n = 65536;
      // set 0: grouped (it holds the count) or a standalone grouping after it; set 1: grouped or not
      CHECK(c.hash_regions(n) && c.group_regions(n, 400));
      if (!rescue) c.group(9);
      CHECK(c.hash_regions(n) && (ungrouped || c.group_regions(n, 401)));
      if (!ungrouped) c.group(9);  // (the count away from set 1, so that set 0's case is the one tested)
      if (rescue && !ungrouped) continue;  // set 0 cannot hold the count then
      const RegionSets::Refill want = c.sets.next_refill();
      const uint64_t count = c.copy_objects();
      const bool could = c.sets.can_group(n);
      CHECK(want.set == 0 && want.wait_done && !want.wait_hashed && want.rescue == (rescue != 0));
      CHECK(could == (ungrouped != 0));
      CHECK(!c.hash_regions(n, false));
      RegionSets::Refill now = c.sets.next_refill();
      CHECK(now.rescue == false && c.copy_objects() == count);
      now.rescue = want.rescue;
      CHECK(same(now, want) && c.sets.cur == 1 && c.sets.can_group(n) == could);
      // after the failed refill of set 0, set 1's batch is still the last one: grouped already ->
      // refused; still ungrouped -> its tables run
      CHECK(c.group_regions(n, 402) == could);
      CHECK(c.hash_regions(n) && c.last.set == 0 && !c.last.rescue && c.dirty[0]);
    }
  // the same with the failing refill going into a set that was hashed and never grouped: the wait
  // for its K1G and the clear are asked for again
  Chain c;
  const uint64_t n = 65536;
  CHECK(c.hash_regions(n) && c.hash_regions(n) && c.group_regions(n, 500));
  CHECK(!c.hash_regions(n, false) && waits(c.last, 0, false, true, false) && !c.dirty[0]);
  CHECK(waits(c.sets.next_refill(), 0, false, true, false) && c.copy_objects() == 500);
  CHECK(!c.group_regions(n, 501));  // set 1's batch is grouped already
  CHECK(c.hash_regions(n) && c.group_regions(n, 502) && c.copy_objects() == 502);
}

int main() {
  split_pipelined();
  streams_and_ungrouped();
  alternating_then_group();
  failed_refill();
  if (fails) return 1;
  printf("region_sets ok\n");
  return 0;
}
