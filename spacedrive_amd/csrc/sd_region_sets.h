// sd_region_sets.h — the decisions of the fused hash + group chain's two region sets
// (group_host.cpp: sd_cas_hash_regions_sampled_dev, sd_cas_group_regions_dev,
// sd_cas_copy_objects_dev).  Plain host arithmetic over a few flags and no HIP, so a host program
// replays the callers' sequences (tests/native/region_sets_test.cpp); the entry points perform the
// waits, memsets and copies these decisions name, on the events and buffers the context keeps
// beside this state (RegionChain, ctx_internal.h).
//
// The sets are used alternately, so set k's bucket tables can run on a side stream while the next
// batch's K1G fills set k^1.  Per set: `hashed` is recorded after its K1G, `done` after its tables.
#pragma once
#include <stdint.h>

namespace sdcas {

struct RegionSets {
  uint64_t n[2] = {0, 0};                        // files of the batch last hashed into set k
  const uint64_t* keys[2] = {nullptr, nullptr};  // that batch's keys (an overflowed region's regroup)
  bool pending[2] = {false, false};              // set k's tables have been enqueued at least once
  bool grouped[2] = {true, true};                // ... and since its last K1G
  int cur = -1;                                  // the last batch's set (-1: no batch yet)
  // The Object count of the context's last grouping is what sd_cas_copy_objects_dev copies: it
  // lies in this set's counter, or in d_scalar (-1).
  int objects_set = -1;

  // What a hash_regions call does to the set it refills before its K1G, in this order.
  struct Refill {
    int set;
    bool wait_done;    // grouped two batches ago: its tables (`done`) must have finished
    bool wait_hashed;  // hashed, never grouped: after that K1G (`hashed`, whatever its stream),
                       // clear the set's cursors and spill count, which it left counted
    bool rescue;       // the set holds the Object count, which K1G zeroes: to d_scalar first
  };
  Refill next_refill() const {
    const int k = (cur + 1) & 1;
    return {k, pending[k], !grouped[k], objects_set == k};
  }
  // the count now lies in d_scalar: the refill's rescue copy, or any standalone grouping
  void objects_in_scalar() { objects_set = -1; }
  // set k's K1G has been enqueued (a refill that fails before this commits nothing)
  void hashed(int k, uint64_t files, const uint64_t* batch_keys) {
    n[k] = files;
    keys[k] = batch_keys;
    cur = k;
    grouped[k] = false;
  }
  // group_regions(files) runs only on the last batch, once, and with that batch's size
  bool can_group(uint64_t files) const { return cur >= 0 && !grouped[cur] && n[cur] == files; }
  // the last batch's tables have been enqueued: its set now holds the Object count
  void tables_enqueued() {
    pending[cur] = grouped[cur] = true;
    objects_set = cur;
  }
};

}  // namespace sdcas
