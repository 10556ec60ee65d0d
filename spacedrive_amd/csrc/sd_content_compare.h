// sd_content_compare.h — launchers of the whole-content compare's kernels (content_compare.hip)
// and its workspace layout (reports_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sd_content_tasks.h"

namespace sdcas {

// the counter block of one call (u32 words; CT_QUEUE is the compare kernel's task queue)
constexpr uint32_t CT_BAD = 0, CT_UNEQUAL = 1, CT_UNRESOLVED = 2, CT_OVERFLOW = 3, CT_QUEUE = 4,
                   CT_MARKED = 5, CT_COUNTERS = 64;

// The workspace of sd_cas_group_exact_contents_dev for n rows (c->contents).  Entry lists are
// (key, row) pairs, key = the row's pivot, or n for a resolved row (it sorts last).
struct ContentCompareWs {
  uint64_t* keys;                     // the class grouping's pair keys; the digest finish's sort keys
  uint32_t *ids, *cls;                // the length grouping; each row's class (its first row)
  uint64_t *ekey_in, *ekey;           // the entry list as the resolve pass leaves it / sorted by pivot
  uint32_t *erow_in, *erow;
  uint32_t *neq, *slot;               // per row: refuted by its pivot; per pivot: its smallest unequal row
  uint32_t *wpieces, *wstart, *scan;  // per window: pieces, their exclusive scan; the scan's scratch
  unsigned long long* tasks;          // the scan's total
  uint32_t* counters;                 // CT_COUNTERS words
  uint32_t *pval, *order, *cpiv, *crep;  // the digest finish: pivot value per row, the compacted rows
  uint64_t *coffs, *clens, *skeys;
  uint8_t* cdig;
  size_t bytes;
};
extern "C" ContentCompareWs sd_content_compare_layout(void* base, size_t n);

// counters[CT_BAD] |= 1 for a content over 64 GiB, 4 for one misaligned or not within arena_bytes
// (the checksum batch chain's flags).  Zeroes the counter block first.  n > 0.
hipError_t ct_check_bounds(uint64_t arena_bytes, const uint64_t* offs, const uint64_t* lens, uint64_t n,
                           uint32_t* counters, hipStream_t s);
// The first list: row i with cls[i] == i is a head (rep_exact[i] = i, key n), any other row an
// entry with pivot cls[i].  Clears neq.
hipError_t ct_first_entries(const uint32_t* cls, uint64_t n, uint32_t* rep_exact, uint64_t* ekey_in,
                            uint32_t* erow_in, uint32_t* neq, hipStream_t s);
// One round over the m live entries of the sorted list (ekey, erow): window pieces and their scan,
// the compare (grid workgroups of 256), then the two resolve passes, which write the next list
// into (ekey_in, erow_in), add the unequal entries to counters[CT_UNEQUAL] and leave the entries
// still unresolved in counters[CT_UNRESOLVED].  A round of 2^32 tasks or more sets
// counters[CT_OVERFLOW] and changes nothing else.
hipError_t ct_round(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens, uint64_t n,
                    uint32_t m, const ContentCompareWs& L, uint32_t* rep_exact, uint32_t grid,
                    hipStream_t s);
// The digest finish's rows: pval[r] = the pivot of live entry r and pval[p] = p for its pivot
// (pval preset to 0xFF), then skeys[i] = 0 where pval[i] is set, 1 elsewhere, and
// counters[CT_MARKED] = the rows set.
hipError_t ct_mark(const ContentCompareWs& L, uint32_t m, uint64_t n, hipStream_t s);
// coffs / clens / cpiv of the marked rows order[0 .. marked)
hipError_t ct_gather(const ContentCompareWs& L, const uint64_t* offs, const uint64_t* lens,
                     uint32_t marked, hipStream_t s);
// *d_objects = the rows with rep_exact[i] == i.  The debug build counts a violation for a row with
// rep_exact[i] > i or whose rep_exact row is not a head of its class (rep value, length).
hipError_t ct_count_heads(const uint32_t* rep, const uint64_t* lens, const uint32_t* rep_exact, uint64_t n,
                          uint64_t* d_objects, hipStream_t s);

}  // namespace sdcas
