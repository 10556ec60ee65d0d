// ws_layout_test.cpp — the workspace layouts of libsd_hip_cas.so, printed for
// tests/test_ws_layout_cpu.py.  Host only: it calls the pure size / layout functions, never
// the GPU.  Two kinds of line:
//   S <key> <value>                      a *_workspace_bytes total (or an input of one)
//   L <key> <total> <wrapper> m:off:need ...
//                                        a layout carved at a dummy base: every member's offset
//                                        and the bytes its launcher indexes there (a member
//                                        printed as name:-:0 is an absent section); <wrapper> is
//                                        the layout's *_workspace_bytes function, or - where it
//                                        has none (its total is pinned by the golden file alone)
// With -DWS_SIZES_ONLY only the S lines are compiled: those functions exist unchanged in older
// builds of the library, whose totals tests/golden/ws_sizes.json records.
#include <stdio.h>

#include <algorithm>

#include "ctx_internal.h"
#include "sd_checksum.h"
#include "sd_dup_runs.h"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_links.h"
#include "sd_mix.h"
#include "sd_object_stats.h"

using namespace sdcas;

static const uint64_t NS[] = {1, 255, 256, 257, 4095, 4096, 4097, 65536, 1441792, 1441793,
                              12500000, 40000001, 4294967295ull};
static const uint64_t TARGETS[] = {0, 1, 16};
static const uint64_t CK_NS[] = {1, 65535, 65536};
static const uint64_t ARENAS[] = {0, 1ull << 20, 64ull << 30};
static const uint32_t PARTS[] = {1, 1023, 1024, 16384};

static void S(const char* name, uint64_t a, uint64_t b, int nargs, uint64_t v) {
  if (nargs == 1) printf("S %s(%llu) %llu\n", name, (unsigned long long)a, (unsigned long long)v);
  else printf("S %s(%llu,%llu) %llu\n", name, (unsigned long long)a, (unsigned long long)b, (unsigned long long)v);
}

static void sizes() {
  sd_cas_ctx ctx;  // (never touches a device: sd_packed_workspace_bytes reads two thresholds)
  for (uint64_t n : NS) {
    S("sort_workspace_bytes", n, 0, 1, sort_workspace_bytes(n));
    S("group_workspace_bytes", n, 0, 1, group_workspace_bytes(n));
    S("group_min_sorted_workspace_bytes", n, 0, 1, group_min_sorted_workspace_bytes(n));
    for (uint64_t t : TARGETS) S("hash_group_workspace_bytes", n, t, 2, hash_group_workspace_bytes(n, t));
    S("region_group_workspace_bytes", n, 0, 1, region_group_workspace_bytes(n));
    S("region_capacity", n, 0, 1, region_capacity(n));
    S("checksum_workspace_bytes", n, 0, 1, checksum_workspace_bytes(n));
    S("inplace_workspace_bytes", n, 0, 1, inplace_workspace_bytes(n));
    S("sd_packed_workspace_bytes", n, 0, 1, sd_packed_workspace_bytes(&ctx, n));
    S("pre_blocks", n, 0, 1, pre_blocks(n));
    S("segmin_tiles_bytes", n, 0, 1, segmin_tiles_bytes(n));
    S("top_scan_bytes", n, 0, 1, top_scan_bytes(n));
  }
  for (uint64_t len : {(uint64_t)0, (uint64_t)1 << 20, ((uint64_t)1 << 20) + 1, (uint64_t)64 << 30})
    S("checksum_workspace_bytes", len, 0, 1, checksum_workspace_bytes(len));
  for (uint32_t p : PARTS) S("partition_workspace_bytes", 4097, p, 2, partition_workspace_bytes(4097, p));
  for (uint64_t n : CK_NS)
    for (uint64_t a : ARENAS) S("checksum_batch_workspace_bytes", n, a, 2, checksum_batch_workspace_bytes(n, a));
  S("pre_filter_bytes", 0, 0, 1, pre_filter_bytes());
  S("stats_shard_bytes", 0, 0, 1, stats_shard_bytes());
}

#ifndef WS_SIZES_ONLY
static char* const BASE = (char*)((uintptr_t)1 << 44);  // never dereferenced

struct Line {
  Line(const char* key, size_t total, size_t wrapper) {
    printf("L %s %llu %llu", key, (unsigned long long)total, (unsigned long long)wrapper);
  }
  Line(const char* key, size_t total) { printf("L %s %llu -", key, (unsigned long long)total); }
  ~Line() { printf("\n"); }
  Line& m(const char* name, const void* p, long long need) {
    if (!p) printf(" %s:-:0", name);
    else printf(" %s:%llu:%lld", name, (unsigned long long)((const char*)p - BASE), need);
    return *this;
  }
};
#define M(x, need) m(#x, L.x, (long long)(need))

static uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// What hash_group_min's kernels index, restated from group_hash.hip (group_plan, totals_repl,
// region_capacity_nb and their constants): nb1 coarse buckets, nb final buckets, repl
// interleaved copies of the coarse totals, 64 Object-count shards of 16 u64.
struct HashPlan { uint64_t nb1, nb, repl; };
static HashPlan hash_plan(uint64_t n, uint64_t target) {
  if (target == 0) target = 1536;
  uint32_t bits = 1;
  while (bits < 19 && ((uint64_t)1 << bits) * target < n) ++bits;
  const uint32_t cb = n <= 40000000 ? 8u : 10u;
  const uint32_t b1 = bits < cb ? bits : (bits - cb > 9 ? bits - 9 : cb);
  uint32_t b2 = bits - b1;
  if (b2 > 0 && n <= 256ull * 5632) b2 = 0;  // coarse buckets straight to the big tables
  const uint64_t nb1 = (uint64_t)1 << b1;
  return {nb1, (uint64_t)1 << (b1 + b2), nb1 <= 1024 ? 16u : 1u};
}
static uint64_t capacity_nb(uint64_t n, uint64_t nb) {  // mean + 8 sd (binomial) + 64 rows
  const double mean = (double)n / nb, var = mean * (1.0 - 1.0 / nb);
  uint64_t sd = 1;
  while ((double)(sd * sd) < var) ++sd;
  return (uint64_t)mean + 1 + 8 * sd + 64;
}
constexpr uint64_t SHARD_BYTES = 64 * 16 * 8;

static void layouts() {
  char key[128];
  sd_cas_ctx ctx;
  for (uint64_t n : NS) {
    const unsigned long long un = n;
    {
      // 4,096-key sort tiles, 256 digits, upsweep blocks of 4 tiles; 4,096-key run tiles
      const uint64_t nt = ceil_div(n, 4096), nb = ceil_div(nt, 4);
      const SortWs L = sort_layout(BASE, n);
      snprintf(key, sizeof key, "sort(%llu)", un);
      Line(key, L.bytes, sort_workspace_bytes(n)).M(kalt, n * 8).M(valt, n * 4).M(hist, 256 * nt * 4)
          .M(bsum, 256 * nb * 4).M(rowtot, 256 * 4);
    }
    {
      const GroupWs L = group_layout(BASE, n);
      snprintf(key, sizeof key, "group(%llu)", un);
      Line(key, L.bytes, group_workspace_bytes(n)).M(sort_ws, sort_workspace_bytes(n)).M(skeys, n * 8)
          .M(svals, n * 4).M(heads, ceil_div(n, 4096) * 4);
    }
    {
      const GroupMinSortedWs L = group_min_sorted_layout(BASE, n);
      snprintf(key, sizeof key, "group_min_sorted(%llu)", un);
      Line(key, L.bytes, group_min_sorted_workspace_bytes(n)).M(gws, group_workspace_bytes(n)).M(vkey, n * 8)
          .M(k2, n * 8).M(skeys, n * 8).M(order, n * 4).M(spos, n * 4).M(rep, n * 4);
    }
    const uint64_t rows = (uint64_t)REGIONS * region_capacity(n);
    {
      const RegionGroupWs L = region_group_layout(BASE, n);
      snprintf(key, sizeof key, "region_group(%llu)", un);
      Line(key, L.bytes, region_group_workspace_bytes(n)).M(rkeys, rows * 8).M(rfile, rows * 4)
          .M(gkeys, 2 * rows * 8).M(gvals, 2 * rows * 4).M(spill_keys, n * 8).M(spill_file, n * 4)
          .M(objects, 16);
    }
    {
      const SmallRegionsWs L = small_regions_layout(BASE, n);
      snprintf(key, sizeof key, "small_regions(%llu)", un);
      Line(key, L.bytes).M(rkeys, rows * 8).M(rfile, rows * 4).M(gkeys, 2 * n * 8)
          .M(gvals, 2 * n * 4).M(spill, 8).M(skeys, n * 8).M(sfile, n * 4);
    }
    {
      const BigRegionsWs L = big_regions_layout(BASE, n);
      const HashPlan g = hash_plan(n, 0);
      const uint64_t brows = g.nb1 * capacity_nb(n, g.nb1);
      snprintf(key, sizeof key, "big_regions(%llu)", un);
      Line(key, L.bytes).M(rkeys, brows * 8).M(rfile, brows * 4).M(skeys, n * 8).M(spos, n * 4).M(k2, n * 8)
          .M(p2, n * 4).M(starts, g.nb * 4).M(shards, SHARD_BYTES).M(gkeys, 2 * n * 8).M(gvals, 2 * n * 4);
    }
    for (uint64_t t : TARGETS) {
      const HashChainWs L = hash_chain_layout(BASE, n, t);
      snprintf(key, sizeof key, "hash_chain(%llu,%llu)", un, (unsigned long long)t);
      const HashPlan g = hash_plan(n, t);
      Line(key, L.bytes).M(k1, n * 8).M(p1, n * 4).M(k2, n * 8).M(p2, n * 4).M(fill, g.repl * g.nb1 * 4)
          .M(starts1, g.nb1 * 4).M(starts, g.nb * 4).M(shards, SHARD_BYTES).M(gkeys, 2 * n * 8)
          .M(gvals, 2 * n * 4);
      // the wrapper: this chain, or the larger of it and the region chain hash_group_min may
      // pick instead (the default target only)
      const size_t w = hash_group_workspace_bytes(n, t), sm = small_regions_layout(nullptr, n).bytes,
                   bg = big_regions_layout(nullptr, n).bytes;
      printf("S hash_group_is_max(%llu,%llu) %d\n", un, (unsigned long long)t,
             (int)(w == L.bytes || (t == 0 && (w == std::max(L.bytes, sm) || w == std::max(L.bytes, bg)))));
    }
    {
      const InplaceWs L = inplace_layout(BASE, n);
      snprintf(key, sizeof key, "inplace(%llu)", un);
      Line(key, L.bytes, inplace_workspace_bytes(n)).M(counters, 8).M(lens32, n * 4).M(sampled_idx, n * 4);
    }
    {
      // K1V: a probe and seven list words per file, exclusive_scan_u32's partial sums per 4,096
      const DupVerifyWs L = dup_verify_layout(BASE, n);
      snprintf(key, sizeof key, "dup_verify(%llu)", un);
      Line(key, L.bytes, dup_verify_workspace_bytes(n)).M(probes, n * 8).M(cand, n * 4).M(list_h, n * 4)
          .M(list_c, n * 4).M(same, n * 4).M(cnt, n * 4).M(first, n * 4).M(rank, n * 4)
          .M(partial, (n / 4096 + 1) * 4).M(counters, DUP_COUNTERS * 4).M(cu, DUP_CU_SLOTS * 4).M(objects, 8);
    }
    {
      const PackedWs L = sd_packed_layout(BASE, n);
      snprintf(key, sizeof key, "packed(%llu)", un);
      Line(key, L.bytes, sd_packed_workspace_bytes(&ctx, n)).M(lkeys, n * 8).M(skeys, n * 8).M(order, n * 4)
          .M(sort_ws, sort_workspace_bytes(n));
    }
    {
      const CvPingPong L = cv_pingpong_layout(BASE, ceil_div(n, 256));
      snprintf(key, sizeof key, "reduce_cvs(%llu)", un);
      Line(key, L.bytes, reduce_cvs_workspace_bytes(n)).M(a, ceil_div(n, 256) * 32).M(b, ceil_div(ceil_div(n, 256), 256) * 32);
    }
    for (uint64_t m : {(uint64_t)0, n}) {
      const TopWs L = sd_top_layout(BASE, n, m);
      snprintf(key, sizeof key, "top(%llu,%llu)", un, (unsigned long long)m);
      Line(key, L.bytes).M(hist, TOP_BINS * 8).M(sel, TOP_SEL_WORDS * 8).M(scan, top_scan_bytes(n))
          .M(ckeys, m * 8).M(cvals, m * 4).M(skeys, m * 8).M(svals, m * 4)
          .M(sort_ws, m ? sort_workspace_bytes(m) : 0);
    }
    for (int state = 0; state < 2; state++) {
      const size_t k = state ? 1024 : 0;
      const DupReportWs L = sd_dup_report_layout(BASE, n, state, k);
      snprintf(key, sizeof key, "dup_report(%llu,%d,%zu)", un, state, k);
      Line(key, L.bytes).M(keys, n * 8).M(sizes, n * 8).M(rep, n * 4).M(copies, n * 4).M(state, n)
          .M(hkeys, n * 8).M(hrows, n * 4).M(minrow, n * 4).M(orphans, n * 8).M(top_heads, k * 4)
          .M(top_waste, k * 8).M(counters, 16);
    }
    for (int pre = 0; pre < 2; pre++)
      for (uint64_t n_seed : {(uint64_t)0, (uint64_t)5}) {
        const uint64_t m = n + n_seed, steps = ceil_div(n, 100);
        {
          const LinkStagingWs L = sd_link_staging_layout(BASE, n, n_seed, steps, pre);
          snprintf(key, sizeof key, "link_staging(%llu,%llu,%llu,%d)", un, (unsigned long long)n_seed,
                   (unsigned long long)steps, pre);
          Line(key, L.bytes).M(rep, n * 4).M(hkeys, m * 8).M(hrows, m * 4).M(minrow, m * 4)
              .M(orphans, n * 8).M(starts, (steps + 1) * 4).M(counts, steps * 8)
              .M(boff, pre ? pre_blocks(n) * 4 : 0).M(tiles, pre ? segmin_tiles_bytes(n) : 0)
              .M(filter, pre ? pre_filter_bytes() : 0).M(counters, 32);
        }
        {
          const LinkIoWs L = sd_link_io_layout(BASE, n, n_seed, pre);
          snprintf(key, sizeof key, "link_io(%llu,%llu,%d)", un, (unsigned long long)n_seed, pre);
          Line(key, L.bytes).M(keys, n * 8).M(state, n).M(step, n * 4).M(object, n * 4).M(action, n)
              .M(seed_keys, n_seed * 8).M(seed_objects, n_seed * 4).M(pre, n * 4);
        }
      }
    for (int G : {1, 8}) {
      const uint64_t m = n / 2 + 3;
      const MultiBufs L = sd_multi_bufs_layout(BASE, n, m, G);
      snprintf(key, sizeof key, "multi_bufs(%llu,%llu,%d)", un, (unsigned long long)m, G);
      Line(key, L.bytes).M(skeys, n * 8).M(sidx, n * 4).M(gidx, n * 8).M(splits, (G + 1) * 8)
          .M(back, n * 8).M(rkeys, m * 8).M(ridx, m * 8).M(k2, m * 8).M(pos, m * 4).M(rep_pos, m * 4)
          .M(repg, m * 8);
    }
  }
  for (uint32_t parts : PARTS) {
    const PartitionWs L = partition_layout(BASE, parts);
    snprintf(key, sizeof key, "partition(%u)", parts);
    Line(key, L.bytes, partition_workspace_bytes(4097, parts)).M(totals, (parts <= 1024 ? 16 : 1) * parts * 4)
        .M(fill, (parts <= 1024 ? 16 : 1) * parts * 4);
  }
  for (uint64_t n : CK_NS)
    for (uint64_t a : ARENAS) {
      const uint64_t items = n + a / (1 << 20) + 1;  // work items: one per buffer and per MiB
      const ChecksumBatchWs L = checksum_batch_layout(BASE, n, a);
      const bool lane = L.lane_info != nullptr;
      snprintf(key, sizeof key, "checksum_batch(%llu,%llu)", (unsigned long long)n, (unsigned long long)a);
      Line(key, L.bytes, checksum_batch_workspace_bytes(n, a)).M(groups, (n + 1) * 4).M(gstart, (n + 1) * 4)
          .M(partial, (n / 4096 + 1) * 4).M(gtotal, 8).M(owner, items * 4).M(cvs, items * 32)
          .M(lane_info, 256).M(lkeys, n * 8).M(skeys, n * 8).M(order, n * 4)
          .M(sort_ws, lane ? sort_workspace_bytes(n) : 0);
      printf("S checksum_batch_lane(%llu) %d\n", (unsigned long long)n, (int)lane);
    }
  {
    const StatsWs L = sd_stats_layout(BASE);
    Line("stats()", L.bytes).M(shards, stats_shard_bytes()).M(totals, SD_CAS_STAT_COUNT * 8);
  }
  // the staged host batch: ns sampled files of 57,344 B, np whole files packed on 128-B lines
  const uint64_t shapes[][2] = {{0, 1}, {1, 0}, {100, 0}, {37, 63}};
  const uint64_t plens[] = {0, 1, 127, 128, 102400};
  for (const auto& sh : shapes)
    for (uint64_t plen : plens) {
      const uint64_t ns = sh[0], np = sh[1], n = ns + np;
      const size_t sampled_bytes = ns * 57344, packed_bytes = np * up128(plen) + 16;
      const StagedLayout L = sd_staged_layout(sampled_bytes, packed_bytes, ns, np, n);
      printf("L staged(%llu,%llu,%llu) %zu - sampled:0:%zu packed:%zu:%zu sizes:%zu:%llu poffs:%zu:%llu "
             "plens:%zu:%llu keys:%zu:%llu\n",
             (unsigned long long)ns, (unsigned long long)np, (unsigned long long)plen, L.bytes, sampled_bytes, L.packed, packed_bytes, L.sizes, (unsigned long long)n * 8, L.poffs,
             (unsigned long long)np * 8, L.plens, (unsigned long long)np * 4, L.keys, (unsigned long long)n * 8);
      printf("S staged_h2d(%llu,%llu,%llu) %d\n", (unsigned long long)ns, (unsigned long long)np,
             (unsigned long long)plen, (int)(L.h2d_bytes == L.keys));
    }
}
#endif

int main(int argc, char** argv) {
  (void)argc;
  (void)argv;
  sizes();
#ifndef WS_SIZES_ONLY
  layouts();
#endif
  return 0;
}
