// group_host.cpp — the grouping entry points of the C ABI (include/sd_hip_cas.h): the radix sort,
// the standalone Object groupings (group, group_min, group_sorted, group_chunked), the key-range
// partition, and the fused hash + group chain over two region sets (sd_region_sets.h holds its
// decisions) with its duplicate-verification counters and the asynchronous Object count.
#include "ctx_internal.h"
#include "sd_dup_runs.h"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_mix.h"

using namespace sdcas;

// The end of a standalone grouping: its use of ws is recorded, the context's Object count now lies
// in d_scalar, and a caller that asks for the count waits for it.
static int finish_grouping(sd_cas_ctx* c, WsLease& ws, hipStream_t s, uint64_t* out_objects) {
  HIP_TRY(c, ws.release());
  c->regions.sets.objects_in_scalar();
  if (out_objects) {
    HIP_TRY(c, hipMemcpyAsync(out_objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SD_CAS_OK;
}

extern "C" {

int sd_cas_sort_pairs_dev(sd_cas_ctx* c, const uint64_t* d_keys_in, const uint32_t* d_vals_in,
                          size_t n, uint64_t* d_keys_out, uint32_t* d_vals_out, int begin_bit,
                          int end_bit, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!d_keys_in || !d_keys_out || !d_vals_out || n >= (1ull << 32) || begin_bit < 0 ||
      end_bit > 64 || begin_bit >= end_bit)
    return fail(c, SD_CAS_EINVAL, "sort_pairs: bad arguments");
  int rc = ensure(c, c->ws, sort_workspace_bytes(n));
  if (rc) return rc;
  hipStream_t s = pick(c, stream);
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, radix_sort_pairs(d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, begin_bit, end_bit,
                              c->ws.p, s));
  HIP_TRY(c, ws.release());
  return SD_CAS_OK;
}

int sd_cas_group_dev(sd_cas_ctx* c, const uint64_t* d_keys, size_t n, uint32_t* d_rep,
                     uint64_t* out_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_keys || !d_rep)))
    return fail(c, SD_CAS_EINVAL, "group: bad arguments");
  if (c->group_method == SD_CAS_GROUP_HASH && !hash_group_supported(n))
    return fail(c, SD_CAS_EINVAL, "group: %zu keys exceed the hash grouping's range", n);
  hipStream_t s = pick(c, stream);
  // K4h/K5h: bucket partition + LDS hash min (no full sort); beyond the hash grouping's range:
  // LSD radix sort + run heads (K4 + K5)
  const bool hash = c->use_hash_group(n);
  int rc = ensure(c, c->ws, hash ? hash_group_workspace_bytes(n, c->group_target) : group_workspace_bytes(n));
  if (rc) return rc;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  if (hash)
    HIP_TRY(c, hash_group_min(d_keys, nullptr, n, d_rep, c->d_scalar, c->ws.p, c->gtotals, s,
                              c->group_target));
  else
    HIP_TRY(c, group_keys(d_keys, n, d_rep, c->d_scalar, c->ws.p, s));
  return finish_grouping(c, ws, s, out_objects);
}

int sd_cas_group_min_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint32_t* d_vals, size_t n,
                         uint32_t* d_out, uint64_t* out_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_keys || !d_out)))
    return fail(c, SD_CAS_EINVAL, "group_min: bad arguments");
  if (c->group_method == SD_CAS_GROUP_HASH && !hash_group_supported(n))
    return fail(c, SD_CAS_EINVAL, "group_min: %zu keys exceed the hash grouping's range", n);
  hipStream_t s = pick(c, stream);
  // beyond the hash grouping's range: stable LSD sort of (key, val) + run minima
  const bool hash = c->use_hash_group(n);
  int rc = ensure(c, c->ws, hash ? hash_group_workspace_bytes(n, c->group_target) : group_min_sorted_workspace_bytes(n));
  if (rc) return rc;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  if (hash)
    HIP_TRY(c, hash_group_min(d_keys, d_vals, n, d_out, c->d_scalar, c->ws.p, c->gtotals, s,
                              c->group_target));
  else
    HIP_TRY(c, group_min_by_sort(d_keys, d_vals, n, d_out, c->d_scalar, c->ws.p, s));
  return finish_grouping(c, ws, s, out_objects);
}

int sd_cas_partition_dev(sd_cas_ctx* c, const uint64_t* d_keys, size_t n, uint32_t parts,
                         uint64_t* d_keys_out, uint32_t* d_pos_out, uint64_t* d_counts,
                         void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (parts == 0 || parts > 16384 || n >= (1ull << 32) || !d_counts ||
      (n && (!d_keys || !d_keys_out || !d_pos_out)))
    return fail(c, SD_CAS_EINVAL, "partition: bad arguments");
  hipStream_t s = pick(c, stream);
  int rc = ensure(c, c->ws, partition_workspace_bytes(n, parts));
  if (rc) return rc;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, partition_range(d_keys, n, parts, d_keys_out, d_pos_out, d_counts, c->ws.p, s));
  HIP_TRY(c, ws.release());
  return SD_CAS_OK;
}

int sd_cas_group_sorted_dev(sd_cas_ctx* c, const uint64_t* d_sorted_keys,
                            const uint32_t* d_sorted_vals, size_t n, uint32_t* d_rep,
                            uint64_t* out_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_sorted_keys || !d_sorted_vals || !d_rep)))
    return fail(c, SD_CAS_EINVAL, "group_sorted: bad arguments");
  hipStream_t s = pick(c, stream);
  int rc = ensure(c, c->ws, group_workspace_bytes(n));
  if (rc) return rc;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, group_sorted(d_sorted_keys, d_sorted_vals, n, d_rep, c->d_scalar, c->ws.p, s));
  return finish_grouping(c, ws, s, out_objects);
}

int sd_cas_group_chunked_dev(sd_cas_ctx* c, const uint32_t* d_rep, size_t n, uint32_t chunk,
                             uint32_t* d_rep_chunked, uint64_t* out_created,
                             uint64_t* out_linked, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (chunk == 0 || n >= (1ull << 32) || (n && (!d_rep || !d_rep_chunked)))
    return fail(c, SD_CAS_EINVAL, "group_chunked: bad arguments");
  hipStream_t s = pick(c, stream);
  uint64_t* d_created = c->d_scalar + 1;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, hipMemsetAsync(d_created, 0, 8, s));
  HIP_TRY(c, group_chunked(d_rep, n, chunk, d_rep_chunked, d_created, s));
  HIP_TRY(c, ws.release());
  uint64_t created = 0;
  HIP_TRY(c, hipMemcpyAsync(&created, d_created, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (out_created) *out_created = created;
  if (out_linked) *out_linked = n - created;
  return SD_CAS_OK;
}

// ---- the fused hash + group chain -------------------------------------------------
static bool fused_eligible(const sd_cas_ctx* c, size_t n) {
  return n && n % c->quantum == 0 && region_group_supported(n) &&
         (c->group_method == SD_CAS_GROUP_AUTO || c->group_method == SD_CAS_GROUP_HASH) &&
         c->group_target == 0;
}

static uint32_t* region_cursors(const RegionChain& r, int k) { return r.cursors + REGION_SET_WORDS * k; }
// set k's Object counter (the layout of the batch last hashed into it)
static uint64_t* region_objects(const RegionChain& r, int k) {
  return region_group_layout(r.buf[k].p, r.sets.n[k]).objects;
}

// The region target of one set for K1G / K1V and the bucket tables after them: the set's rows and
// spill list, its cursors, and the caller's rep / overflow (the tables take no overflow).
static RegionOut region_out(const RegionGroupWs& L, uint32_t* cursor, uint64_t cap, uint32_t* d_rep,
                            uint32_t* d_overflow) {
  return RegionOut{L.rkeys, L.rfile, cursor, cap, L.spill_keys, L.spill_file, d_rep, d_overflow,
                   (unsigned long long*)L.objects};
}

// Does this hash_regions call verify duplicates (K1V) or run plain K1G?  Not with the setter off,
// nor during a pause; a new note of an earlier call with too few candidates to pay for the probe
// starts one (DupVerifyState::note).
static bool dup_verify_this_call(DupVerifyState& v) {
  if (!v.on) return false;
  if (v.skip) {
    v.skip--;
    return false;
  }
  const volatile uint32_t* note = v.note;
  const uint32_t seq = note[0], cand = note[1], files = note[2];
  if (seq != v.seen && note[0] == seq) {
    v.seen = seq;
    if ((uint64_t)cand * DUPV_MIN_CANDIDATE_SHARE < files) {
      v.skip = DUPV_SKIP_CALLS - 1;
      return false;
    }
  }
  return true;
}

// K1V's placement for n files: roles taken at run time, or the static tile map
static bool dup_roles_at_run_time(DupPlacement placement, size_t n, uint32_t cus) {
  return placement == DUP_PLACE_CU ||
         (placement == DUP_PLACE_AUTO && dup_roles_pay(dup_role_grid(n), 4 * cus));
}

int sd_cas_hash_regions_sampled_dev(sd_cas_ctx* c, const void* d_content, uint64_t stride,
                                    const uint64_t* d_sizes, size_t n, uint64_t* d_keys,
                                    uint32_t* d_rep, uint32_t* d_overflow, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (!fused_eligible(c, n))
    return fail(c, SD_CAS_EINVAL,
                "hash_regions: %zu files (a multiple of %zu up to 1,441,792, default group method)",
                n, c->quantum);
  if (!d_content || !d_sizes || !d_keys || !d_rep || !d_overflow || stride < SAMPLED_CONTENT_LEN ||
      (stride & 15) || ((uintptr_t)d_content & 15))
    return fail(c, SD_CAS_EINVAL, "hash_regions: bad arguments (stride=%llu)",
                (unsigned long long)stride);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick(c, stream);
  RegionChain& r = c->regions;
  const RegionSets::Refill f = r.sets.next_refill();
  const int k = f.set;
  uint32_t* cur = region_cursors(r, k);
  if (f.wait_done) HIP_TRY(c, hipStreamWaitEvent(s, r.done[k], 0));
  if (f.wait_hashed) {
    HIP_TRY(c, hipStreamWaitEvent(s, r.hashed[k], 0));
    HIP_TRY(c, hipMemsetAsync(cur, 0, REGION_SET_WORDS * 4, s));
  }
  if (f.rescue) {  // kept in d_scalar for sd_cas_copy_objects_dev
    WsLease ws(c, s);  HIP_TRY(c, ws.error());
    HIP_TRY(c, hipMemcpyAsync(c->d_scalar, region_objects(r, k), 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, ws.release());
    r.sets.objects_in_scalar();
  }
  int rc = ensure(c, r.buf[k], region_group_workspace_bytes(n));
  if (rc) return rc;
  const RegionOut ro = region_out(region_group_layout(r.buf[k].p, n), cur, region_capacity(n), d_rep, d_overflow);
  const uint32_t cus = (uint32_t)(c->quantum / 256);
  hipError_t e;
  if (dup_verify_this_call(c->dupv)) {  // K1V: duplicate contents are compared, not hashed
    DupVerifyState& v = c->dupv;
    if ((rc = ensure(c, v.buf, dup_verify_workspace_bytes(n)))) return rc;
    if ((rc = ensure(c, c->ws, hash_group_workspace_bytes(n)))) return rc;
    // the last call's lists, on another stream: after its chain (the other set's event)
    if (v.n && v.stream != s && r.sets.cur >= 0) HIP_TRY(c, hipStreamWaitEvent(s, r.hashed[r.sets.cur], 0));
    const DupVerifyWs D = dup_verify_layout(v.buf.p, n);
    {
      WsLease ws(c, s);  HIP_TRY(c, ws.error());  // the probes' grouping runs in ws / gtotals
      e = dup_candidates((const uint8_t*)d_content, stride, d_sizes, n, D, c->ws.p, c->gtotals, s);
      HIP_TRY(c, ws.release());
    }
    if (e == hipSuccess)
      e = hash_sampled_regions_verify((const uint8_t*)d_content, stride, d_sizes, n, d_keys, ro, D, v.note,
                                      ++v.seq, s, cus, dup_roles_at_run_time(v.placement, n, cus));
    v.n = e == hipSuccess ? n : 0;
    v.stream = s;
  } else {
    e = hash_sampled_regions((const uint8_t*)d_content, stride, d_sizes, n, d_keys, ro, s, cus);
    c->dupv.n = 0;
  }
  if (e != hipSuccess) {
    (void)hipMemsetAsync(cur, 0, REGION_SET_WORDS * 4, s);  // restore the cursors' invariant
    return fail(c, SD_CAS_EHIP, "hash_regions: %s", hipGetErrorString(e));
  }
  HIP_TRY(c, hipEventRecord(r.hashed[k], s));
  r.sets.hashed(k, n, d_keys);
  return SD_CAS_OK;
}

// the counters of the context's last hash_regions call (zeros when it did not verify duplicates)
static int dup_verify_words(sd_cas_ctx* c, uint32_t (&h)[DUP_COUNTERS]) {
  if (c->dupv.n && c->regions.sets.cur >= 0) {  // the last hash_regions call verified duplicates
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->regions.hashed[c->regions.sets.cur], 0));
    HIP_TRY(c, hipMemcpyAsync(h, dup_verify_layout(c->dupv.buf.p, c->dupv.n).counters, sizeof h,
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return SD_CAS_OK;
}

int sd_cas_dup_verify_counters(sd_cas_ctx* c, uint64_t* out_candidates, uint64_t* out_verified,
                               uint64_t* out_rehashed) {
  if (!c || !out_candidates || !out_verified || !out_rehashed) return SD_CAS_EINVAL;
  uint32_t h[DUP_COUNTERS] = {0};
  const int rc = dup_verify_words(c, h);
  if (rc) return rc;
  *out_candidates = h[DUP_N_CAND];
  *out_verified = h[DUP_VERIFIED];
  *out_rehashed = h[DUP_REHASHED];
  return SD_CAS_OK;
}

int sd_cas_dup_verify_rows(sd_cas_ctx* c, uint64_t* out_groups, uint64_t* out_tasks,
                           uint64_t* out_references) {
  if (!c || !out_groups || !out_tasks || !out_references) return SD_CAS_EINVAL;
  uint32_t h[DUP_COUNTERS] = {0};
  const int rc = dup_verify_words(c, h);
  if (rc) return rc;
  *out_groups = h[DUP_GROUPS];
  *out_tasks = h[DUP_TASKS];
  *out_references = h[DUP_REFS];
  return SD_CAS_OK;
}

int sd_cas_group_regions_dev(sd_cas_ctx* c, size_t n, uint32_t* d_rep, uint64_t* out_objects,
                             void* stream) {
  if (!c) return SD_CAS_EINVAL;
  RegionChain& r = c->regions;
  if (!r.sets.can_group(n) || !d_rep)
    return fail(c, SD_CAS_EINVAL, "group_regions: no ungrouped hash_regions batch of %zu files", n);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick(c, stream);
  const int k = r.sets.cur;
  const RegionGroupWs L = region_group_layout(r.buf[k].p, n);
  uint32_t* cur = region_cursors(r, k);
  HIP_TRY(c, hipStreamWaitEvent(s, r.hashed[k], 0));  // after its K1G, whatever stream
  hipError_t e = region_group_min(L, region_out(L, cur, region_capacity(n), d_rep, nullptr), r.sets.keys[k], n,
                                  c->test_table_fill, s);
  if (e != hipSuccess) {
    (void)hipMemsetAsync(cur, 0, REGION_SET_WORDS * 4, s);
    return fail(c, SD_CAS_EHIP, "group_regions: %s", hipGetErrorString(e));
  }
  HIP_TRY(c, hipEventRecord(r.done[k], s));
  r.sets.tables_enqueued();
  if (out_objects) {
    HIP_TRY(c, hipMemcpyAsync(out_objects, L.objects, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SD_CAS_OK;
}

int sd_cas_hash_group_sampled_dev(sd_cas_ctx* c, const void* d_content, uint64_t stride,
                                  const uint64_t* d_sizes, size_t n, uint64_t* d_keys,
                                  uint32_t* d_rep, uint32_t* d_overflow, uint64_t* out_objects,
                                  void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n && (!d_rep || !d_overflow))
    return fail(c, SD_CAS_EINVAL, "hash_group_sampled: null rep/overflow");
  if (!fused_eligible(c, n)) {  // the two calls in sequence
    int rc = sd_cas_hash_sampled_dev(c, d_content, stride, d_sizes, n, d_keys, stream);
    if (rc) return rc;
    return sd_cas_group_dev(c, d_keys, n, d_rep, out_objects, stream);
  }
  int rc = sd_cas_hash_regions_sampled_dev(c, d_content, stride, d_sizes, n, d_keys, d_rep,
                                           d_overflow, stream);
  if (rc) return rc;
  // (an overflowed region is regrouped by its own table workgroup: exact either way)
  return sd_cas_group_regions_dev(c, n, d_rep, out_objects, stream);
}

// The Object count of the context's last grouping, without a host sync: from the region set that
// holds it (after its tables), or from d_scalar.
int sd_cas_copy_objects_dev(sd_cas_ctx* c, uint64_t* d_dst, void* stream) {
  if (!c || !d_dst) return SD_CAS_EINVAL;
  hipStream_t s = pick(c, stream);
  RegionChain& r = c->regions;
  const int k = r.sets.objects_set;
  if (k >= 0) {
    HIP_TRY(c, hipStreamWaitEvent(s, r.done[k], 0));
    HIP_TRY(c, hipMemcpyAsync(d_dst, region_objects(r, k), 8, hipMemcpyDeviceToDevice, s));
    // the set's next refill (its K1G zeroes this counter) must also wait for this copy
    HIP_TRY(c, hipEventRecord(r.done[k], s));
    return SD_CAS_OK;
  }
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, hipMemcpyAsync(d_dst, c->d_scalar, 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(c, ws.release());
  return SD_CAS_OK;
}

}  // extern "C"
