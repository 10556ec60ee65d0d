// object_index_host.cpp — the library-resident Object index of the C ABI (include/sd_hip_cas.h)
// over object_index.hip: handles, the table's size decisions (sd_object_index_plan.h), the order
// of the calls on one index across streams, and the host-array forms.
#include "ctx_internal.h"
#include "sd_links.h"
#include "sd_object_index.h"
#include "sd_object_index_plan.h"

using namespace sdcas;

static_assert(SD_CAS_NO_OBJECT == INDEX_NO_ID, "index constants");

// An index of a context.  The table and the counter block are its own allocations (they outlive
// every call); used_bound is the host's upper bound of the used slots (sd_object_index_plan.h).
// Calls on one index are ordered like the uses of the shared workspace: the last enqueued use is
// recorded in ev, and a use on another stream waits for it first (IndexLease).
struct sd_object_index {
  IndexSlot* slots = nullptr;
  uint64_t nslots = 0;
  uint64_t* ctr = nullptr;
  uint64_t used_bound = 0, rehashes = 0;
  uint32_t op = 0;          // insert / lookup / erase calls that launched, numbered from 1 (next_op)
  bool last_probed = false;  // the last of them is the last such call (else it had n == 0)
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
  bool pending = false;
  IndexTable table() const { return IndexTable{slots, ctr, index_log2(nslots)}; }
};

namespace {

// the maximum load in percent: the built-in value, or what the context read from
// SD_CAS_INDEX_LOAD_PERCENT when it was created (the sweep of tools/bench_object_index.py)
uint32_t load_percent(const sd_cas_ctx* c) {
  return c->index_load_percent ? c->index_load_percent : INDEX_LOAD_PERCENT;
}

// One use of an index on a stream, as a scope (compare WsLease): acquired at construction,
// recorded when it goes out of scope, on every path.
class IndexLease {
 public:
  IndexLease(sd_object_index* ix, hipStream_t s) : ix_(ix), s_(s) {
    err_ = ix->pending && ix->last != s ? hipStreamWaitEvent(s, ix->ev, 0) : hipSuccess;
  }
  ~IndexLease() {
    ix_->last = s_;
    ix_->pending = true;
    (void)hipEventRecord(ix_->ev, s_);
  }
  hipError_t error() const { return err_; }

 private:
  sd_object_index* ix_;
  hipStream_t s_;
  hipError_t err_;
};

sd_object_index* get(sd_cas_ctx* c, uint32_t index, const char* what) {
  if (index < SD_CAS_INDEX_MAX && c->index[index]) return c->index[index];
  (void)fail(c, SD_CAS_EINVAL, "%s: no index %u", what, index);
  return nullptr;
}

hipError_t clear_table(IndexSlot* slots, uint64_t nslots, hipStream_t s) {
  return hipMemsetAsync(slots, 0xFF, nslots * sizeof(IndexSlot), s);
}
hipError_t clear_counters(uint64_t* ctr, hipStream_t s) {
  hipError_t e = hipMemsetAsync(ctr, 0, INDEX_CTR_SIDE * 8, s);
  return e != hipSuccess ? e : hipMemsetAsync(ctr + INDEX_CTR_SIDE, 0xFF, 8, s);
}

void free_index(sd_object_index* ix) {
  if (ix->pending) (void)hipEventSynchronize(ix->ev);
  if (ix->slots) (void)sd_dev_free(ix->slots);
  if (ix->ctr) (void)sd_dev_free(ix->ctr);
  if (ix->ev) (void)hipEventDestroy(ix->ev);
  delete ix;
}

// the counter block as it is once everything enqueued on s has run (blocks)
int read_counters(sd_cas_ctx* c, sd_object_index* ix, uint64_t out[INDEX_CTR_WORDS], hipStream_t s) {
  HIP_TRY(c, hipMemcpyAsync(out, ix->ctr, INDEX_CTR_WORDS * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (out[INDEX_CTR_FULL])
    return fail(c, SD_CAS_EHIP, "object index: a probe found no empty slot in %llu slots",
                (unsigned long long)ix->nslots);
  return SD_CAS_OK;
}

// The bound tripped: read the exact counts and, where they say so, move the live slots into a
// fresh table (blocks; the old table is freed once the move has run).
int make_room(sd_cas_ctx* c, sd_object_index* ix, uint64_t n, hipStream_t s) {
  uint64_t ctr[INDEX_CTR_WORDS];
  int rc = read_counters(c, ix, ctr, s);
  if (rc) return rc;
  const uint64_t live = ctr[INDEX_CTR_ENTRIES], tombs = ctr[INDEX_CTR_TOMBS];
  const uint64_t target = index_rehash_slots(ix->nslots, live, tombs, n, load_percent(c));
  if (target == 0) {
    ix->used_bound = live + tombs;
    return SD_CAS_OK;
  }
  IndexSlot* fresh = nullptr;
  if (target == ~0ull || sd_dev_malloc((void**)&fresh, target * sizeof(IndexSlot), "object index") != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SD_CAS_ENOMEM, "object index: no table for %llu + %llu keys",
                (unsigned long long)live, (unsigned long long)n);
  }
  const IndexTable from = ix->table();
  const IndexTable to{fresh, ix->ctr, index_log2(target)};
  hipError_t e = clear_table(fresh, target, s);
  if (e == hipSuccess) e = index_rehash(from, to, s);
  if (e == hipSuccess) e = hipMemsetAsync(ix->ctr + INDEX_CTR_TOMBS, 0, 8, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)sd_dev_free(fresh);
    return fail(c, SD_CAS_EHIP, "object index: rehash failed: %s", hipGetErrorString(e));
  }
  HIP_TRY(c, sd_dev_free(ix->slots));
  ix->slots = fresh;
  ix->nslots = target;
  ix->used_bound = live;
  ix->rehashes += 1;
  return SD_CAS_OK;
}

// The number of a call that launches on s, from 1.  The device's longest-probe word is op << 32 |
// probe and only grows (atomicMax), so once the 32-bit numbers are used up the word is zeroed on
// s, inside the call's lease and so after every earlier call, and the numbering starts again: a
// long-lived index keeps reporting its last call's probe.
hipError_t next_op(sd_object_index* ix, hipStream_t s, uint32_t* op) {
  if (ix->op == UINT32_MAX) {
    const hipError_t e = hipMemsetAsync(ix->ctr + INDEX_CTR_PROBE, 0, 8, s);
    if (e != hipSuccess) return e;
    ix->op = 0;
  }
  ix->last_probed = true;
  *op = ++ix->op;
  return hipSuccess;
}
// a call with n == 0 launches nothing and is the last call all the same: LAST_MAX_PROBE is 0
void no_op(sd_object_index* ix) { ix->last_probed = false; }

}  // namespace

void sd_index_free_all(sd_cas_ctx* c) {
  for (sd_object_index*& ix : c->index) {
    if (ix) free_index(ix);
    ix = nullptr;
  }
}

bool sd_index_alive(const sd_cas_ctx* c, uint32_t index) {
  return index < SD_CAS_INDEX_MAX && c->index[index];
}

int sd_index_lookup_min(sd_cas_ctx* c, uint32_t index, const uint64_t* d_keys, uint64_t n,
                        uint32_t* d_inout, hipStream_t s) {
  sd_object_index* ix = get(c, index, "identifier_links");
  if (!ix) return SD_CAS_EINVAL;
  if (n == 0) { no_op(ix);  return SD_CAS_OK; }
  IndexLease lease(ix, s);
  HIP_TRY(c, lease.error());
  uint32_t op = 0;
  HIP_TRY(c, next_op(ix, s, &op));
  HIP_TRY(c, index_lookup(ix->table(), d_keys, n, d_inout, true, op, s));
  return SD_CAS_OK;
}

extern "C" {

// the host forms' device copies of their arrays (c->io)
IndexIoWs sd_index_io_layout(void* base, size_t n) {
  WsCarve w(base);  IndexIoWs L;
  L.keys = w.take<uint64_t>(n);  L.objects = w.take<uint32_t>(n);
  L.bytes = w.bytes();  return L;
}

int sd_cas_index_create(sd_cas_ctx* c, uint64_t expected_entries, uint32_t* out_index) {
  if (!c) return SD_CAS_EINVAL;
  if (!out_index) return fail(c, SD_CAS_EINVAL, "index_create: bad arguments");
  uint32_t h = 0;
  while (h < SD_CAS_INDEX_MAX && c->index[h]) ++h;
  if (h == SD_CAS_INDEX_MAX)
    return fail(c, SD_CAS_EINVAL, "index_create: %d indexes are alive on this context", SD_CAS_INDEX_MAX);
  const uint64_t nslots = index_slots_for(expected_entries, load_percent(c));
  if (!nslots)
    return fail(c, SD_CAS_EINVAL, "index_create: %llu expected entries", (unsigned long long)expected_entries);
  HIP_TRY(c, hipSetDevice(c->device));
  sd_object_index* ix = new sd_object_index();
  ix->nslots = nslots;
  if (sd_dev_malloc((void**)&ix->slots, nslots * sizeof(IndexSlot), "object index") != hipSuccess ||
      sd_dev_malloc((void**)&ix->ctr, INDEX_CTR_WORDS * 8, "object index counters") != hipSuccess) {
    (void)hipGetLastError();
    free_index(ix);
    return fail(c, SD_CAS_ENOMEM, "index_create: no memory for %llu slots", (unsigned long long)nslots);
  }
  if (hipEventCreateWithFlags(&ix->ev, hipEventDisableTiming) != hipSuccess ||
      clear_table(ix->slots, nslots, c->stream) != hipSuccess || clear_counters(ix->ctr, c->stream) != hipSuccess ||
      hipEventRecord(ix->ev, c->stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
    free_index(ix);
    return fail(c, SD_CAS_EHIP, "index_create: clearing %llu slots failed", (unsigned long long)nslots);
  }
  ix->last = c->stream;
  ix->pending = true;
  c->index[h] = ix;
  *out_index = h;
  return SD_CAS_OK;
}

int sd_cas_index_destroy(sd_cas_ctx* c, uint32_t index) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_destroy");
  if (!ix) return SD_CAS_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  free_index(ix);
  c->index[index] = nullptr;
  return SD_CAS_OK;
}

int sd_cas_index_clear(sd_cas_ctx* c, uint32_t index, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_clear");
  if (!ix) return SD_CAS_EINVAL;
  hipStream_t s = pick(c, stream);
  IndexLease lease(ix, s);
  HIP_TRY(c, lease.error());
  HIP_TRY(c, clear_table(ix->slots, ix->nslots, s));
  HIP_TRY(c, clear_counters(ix->ctr, s));
  ix->used_bound = 0;
  ix->rehashes = 0;
  ix->last_probed = false;
  return SD_CAS_OK;
}

int sd_cas_index_insert_dev(sd_cas_ctx* c, uint32_t index, const uint64_t* d_keys,
                            const uint32_t* d_objects, size_t n, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_insert");
  if (!ix) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_keys || !d_objects)))
    return fail(c, SD_CAS_EINVAL, "index_insert: bad arguments");
  if (n == 0) { no_op(ix);  return SD_CAS_OK; }
  hipStream_t s = pick(c, stream);
  IndexLease lease(ix, s);
  HIP_TRY(c, lease.error());
  // the verdict on the ids, before anything is inserted
  uint64_t bad = 0;
  HIP_TRY(c, hipMemsetAsync(ix->ctr + INDEX_CTR_BAD, 0, 8, s));
  HIP_TRY(c, links_check_ids(d_objects, n, false, ix->ctr + INDEX_CTR_BAD, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, ix->ctr + INDEX_CTR_BAD, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad) return fail(c, SD_CAS_EINVAL, "index_insert: an Object id is >= 2^31");
  if (index_bound_trips(ix->nslots, ix->used_bound, n, load_percent(c))) {
    const int rc = make_room(c, ix, n, s);
    if (rc) return rc;
  }
  ix->used_bound += n;
  uint32_t op = 0;
  HIP_TRY(c, next_op(ix, s, &op));
  HIP_TRY(c, index_insert(ix->table(), d_keys, d_objects, n, op, s));
  return SD_CAS_OK;
}

int sd_cas_index_lookup_dev(sd_cas_ctx* c, uint32_t index, const uint64_t* d_keys, size_t n,
                            uint32_t* d_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_lookup");
  if (!ix) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_keys || !d_objects)))
    return fail(c, SD_CAS_EINVAL, "index_lookup: bad arguments");
  if (n == 0) { no_op(ix);  return SD_CAS_OK; }
  hipStream_t s = pick(c, stream);
  IndexLease lease(ix, s);
  HIP_TRY(c, lease.error());
  uint32_t op = 0;
  HIP_TRY(c, next_op(ix, s, &op));
  HIP_TRY(c, index_lookup(ix->table(), d_keys, n, d_objects, false, op, s));
  return SD_CAS_OK;
}

int sd_cas_index_erase_dev(sd_cas_ctx* c, uint32_t index, const uint64_t* d_keys, size_t n, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_erase");
  if (!ix) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && !d_keys)) return fail(c, SD_CAS_EINVAL, "index_erase: bad arguments");
  if (n == 0) { no_op(ix);  return SD_CAS_OK; }
  hipStream_t s = pick(c, stream);
  IndexLease lease(ix, s);
  HIP_TRY(c, lease.error());
  uint32_t op = 0;
  HIP_TRY(c, next_op(ix, s, &op));
  HIP_TRY(c, index_erase(ix->table(), d_keys, n, op, s));
  return SD_CAS_OK;
}

int sd_cas_index_export_dev(sd_cas_ctx* c, uint32_t index, uint64_t* d_keys, uint32_t* d_objects,
                            size_t cap, uint64_t* out_n, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_export");
  if (!ix) return SD_CAS_EINVAL;
  if (!out_n || (cap && (!d_keys || !d_objects))) return fail(c, SD_CAS_EINVAL, "index_export: bad arguments");
  hipStream_t s = pick(c, stream);
  IndexLease lease(ix, s);
  HIP_TRY(c, lease.error());
  uint64_t ctr[INDEX_CTR_WORDS];
  const int rc = read_counters(c, ix, ctr, s);
  if (rc) return rc;
  *out_n = ctr[INDEX_CTR_ENTRIES];
  if (*out_n > cap)
    return fail(c, SD_CAS_EINVAL, "index_export: %llu pairs, room for %zu", (unsigned long long)*out_n, cap);
  if (*out_n == 0) return SD_CAS_OK;
  HIP_TRY(c, hipMemsetAsync(ix->ctr + INDEX_CTR_EXPORT, 0, 8, s));
  HIP_TRY(c, index_export(ix->table(), d_keys, d_objects, cap, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

int sd_cas_index_stats(sd_cas_ctx* c, uint32_t index, uint64_t out[8]) {
  if (!c) return SD_CAS_EINVAL;
  sd_object_index* ix = get(c, index, "index_stats");
  if (!ix) return SD_CAS_EINVAL;
  if (!out) return fail(c, SD_CAS_EINVAL, "index_stats: bad arguments");
  IndexLease lease(ix, c->stream);
  HIP_TRY(c, lease.error());
  uint64_t ctr[INDEX_CTR_WORDS];
  const int rc = read_counters(c, ix, ctr, c->stream);
  if (rc) return rc;
  for (int k = 0; k < 8; k++) out[k] = 0;
  out[SD_CAS_INDEX_STAT_ENTRIES] = ctr[INDEX_CTR_ENTRIES];
  out[SD_CAS_INDEX_STAT_SLOTS] = ix->nslots;
  out[SD_CAS_INDEX_STAT_TOMBSTONES] = ctr[INDEX_CTR_TOMBS];
  out[SD_CAS_INDEX_STAT_REHASHES] = ix->rehashes;
  if (ix->last_probed && (uint32_t)(ctr[INDEX_CTR_PROBE] >> 32) == ix->op)
    out[SD_CAS_INDEX_STAT_LAST_MAX_PROBE] = (uint32_t)ctr[INDEX_CTR_PROBE];
  return SD_CAS_OK;
}

// ---- host arrays: staged in c->io, on the context's stream, blocking ---------------------------

static int stage_keys(sd_cas_ctx* c, const uint64_t* h_keys, const uint32_t* h_objects, size_t n, IndexIoWs* L) {
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = ensure(c, c->io, sd_index_io_layout(nullptr, n).bytes);
  if (rc) return rc;
  *L = sd_index_io_layout(c->io.p, n);
  HIP_TRY(c, hipMemcpyAsync(L->keys, h_keys, n * 8, hipMemcpyHostToDevice, c->stream));
  if (h_objects) HIP_TRY(c, hipMemcpyAsync(L->objects, h_objects, n * 4, hipMemcpyHostToDevice, c->stream));
  return SD_CAS_OK;
}

int sd_cas_index_insert(sd_cas_ctx* c, uint32_t index, const uint64_t* h_keys, const uint32_t* h_objects,
                        size_t n) {
  if (!c) return SD_CAS_EINVAL;
  if (!get(c, index, "index_insert")) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!h_keys || !h_objects)))
    return fail(c, SD_CAS_EINVAL, "index_insert: bad arguments");
  if (n == 0) return sd_cas_index_insert_dev(c, index, nullptr, nullptr, 0, c->stream);
  IndexIoWs L;
  int rc = stage_keys(c, h_keys, h_objects, n, &L);
  if (rc) return rc;
  if ((rc = sd_cas_index_insert_dev(c, index, L.keys, L.objects, n, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SD_CAS_OK;
}

int sd_cas_index_lookup(sd_cas_ctx* c, uint32_t index, const uint64_t* h_keys, size_t n, uint32_t* h_objects) {
  if (!c) return SD_CAS_EINVAL;
  if (!get(c, index, "index_lookup")) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!h_keys || !h_objects)))
    return fail(c, SD_CAS_EINVAL, "index_lookup: bad arguments");
  if (n == 0) return sd_cas_index_lookup_dev(c, index, nullptr, 0, nullptr, c->stream);
  IndexIoWs L;
  int rc = stage_keys(c, h_keys, nullptr, n, &L);
  if (rc) return rc;
  if ((rc = sd_cas_index_lookup_dev(c, index, L.keys, n, L.objects, c->stream))) return rc;
  HIP_TRY(c, hipMemcpyAsync(h_objects, L.objects, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SD_CAS_OK;
}

int sd_cas_index_erase(sd_cas_ctx* c, uint32_t index, const uint64_t* h_keys, size_t n) {
  if (!c) return SD_CAS_EINVAL;
  if (!get(c, index, "index_erase")) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && !h_keys)) return fail(c, SD_CAS_EINVAL, "index_erase: bad arguments");
  if (n == 0) return sd_cas_index_erase_dev(c, index, nullptr, 0, c->stream);
  IndexIoWs L;
  int rc = stage_keys(c, h_keys, nullptr, n, &L);
  if (rc) return rc;
  if ((rc = sd_cas_index_erase_dev(c, index, L.keys, n, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SD_CAS_OK;
}

}  // extern "C"
