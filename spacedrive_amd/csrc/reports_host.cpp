// reports_host.cpp — what the C ABI (include/sd_hip_cas.h) says about a grouping: the Object
// statistics and top duplicates (object_stats.hip), the two duplicate reports over host arrays, and
// the two exact-duplicate groupings (exact_dups.hip by checksum, content_compare.hip by comparison).
#include "ctx_internal.h"
#include "sd_content_compare.h"
#include "sd_exact_dups.h"
#include "sd_group.h"
#include "sd_links.h"
#include "sd_object_stats.h"

using namespace sdcas;

extern "C" {

// ---- Object statistics -----------------------------------------------------------------
// statistics.rs:42,46 writes total_object_count and total_unique_bytes as 0 (schema.prisma:
// 83,87): object_stats.hip fills them from rep and sizes.

static_assert(SD_CAS_STAT_ROWS == STAT_ROWS && SD_CAS_STAT_OBJECTS == STAT_OBJECTS &&
                  SD_CAS_STAT_TOTAL_BYTES == STAT_TOTAL_BYTES &&
                  SD_CAS_STAT_UNIQUE_BYTES == STAT_UNIQUE_BYTES &&
                  SD_CAS_STAT_DUPLICATE_SETS == STAT_DUPLICATE_SETS &&
                  SD_CAS_STAT_MAX_COPIES == STAT_MAX_COPIES &&
                  SD_CAS_STAT_SIZE_MISMATCH_ROWS == STAT_SIZE_MISMATCH_ROWS &&
                  SD_CAS_STAT_BAD_ROWS == STAT_BAD_ROWS && SD_CAS_STAT_COUNT == STAT_COUNT,
              "stat constants");

// ws: totals shards | the context's totals (d_totals NULL)
StatsWs sd_stats_layout(void* ws) {
  WsCarve w(ws);  StatsWs L;
  L.shards = w.take<uint64_t>(stats_shard_bytes() / 8);  L.totals = w.take<uint64_t>(SD_CAS_STAT_COUNT);
  L.bytes = w.bytes();  return L;
}
// top duplicates' ws: histogram | selection words | tile counts and offsets (small_bytes up to
// here) | m candidates (~waste, head) | sorted candidates | the sort's workspace
TopWs sd_top_layout(void* ws, uint64_t n, uint64_t m) {
  WsCarve w(ws);  TopWs L;
  L.hist = w.take<uint64_t>(TOP_BINS);  L.sel = w.take<uint64_t>(TOP_SEL_WORDS);
  L.scan = w.take<uint32_t>(top_scan_bytes(n) / 4);  L.ckeys = w.take<uint64_t>(m);
  L.cvals = w.take<uint32_t>(m);  L.skeys = w.take<uint64_t>(m);  L.svals = w.take<uint32_t>(m);
  L.sort_ws = w.nest(m ? sort_workspace_bytes(m) : 0);
  L.bytes = w.bytes();  return L;
}
// the duplicate report's device copies (c->io): keys | sizes | rep | copies | [state | hashed
// keys | hashed rows | their minimum rows | orphan list] | top heads | top waste | 2 counters;
// the bracketed section serves row states and is null without them
DupReportWs sd_dup_report_layout(void* base, size_t n, bool state, size_t k) {
  WsCarve w(base);  DupReportWs L;
  L.keys = w.take<uint64_t>(n);  L.sizes = w.take<uint64_t>(n);
  L.rep = w.take<uint32_t>(n);  L.copies = w.take<uint32_t>(n);
  L.state = state ? w.take<uint8_t>(n) : nullptr;  L.hkeys = state ? w.take<uint64_t>(n) : nullptr;
  L.hrows = state ? w.take<uint32_t>(n) : nullptr;  L.minrow = state ? w.take<uint32_t>(n) : nullptr;
  L.orphans = state ? w.take<uint64_t>(n) : nullptr;  L.top_heads = w.take<uint32_t>(k);
  L.top_waste = w.take<uint64_t>(k);  L.counters = w.take<uint64_t>(2);
  L.bytes = w.bytes();  return L;
}

// state: the host form's row states (rows that are not hashed take no part).
static int object_stats_impl(sd_cas_ctx* c, const uint32_t* d_rep, const uint64_t* d_sizes,
                             const uint8_t* d_state, size_t n, uint32_t* d_copies,
                             uint64_t* d_totals, uint64_t* out_totals, hipStream_t s) {
  if (n == 0) {
    if (d_totals) HIP_TRY(c, hipMemsetAsync(d_totals, 0, SD_CAS_STAT_COUNT * 8, s));
    if (out_totals) {
      for (int k = 0; k < SD_CAS_STAT_COUNT; k++) out_totals[k] = 0;
      if (d_totals) HIP_TRY(c, hipStreamSynchronize(s));
    }
    return SD_CAS_OK;
  }
  int rc = ensure(c, c->ws, sd_stats_layout(nullptr).bytes);
  if (rc) return rc;
  const StatsWs L = sd_stats_layout(c->ws.p);
  if (!d_totals) d_totals = L.totals;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, object_stats(d_rep, d_sizes, d_state, n, d_copies, d_totals, L.shards, s));
  if (out_totals)
    HIP_TRY(c, hipMemcpyAsync(out_totals, d_totals, SD_CAS_STAT_COUNT * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, ws.release());
  if (out_totals) {
    HIP_TRY(c, hipStreamSynchronize(s));
    if (out_totals[SD_CAS_STAT_BAD_ROWS])
      return fail(c, SD_CAS_EINVAL,
                  "object_stats: %llu rows whose rep is not a grouping (rep[i] > i or rep[rep[i]] != rep[i])",
                  (unsigned long long)out_totals[SD_CAS_STAT_BAD_ROWS]);
  }
  return SD_CAS_OK;
}

int sd_cas_object_stats_dev(sd_cas_ctx* c, const uint32_t* d_rep, const uint64_t* d_sizes, size_t n,
                            uint32_t* d_copies, uint64_t* d_totals, uint64_t out_totals[8],
                            void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_rep || !d_sizes || !d_copies)))
    return fail(c, SD_CAS_EINVAL, "object_stats: bad arguments");
  return object_stats_impl(c, d_rep, d_sizes, nullptr, n, d_copies, d_totals, out_totals,
                           pick(c, stream));
}

int sd_cas_top_duplicates_dev(sd_cas_ctx* c, const uint32_t* d_rep, const uint64_t* d_sizes,
                              const uint32_t* d_copies, size_t n, size_t k, uint32_t* d_top_heads,
                              uint64_t* d_top_waste, uint64_t* out_found, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (!out_found || n >= (1ull << 32) || (n && (!d_rep || !d_sizes || !d_copies)) ||
      (k && (!d_top_heads || !d_top_waste)))
    return fail(c, SD_CAS_EINVAL, "top_duplicates: bad arguments");
  if (k > SD_CAS_TOP_MAX)
    return fail(c, SD_CAS_EINVAL, "top_duplicates: k = %zu exceeds SD_CAS_TOP_MAX", k);
  *out_found = 0;
  if (k == 0) return SD_CAS_OK;
  hipStream_t s = pick(c, stream);
  if (n == 0) {
    HIP_TRY(c, top_write(nullptr, nullptr, 0, k, d_top_heads, d_top_waste, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return SD_CAS_OK;
  }
  // The candidate count m is known only after the selection, so the layout's first part (m = 0)
  // is sized up front; if the rest does not fit, ws grows (that synchronises and drops its
  // contents) and the selection runs once more — the steady state is one 32-byte read-back,
  // the call's one sync before the final one.
  int rc = ensure(c, c->ws, sd_top_layout(nullptr, n, 0).bytes);
  if (rc) return rc;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  uint64_t sel[TOP_SEL_WORDS] = {0, 0, 0, 0};
  TopWs L = sd_top_layout(c->ws.p, n, 0);
  HIP_TRY(c, top_select(d_rep, d_sizes, d_copies, n, k, L.hist, L.sel, L.scan, s));
  HIP_TRY(c, hipMemcpyAsync(sel, L.sel, sizeof sel, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t m = sel[TOP_SEL_M];
  const int top_bin = (int)sel[TOP_SEL_TOP];
  const size_t need = sd_top_layout(nullptr, n, m).bytes;
  if (need > c->ws.bytes) {
    if ((rc = ensure(c, c->ws, need))) return rc;
    L = sd_top_layout(c->ws.p, n, 0);
    HIP_TRY(c, top_select(d_rep, d_sizes, d_copies, n, k, L.hist, L.sel, L.scan, s));
  }
  L = sd_top_layout(c->ws.p, n, m);
  uint64_t* skeys = L.skeys;  uint32_t* svals = L.svals;
  const uint64_t found = std::min<uint64_t>(k, m);
  if (m) {
    HIP_TRY(c, top_emit(d_rep, d_sizes, d_copies, n, L.sel, L.scan, L.ckeys, L.cvals, s));
    // every candidate's waste is below 2^top_bin, so ~waste differs in bits [0, top_bin) only
    if (m > 1 && top_bin > 0) {
      HIP_TRY(c, radix_sort_pairs(L.ckeys, L.cvals, skeys, svals, m, 0, top_bin, L.sort_ws, s));
    } else {
      skeys = L.ckeys;
      svals = L.cvals;
    }
  }
  HIP_TRY(c, top_write(skeys, svals, found, k, d_top_heads, d_top_waste, s));
  HIP_TRY(c, ws.release());
  HIP_TRY(c, hipStreamSynchronize(s));
  *out_found = found;
  return SD_CAS_OK;
}

// ---- the duplicate reports ---------------------------------------------------------------

// The host outputs both reports give about one grouping (any may be null; the top lists come as
// a pair, with found), and what both do with them: the argument checks (`who` names the entry
// point), the answer for no rows, and the second half over the device rep.
struct ReportOut {
  uint32_t *rep, *copies;
  uint64_t* totals;
  size_t k;
  uint32_t* top_heads;
  uint64_t *top_waste, *found;
  bool want_top() const { return top_heads && top_waste; }
};
static int report_check(sd_cas_ctx* c, const char* who, size_t n, bool inputs, const ReportOut& o) {
  if (n >= (1ull << 32) || (n && !inputs) || (!o.top_heads != !o.top_waste) || (o.want_top() && !o.found))
    return fail(c, SD_CAS_EINVAL, "%s: bad arguments", who);
  if (o.want_top() && o.k > SD_CAS_TOP_MAX)
    return fail(c, SD_CAS_EINVAL, "%s: k = %zu exceeds SD_CAS_TOP_MAX", who, o.k);
  return SD_CAS_OK;
}
// zero totals and found; with no rows also an empty top list, and the report is complete (true)
static bool report_empty(const ReportOut& o, size_t n) {
  if (o.found) *o.found = 0;
  if (o.totals)
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++) o.totals[j] = 0;
  if (n == 0 && o.want_top())
    for (size_t j = 0; j < o.k; j++) { o.top_heads[j] = SD_CAS_NO_OBJECT; o.top_waste[j] = 0; }
  return n == 0;
}
// statistics, the top list (into d_top_heads / d_top_waste) and everything copied back
static int report_finish(sd_cas_ctx* c, const uint32_t* d_rep, const uint64_t* d_sizes, const uint8_t* d_state,
                         size_t n, uint32_t* d_copies, uint32_t* d_top_heads, uint64_t* d_top_waste,
                         const ReportOut& o, hipStream_t s) {
  int rc;
  uint64_t totals[SD_CAS_STAT_COUNT];
  if ((rc = object_stats_impl(c, d_rep, d_sizes, d_state, n, d_copies, nullptr, totals, s))) return rc;
  if (o.totals)
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++) o.totals[j] = totals[j];
  if (o.want_top()) {
    if ((rc = sd_cas_top_duplicates_dev(c, d_rep, d_sizes, d_copies, n, o.k, d_top_heads, d_top_waste, o.found, s)))
      return rc;
    if (o.k) {
      HIP_TRY(c, hipMemcpyAsync(o.top_heads, d_top_heads, o.k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipMemcpyAsync(o.top_waste, d_top_waste, o.k * 8, hipMemcpyDeviceToHost, s));
    }
  }
  if (o.rep) HIP_TRY(c, hipMemcpyAsync(o.rep, d_rep, n * 4, hipMemcpyDeviceToHost, s));
  if (o.copies) HIP_TRY(c, hipMemcpyAsync(o.copies, d_copies, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

int sd_cas_duplicate_report(sd_cas_ctx* c, const uint64_t* h_keys, const uint64_t* h_sizes,
                            const uint8_t* h_state, size_t n, uint32_t* h_rep, uint32_t* h_copies,
                            uint64_t out_totals[8], size_t k, uint32_t* h_top_heads,
                            uint64_t* h_top_waste, uint64_t* out_found) {
  if (!c) return SD_CAS_EINVAL;
  const ReportOut o{h_rep, h_copies, out_totals, k, h_top_heads, h_top_waste, out_found};
  int rc = report_check(c, "duplicate_report", n, h_keys && h_sizes, o);
  if (rc) return rc;
  if (report_empty(o, n)) return SD_CAS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t kk = o.want_top() ? k : 0;
  if ((rc = ensure(c, c->io, sd_dup_report_layout(nullptr, n, h_state != nullptr, kk).bytes))) return rc;
  const DupReportWs L = sd_dup_report_layout(c->io.p, n, h_state != nullptr, kk);
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(L.keys, h_keys, n * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(L.sizes, h_sizes, n * 8, hipMemcpyHostToDevice, s));
  if (h_state) {
    // the hashed rows compacted as (key, row) pairs, grouped by the minimum row per key and
    // scattered back: rep in the CALLER's numbering, SD_CAS_NO_OBJECT on every other row
    uint64_t cnt[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(L.state, h_state, n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(L.counters, 0, 16, s));
    HIP_TRY(c, hipMemsetAsync(L.rep, 0xFF, n * 4, s));
    HIP_TRY(c, links_split(L.keys, L.state, n, L.hkeys, L.hrows, L.counters, L.orphans, L.counters + 1, 0u, s));
    HIP_TRY(c, hipMemcpyAsync(cnt, L.counters, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (cnt[0]) {
      if ((rc = sd_cas_group_min_dev(c, L.hkeys, L.hrows, cnt[0], L.minrow, nullptr, s))) return rc;
      HIP_TRY(c, links_scatter(L.minrow, L.hrows, cnt[0], L.rep, 0u, s));
    }
  } else {
    if ((rc = sd_cas_group_dev(c, L.keys, n, L.rep, nullptr, s))) return rc;
  }
  return report_finish(c, L.rep, L.sizes, L.state, n, L.copies, L.top_heads, L.top_waste, o, s);
}

// ---- exact duplicate sets ----------------------------------------------------------------
// A cas_id samples a file longer than 100 KiB (cas.rs:31-58); the whole-content BLAKE3 of
// validation/hash.rs:11-25 does not.  exact_dups.hip joins the two columns.

// c->exact: the fast (or word / pair) keys | the word ids | the mismatch counter
ExactWs sd_exact_layout(void* base, size_t n) {
  WsCarve w(base);  ExactWs L;
  L.keys = w.take<uint64_t>(n);  L.ids = w.take<uint32_t>(n);  L.counter = w.take<uint32_t>(1);
  L.bytes = w.bytes();  return L;
}
// the exact report's device copies (c->io): the m eligible rows compacted (keys | digests | their
// rows | cas grouping | exact grouping), then per caller row sizes | state | rep | copies, then
// the top list
ExactReportWs sd_exact_report_layout(void* base, size_t n, size_t m, size_t k) {
  WsCarve w(base);  ExactReportWs L;
  L.ckeys = w.take<uint64_t>(m);  L.cdigests = w.take<uint8_t>(32 * (uint64_t)m);
  L.crows = w.take<uint32_t>(m);  L.prior = w.take<uint32_t>(m);  L.crep = w.take<uint32_t>(m);
  L.sizes = w.take<uint64_t>(n);  L.state = w.take<uint8_t>(n);  L.rep = w.take<uint32_t>(n);
  L.copies = w.take<uint32_t>(n);  L.top_heads = w.take<uint32_t>(k);  L.top_waste = w.take<uint64_t>(k);
  L.bytes = w.bytes();  return L;
}

int sd_cas_set_exact_method(sd_cas_ctx* c, int method) {
  if (!c) return SD_CAS_EINVAL;
  if (method != SD_CAS_EXACT_AUTO && method != SD_CAS_EXACT_WORDS)
    return fail(c, SD_CAS_EINVAL, "set_exact_method: method %d", method);
  c->exact_method = method;
  return SD_CAS_OK;
}

int sd_cas_group_exact_counters(sd_cas_ctx* c, uint64_t* out_mismatched_rows, uint64_t* out_fallbacks) {
  if (!c || !out_mismatched_rows || !out_fallbacks) return SD_CAS_EINVAL;
  *out_mismatched_rows = c->exact_mismatched;
  *out_fallbacks = c->exact_fallbacks;
  return SD_CAS_OK;
}

// An exact grouping of no rows: the context's Object count is 0 (a memset, no launch)
static int zero_objects(sd_cas_ctx* c, hipStream_t s, uint64_t* out_objects) {
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, hipMemsetAsync(c->d_scalar, 0, 8, s));
  HIP_TRY(c, ws.release());
  c->regions.sets.objects_in_scalar();
  if (out_objects) *out_objects = 0;
  return SD_CAS_OK;
}

// The word-wise path: class = rep (a constant without one), then for each of the four digest
// words id = group(word) and class = group(class << 32 | id).  By induction the class after word
// w is the first row with the same rep and words 0..w, so the last one is rep_exact; the last
// inner grouping's Object count (d_scalar) is the number of distinct (rep, digest) pairs.
static int group_exact_words(sd_cas_ctx* c, const uint32_t* d_rep, const uint8_t* d_digests, size_t n,
                             uint32_t* d_rep_exact, const ExactWs& L, hipStream_t s) {
  int rc;
  for (uint32_t w = 0; w < 4; w++) {
    HIP_TRY(c, exact_word_keys(d_digests, w, n, L.keys, s));
    if ((rc = sd_cas_group_dev(c, L.keys, n, L.ids, nullptr, s))) return rc;
    HIP_TRY(c, exact_pair_keys(w == 0 ? d_rep : d_rep_exact, L.ids, n, L.keys, s));
    if ((rc = sd_cas_group_dev(c, L.keys, n, d_rep_exact, nullptr, s))) return rc;
  }
  return SD_CAS_OK;
}

int sd_cas_group_exact_dev(sd_cas_ctx* c, const uint32_t* d_rep, const uint8_t* d_digests, size_t n,
                           uint32_t* d_rep_exact, uint64_t* out_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_digests || !d_rep_exact)))
    return fail(c, SD_CAS_EINVAL, "group_exact: bad arguments");
  if ((uintptr_t)d_digests & 15) return fail(c, SD_CAS_EINVAL, "group_exact: digests not 16-B aligned");
  if (n && d_rep && (uintptr_t)d_rep < (uintptr_t)d_rep_exact + 4 * n &&
      (uintptr_t)d_rep_exact < (uintptr_t)d_rep + 4 * n)
    return fail(c, SD_CAS_EINVAL, "group_exact: rep_exact aliases rep");
  if (c->group_method == SD_CAS_GROUP_HASH && !hash_group_supported(n))
    return fail(c, SD_CAS_EINVAL, "group_exact: %zu rows exceed the hash grouping's range", n);
  hipStream_t s = pick(c, stream);
  c->exact_mismatched = c->exact_fallbacks = 0;
  if (n == 0) return zero_objects(c, s, out_objects);
  int rc = ensure(c, c->exact, sd_exact_layout(nullptr, n).bytes);
  if (rc) return rc;
  const ExactWs L = sd_exact_layout(c->exact.p, n);
  // c->exact is ordered with ws: the inner groupings use both
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  uint64_t objects = 0;
  bool words = c->exact_method == SD_CAS_EXACT_WORDS;
  if (!words) {
    uint32_t mismatched = 0;
    HIP_TRY(c, hipMemsetAsync(L.counter, 0, 4, s));
    HIP_TRY(c, exact_keys(d_rep, d_digests, n, L.keys, s));
    if ((rc = sd_cas_group_dev(c, L.keys, n, d_rep_exact, nullptr, s))) return rc;
    HIP_TRY(c, exact_verify(d_rep, d_digests, d_rep_exact, n, L.counter, false, s));
    HIP_TRY(c, hipMemcpyAsync(&mismatched, L.counter, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->exact_mismatched = mismatched;
    words = mismatched != 0;
  }
  if (words) {
    c->exact_fallbacks = 1;
    if ((rc = group_exact_words(c, d_rep, d_digests, n, d_rep_exact, L, s))) return rc;
    HIP_TRY(c, hipMemcpyAsync(&objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
#if SD_DBG
    // (the count lands in L.counter and is not read: a differing row reports itself)
    HIP_TRY(c, hipMemsetAsync(L.counter, 0, 4, s));
    HIP_TRY(c, exact_verify(d_rep, d_digests, d_rep_exact, n, L.counter, true, s));
#endif
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  HIP_TRY(c, ws.release());
  if (out_objects) *out_objects = objects;
  return SD_CAS_OK;
}

// ---- exact duplicate sets by comparison (content_compare.hip) -------------------------------

// c->contents: the class grouping | the two entry lists | flags and slots | the task tables | the
// counters | the digest finish's rows
ContentCompareWs sd_content_compare_layout(void* base, size_t n) {
  WsCarve w(base);  ContentCompareWs L;
  const uint64_t n_win = ct_window_count((uint32_t)n);
  L.keys = w.take<uint64_t>(n);  L.ids = w.take<uint32_t>(n);  L.cls = w.take<uint32_t>(n);
  L.ekey_in = w.take<uint64_t>(n);  L.ekey = w.take<uint64_t>(n);
  L.erow_in = w.take<uint32_t>(n);  L.erow = w.take<uint32_t>(n);
  L.neq = w.take<uint32_t>(n);  L.slot = w.take<uint32_t>(n);
  L.wpieces = w.take<uint32_t>(n_win);  L.wstart = w.take<uint32_t>(n_win);
  L.scan = w.take<uint32_t>(n_win / 4096 + 1);  // exclusive_scan_u32's scratch
  L.tasks = w.take<unsigned long long>(1);  L.counters = w.take<uint32_t>(CT_COUNTERS);
  L.pval = w.take<uint32_t>(n);  L.order = w.take<uint32_t>(n);  L.cpiv = w.take<uint32_t>(n);
  L.crep = w.take<uint32_t>(n);  L.coffs = w.take<uint64_t>(n);  L.clens = w.take<uint64_t>(n);
  L.skeys = w.take<uint64_t>(n);  L.cdig = w.take<uint8_t>(32 * (uint64_t)n);
  L.bytes = w.bytes();  return L;
}

// the task arithmetic's constants, for tests that place their boundaries from them (internal,
// like the layouts above): slice, piece, entries per task, default round cap
void sd_content_tasks_constants(uint64_t out[4]) {
  out[0] = CT_SLICE_BYTES;  out[1] = CT_PIECE_BYTES;  out[2] = CT_RUN_K;
  out[3] = SD_CAS_EXACT_COMPARE_ROUNDS_DEFAULT;
}

int sd_cas_set_exact_compare_rounds(sd_cas_ctx* c, uint32_t max_rounds) {
  if (!c) return SD_CAS_EINVAL;
  c->compare_max_rounds = max_rounds;
  return SD_CAS_OK;
}

int sd_cas_exact_compare_counters(sd_cas_ctx* c, uint64_t* out_rounds, uint64_t* out_compares,
                                  uint64_t* out_unequal, uint64_t* out_digest_rows) {
  if (!c || !out_rounds || !out_compares || !out_unequal || !out_digest_rows) return SD_CAS_EINVAL;
  *out_rounds = c->compare_rounds;
  *out_compares = c->compare_compares;
  *out_unequal = c->compare_unequal;
  *out_digest_rows = c->compare_digest_rows;
  return SD_CAS_OK;
}

// The digest finish: the m live entries of the sorted list and their pivots, compacted in row
// order (a stable one-bit sort of the marks), through the checksum chain and the digest split with
// rep = the current pivot; a pivot row carries itself, so rows equal to it join it and it stays the
// smallest of its set.
static int compare_finish_by_digest(sd_cas_ctx* c, const uint8_t* arena, uint64_t arena_bytes,
                                    const uint64_t* d_offs, const uint64_t* d_lens, size_t n, uint32_t m,
                                    const ContentCompareWs& L, uint32_t* d_rep_exact, hipStream_t s) {
  int rc;
  uint32_t marked = 0;
  HIP_TRY(c, ct_mark(L, m, n, s));
  if ((rc = sd_cas_sort_pairs_dev(c, L.skeys, nullptr, n, L.keys, L.order, 0, 1, s))) return rc;
  HIP_TRY(c, hipMemcpyAsync(&marked, L.counters + CT_MARKED, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, ct_gather(L, d_offs, d_lens, marked, s));
  if ((rc = sd_cas_checksums_dev(c, arena, arena_bytes, L.coffs, L.clens, marked, L.cdig, s))) return rc;
  if ((rc = sd_cas_group_exact_dev(c, L.cpiv, L.cdig, marked, L.crep, nullptr, s))) return rc;
  HIP_TRY(c, exact_scatter(L.crep, L.order, marked, d_rep_exact, s));
  return SD_CAS_OK;
}

int sd_cas_group_exact_contents_dev(sd_cas_ctx* c, const uint32_t* d_rep, const void* d_arena,
                                    uint64_t arena_bytes, const uint64_t* d_offs, const uint64_t* d_lens,
                                    size_t n, uint32_t* d_rep_exact, uint64_t* out_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n > CT_MAX_ROWS || (n && (!d_rep || !d_arena || !d_offs || !d_lens || !d_rep_exact)) ||
      ((uintptr_t)d_arena & 15))
    return fail(c, SD_CAS_EINVAL, "group_exact_contents: bad arguments");
  if (n && (uintptr_t)d_rep < (uintptr_t)d_rep_exact + 4 * n && (uintptr_t)d_rep_exact < (uintptr_t)d_rep + 4 * n)
    return fail(c, SD_CAS_EINVAL, "group_exact_contents: rep_exact aliases rep");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick(c, stream);
  c->compare_rounds = c->compare_compares = c->compare_unequal = c->compare_digest_rows = 0;
  if (n == 0) return zero_objects(c, s, out_objects);
  int rc = ensure(c, c->contents, sd_content_compare_layout(nullptr, n).bytes);
  if (rc) return rc;
  const ContentCompareWs L = sd_content_compare_layout(c->contents.p, n);
  const uint8_t* arena = (const uint8_t*)d_arena;
  // c->contents is ordered with ws: the inner calls use both
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  // the bounds verdict first: a batch that breaks them is not read and writes nothing
  uint32_t bad = 0;
  HIP_TRY(c, ct_check_bounds(arena_bytes, d_offs, d_lens, n, L.counters, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, L.counters + CT_BAD, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad)
    return fail(c, SD_CAS_EINVAL, "group_exact_contents: %s",
                (bad & 1) ? "a content is longer than 64 GiB" : "a content is misaligned or extends past arena_bytes");
  // classes: (rep value, length) -> the first row, by the context's grouping; rows of one rep with
  // different lengths split here, without a byte being read
  uint64_t classes = 0;
  if ((rc = sd_cas_group_dev(c, d_lens, n, L.ids, nullptr, s))) return rc;
  HIP_TRY(c, exact_pair_keys(d_rep, L.ids, n, L.keys, s));
  if ((rc = sd_cas_group_dev(c, L.keys, n, L.cls, &classes, s))) return rc;
  HIP_TRY(c, ct_first_entries(L.cls, n, d_rep_exact, L.ekey_in, L.erow_in, L.neq, s));
  int key_bits = 1;
  while (((uint64_t)1 << key_bits) <= n) ++key_bits;  // keys are pivots < n, or n
  const uint32_t grid = (uint32_t)std::max<size_t>(1, c->quantum / 64);  // four workgroups per CU
  uint32_t listed = (uint32_t)n, live = (uint32_t)(n - classes);
  while (live) {
    // the live entries first, a pivot's rows consecutive
    if ((rc = sd_cas_sort_pairs_dev(c, L.ekey_in, L.erow_in, listed, L.ekey, L.erow, 0, key_bits, s))) return rc;
    if (c->compare_max_rounds && c->compare_rounds >= c->compare_max_rounds) break;
    uint32_t after[3] = {0, 0, 0};  // CT_UNEQUAL (of the call so far), CT_UNRESOLVED, CT_OVERFLOW
    HIP_TRY(c, ct_round(arena, d_offs, d_lens, n, live, L, d_rep_exact, grid, s));
    HIP_TRY(c, hipMemcpyAsync(after, L.counters + CT_UNEQUAL, 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    // 2^32 tasks or more in one round (overlapping contents): nothing ran, the sorted list stands
    // and the digest route takes it
    if (after[2]) break;
    c->compare_rounds++;
    c->compare_compares += live;
    c->compare_unequal = after[0];
    listed = live;
    live = after[1];
  }
  if (live) {
    c->compare_digest_rows = live;
    if ((rc = compare_finish_by_digest(c, arena, arena_bytes, d_offs, d_lens, n, live, L, d_rep_exact, s)))
      return rc;
  }
  uint64_t objects = 0;
  HIP_TRY(c, ct_count_heads(d_rep, d_lens, d_rep_exact, n, c->d_scalar, s));
  HIP_TRY(c, hipMemcpyAsync(&objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, ws.release());
  HIP_TRY(c, hipStreamSynchronize(s));
  c->regions.sets.objects_in_scalar();
  if (out_objects) *out_objects = objects;
  return SD_CAS_OK;
}

int sd_cas_duplicate_report_exact(sd_cas_ctx* c, const uint64_t* h_keys, const uint64_t* h_sizes,
                                  const char* h_hex, const uint8_t* h_state, size_t n, uint32_t* h_rep,
                                  uint32_t* h_rep_exact, uint32_t* h_copies_exact, uint64_t out_totals[8],
                                  uint64_t out_totals_exact[8], uint64_t* out_unconfirmed, size_t k,
                                  uint32_t* h_top_heads, uint64_t* h_top_waste, uint64_t* out_found) {
  if (!c) return SD_CAS_EINVAL;
  const ReportOut o{h_rep_exact, h_copies_exact, out_totals_exact, k, h_top_heads, h_top_waste, out_found};
  int rc = report_check(c, "duplicate_report_exact", n, h_keys && h_sizes && h_hex, o);
  if (rc) return rc;
  // every checksum is parsed before any output is written: the eligible rows (HASHED, with a
  // checksum) compacted in ascending row order, so the smallest compacted index of a set is its
  // smallest row
  std::vector<uint64_t> ckeys;
  std::vector<uint8_t> cdig, state(n, (uint8_t)SD_CAS_ROW_ERROR);
  std::vector<uint32_t> crows;
  uint64_t unconfirmed = 0;
  for (size_t i = 0; i < n; i++) {
    const char* hx = h_hex + 65 * i;
    const bool hashed = !h_state || h_state[i] == SD_CAS_ROW_HASHED;
    if (hx[0] == 0) {
      unconfirmed += hashed ? 1 : 0;
      continue;
    }
    uint8_t d[32];
    if (sd_cas_digest_from_hex(hx, d))
      return fail(c, SD_CAS_EINVAL, "duplicate_report_exact: row %zu: malformed checksum", i);
    if (!hashed) continue;
    state[i] = SD_CAS_ROW_HASHED;
    ckeys.push_back(h_keys[i]);
    crows.push_back((uint32_t)i);
    cdig.insert(cdig.end(), d, d + 32);
  }
  const size_t m = crows.size();
  if (h_rep || out_totals)
    if ((rc = sd_cas_duplicate_report(c, h_keys, h_sizes, h_state, n, h_rep, nullptr, out_totals, 0,
                                      nullptr, nullptr, nullptr)))
      return rc;
  if (out_unconfirmed) *out_unconfirmed = unconfirmed;
  if (report_empty(o, n)) return SD_CAS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t kk = o.want_top() ? k : 0;
  if ((rc = ensure(c, c->io, sd_exact_report_layout(nullptr, n, m, kk).bytes))) return rc;
  const ExactReportWs L = sd_exact_report_layout(c->io.p, n, m, kk);
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(L.sizes, h_sizes, n * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(L.state, state.data(), n, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(L.rep, 0xFF, n * 4, s));
  if (m) {
    HIP_TRY(c, hipMemcpyAsync(L.ckeys, ckeys.data(), m * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(L.cdigests, cdig.data(), m * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(L.crows, crows.data(), m * 4, hipMemcpyHostToDevice, s));
    if ((rc = sd_cas_group_dev(c, L.ckeys, m, L.prior, nullptr, s))) return rc;
    if ((rc = sd_cas_group_exact_dev(c, L.prior, L.cdigests, m, L.crep, nullptr, s))) return rc;
    HIP_TRY(c, exact_scatter(L.crep, L.crows, m, L.rep, s));
  }
  return report_finish(c, L.rep, L.sizes, L.state, n, L.copies, L.top_heads, L.top_waste, o, s);
}

}  // extern "C"
