// ctx_internal.h — the sd_cas_ctx object and the host helpers shared by the C-ABI
// translation units (sd_hip_cas.cpp, group_host.cpp, links_host.cpp, object_index_host.cpp,
// reports_host.cpp, host_paths.cpp, validator_host.cpp, sd_multi.cpp).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <dirent.h>
#include <pthread.h>
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sd_hip_cas.h"
#include "sd_debug.h"
#include "sd_region_sets.h"
#include "sd_ws.h"

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// Persistent host workers for the I/O gather (a 100-file job step cannot afford to spawn
// threads per call).  run(k, fn) executes fn on the caller plus k-1 pool threads and
// returns when all are done; fn pulls work items itself (atomic cursor).
class HostPool {
 public:
  // Round 6: the pool's threads may be confined to a CPU set — the CPUs of the GPU's NUMA
  // node (sd_cas_ctx_create), so the gather's page-cache copies and the pinned staging stay
  // on the socket whose PCIe root the DMA reads from.  Empty = the process's own mask.
  void set_cpus(const cpu_set_t& cpus, int ncpus) {
    std::lock_guard<std::mutex> g(mu_);
    cpus_ = cpus;
    ncpus_ = ncpus;
    for (auto& t : th_) (void)pthread_setaffinity_np(t.native_handle(), sizeof cpus_, &cpus_);
  }
  int bound_cpus() const { return ncpus_; }
  // Round 6: each pool thread may start by unsharing the process's descriptor table
  // (unshare(CLONE_FILES): a private copy of the table as it is then).  The readers open and
  // close a file per item, and with one shared table every open / close takes the same
  // table lock: 16 readers of config 1's mix gathered 575 k files/s shared and 745-775 k
  // private (tools/probe_gather.cpp, profiles/r06/gather/).  The rule this imposes: a pool
  // thread only uses descriptors it opened itself (or that existed when it started: the HIP
  // runtime's) — no task may hand a pool thread a descriptor opened elsewhere.  Set before
  // the first run (threads start lazily); SD_CAS_POOL_PRIVATE_FDS=0 keeps the shared table.
  // The copy would also keep every other descriptor of the process alive in this thread (a
  // pipe's write end: its reader never sees EOF; a socket the application closed: its peer
  // never sees the close; a dmabuf: its memory), so the thread then closes all of its copies
  // except 0-2 and what the HIP runtime holds — /dev/kfd, /dev/dri/renderD*, one eventfd
  // (tools/fd_list.py on the box: nothing else after HIP init, a context and a gather).
  void set_private_fds(bool on) { private_fds_ = on; }
  int private_threads() const { return nprivate_.load(); }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  void run(unsigned k, const std::function<void()>& fn) {
    if (k <= 1) { fn(); return; }
    run2(k - 1, fn, fn);
  }
  // `workers` pool threads run fn while the caller runs caller_fn; returns when all are done
  void run2(unsigned workers, const std::function<void()>& fn, const std::function<void()>& caller_fn) {
    std::unique_lock<std::mutex> lk(mu_);
    while (th_.size() < workers) {
      th_.emplace_back([this] { loop(); });
      if (ncpus_) (void)pthread_setaffinity_np(th_.back().native_handle(), sizeof cpus_, &cpus_);
    }
    fn_ = &fn;
    want_ = workers;
    pending_ = workers;
    ++gen_;
    lk.unlock();
    cv_.notify_all();
    caller_fn();
    lk.lock();
    done_.wait(lk, [this] { return pending_ == 0; });
    fn_ = nullptr;
  }

 private:
  static void keep_only_device_fds() {
    DIR* d = opendir("/proc/thread-self/fd");
    if (!d) return;
    const int self = dirfd(d);
    std::vector<int> drop;
    char path[64], link[256];
    while (dirent* e = readdir(d)) {
      if (e->d_name[0] < '0' || e->d_name[0] > '9') continue;
      const int fd = atoi(e->d_name);
      if (fd == self || fd <= 2) continue;  // stdin/out/err stay (logging from a pool thread)
      snprintf(path, sizeof path, "/proc/thread-self/fd/%d", fd);
      const ssize_t n = readlink(path, link, sizeof link - 1);
      if (n < 0) continue;
      link[n] = 0;
      if (!strcmp(link, "/dev/kfd") || !strncmp(link, "/dev/dri/", 9) || !strcmp(link, "anon_inode:[eventfd]"))
        continue;
      drop.push_back(fd);
    }
    closedir(d);
    for (int fd : drop) close(fd);
  }
  void loop() {
    // private only where the copy can be swept (/proc mounted); closing a copy never releases
    // the application's POSIX locks (their owner is the table they were taken through)
    if (private_fds_ && access("/proc/thread-self/fd", R_OK) == 0 && unshare(CLONE_FILES) == 0) {
      keep_only_device_fds();
      nprivate_.fetch_add(1);
    }
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || (gen_ != seen && want_ > 0); });
      if (stop_) return;
      seen = gen_;
      --want_;
      const std::function<void()>* f = fn_;
      lk.unlock();
      (*f)();
      lk.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> th_;
  const std::function<void()>* fn_ = nullptr;
  unsigned want_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
  cpu_set_t cpus_{};
  int ncpus_ = 0;
  bool private_fds_ = false;
  std::atomic<int> nprivate_{0};
};

constexpr uint32_t DUPV_SKIP_CALLS = 16, DUPV_MIN_CANDIDATE_SHARE = 32;
// SD_CAS_DUP_PLACEMENT: how the workgroups of the verified chain's main kernel get their work
enum DupPlacement { DUP_PLACE_STATIC = 0, DUP_PLACE_CU = 1, DUP_PLACE_AUTO = 2 };

// The fused chain's duplicate verification (K1V, dup_verify.hip) as the context keeps it.
struct DupVerifyState {
  // (sd_cas_set_dup_verify): probes, candidates, lists, flags and counters of the LAST
  // hash_regions call; a call on another stream waits for that call's `hashed` event before
  // it refills them
  DevBuf buf;
  bool on = true;
  // SD_CAS_DUP_PLACEMENT=static|cu|auto, read at creation.  static: the tile map fixed before
  // launch (dup_tile_of); cu: roles taken at run time, at most DUP_CU_LIMIT compare workgroups per
  // CU (sd_dup_runs.h); auto (the default): cu for a grid of at least DUP_ROLES_MIN_ROUNDS times the
  // workgroups the chip holds at once (dup_roles_pay), static below
  DupPlacement placement = DUP_PLACE_AUTO;
  uint64_t n = 0;           // files of the last verified call (0: none, or the setter was off)
  hipStream_t stream = nullptr;
  // Probing a batch costs ~0.3 ms at 1.31 M files whatever it finds, and pays from ~1 candidate
  // in 32 files on.  Each verified call leaves {seq, candidates, files} in pinned host memory
  // (note, written by its mixed kernel); a later call that finds a new note with fewer
  // candidates than that runs plain K1G, and so do the next DUPV_SKIP_CALLS - 1 calls, before
  // one probes again.  Read without a sync: a note not yet written just means "probe".
  uint32_t* note = nullptr;
  uint32_t seq = 0;   // verified calls enqueued so far
  uint32_t seen = 0;  // the last note's seq acted on
  uint32_t skip = 0;  // calls left to run without probing
};

// The fused hash + group chain (sd_cas_hash_regions_sampled_dev / sd_cas_group_regions_dev,
// group_host.cpp): the decisions about its two region sets (sd_region_sets.h) and what performs
// them.  cursors holds both sets' cursors (2 x REGION_SET_WORDS u32), zero between calls (the
// tables re-zero); hashed[k] is recorded after set k's K1G (its tables on any stream and its refill
// wait for it), done[k] after its tables (and after a copy of its Object count).
struct RegionChain {
  sdcas::RegionSets sets;
  uint32_t* cursors = nullptr;
  DevBuf buf[2];
  hipEvent_t done[2] = {nullptr, nullptr}, hashed[2] = {nullptr, nullptr};
};

struct sd_object_index;  // a library-resident Object index (object_index_host.cpp)

struct sd_cas_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // compute
  hipStream_t copy = nullptr;    // H2D side stream
  hipStream_t copy2 = nullptr;   // the streamed gather's early whole-file hash (A/B: pieces alternate)
  hipEvent_t copy2_done = nullptr;
  hipEvent_t h2d_done = nullptr;
  hipEvent_t packed_h2d = nullptr;   // the job step's whole-file pieces have landed (early hash)
  hipEvent_t packed_done = nullptr;  // ... and their hash (on copy2) has run
  DevBuf ws;       // kernel workspace
  DevBuf staging;  // device copy of a host batch
  DevBuf small;    // multi-device exchange buffers (sd_cas_multi_*)
  DevBuf cvbuf;    // file_checksum: one 32-B CV per 64 MiB segment
  DevBuf io;       // device copies of host arrays (sd_cas_identifier_links)
  DevBuf inplace;  // cas_ids from whole contents: classify's lists (ordered across streams like ws)
  // the exact duplicate grouping (sd_cas_group_exact_dev): fast keys, word ids and the mismatch
  // counter, beside ws (which the inner grouping calls use); ordered across streams like ws
  DevBuf exact;
  int exact_method = 0;  // SD_CAS_EXACT_* (sd_cas_set_exact_method)
  uint64_t exact_mismatched = 0, exact_fallbacks = 0;  // of the last group_exact call
  // the whole-content compare (sd_cas_group_exact_contents_dev): entry lists, flags, slots, task
  // tables and the digest finish's compacted rows, beside ws and exact (which its inner groupings,
  // sorts and digest finish use); ordered across streams like ws
  DevBuf contents;
  uint32_t compare_max_rounds = SD_CAS_EXACT_COMPARE_ROUNDS_DEFAULT;  // 0: no cap
  uint64_t compare_rounds = 0, compare_compares = 0, compare_unequal = 0, compare_digest_rows = 0;
  DupVerifyState dupv;  // the fused chain's duplicate verification (K1V)
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  uint64_t* d_scalar = nullptr;  // 8 x u64 scratch for counters
  // the hash grouping's bucket totals: zero between calls (each call's last kernel re-zeroes
  // them), so the chain has no zeroing launch; ordered across streams like ws
  uint32_t* gtotals = nullptr;
  RegionChain regions;  // the fused hash + group chain's two region sets
  // the context's Object indexes by handle (sd_cas_index_create), destroyed with it
  sd_object_index* index[SD_CAS_INDEX_MAX] = {};
  // SD_CAS_INDEX_LOAD_PERCENT=10..90 (measurement knob, read at creation): the indexes' maximum
  // load in place of INDEX_LOAD_PERCENT (sd_object_index_plan.h); 0 = the built-in value
  uint32_t index_load_percent = 0;
  // ws and d_scalar are shared by every device call of the context, whatever stream the
  // caller passes: the last enqueued use is recorded here and a use on another stream
  // waits for it first (WsLease)
  hipEvent_t ws_ev = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_pending = false;
  size_t quantum = 65536;  // files per full wave of the device (CUs x 4 SIMDs x 64 lanes)
  int group_method = 0;       // SD_CAS_GROUP_* (sd_cas_set_group_method)
  uint64_t group_target = 0;  // mean keys per hash-grouping bucket (0 = tuned default)
  bool use_hash_group(uint64_t n) const {
    return group_method == SD_CAS_GROUP_HASH ||
           (group_method == SD_CAS_GROUP_AUTO && n <= SD_CAS_HASH_GROUP_MAX_KEYS);
  }
  // batches below these sizes use the chunk-parallel K1L kernel (sd_cas_set_latency_threshold)
  size_t latency_sampled = 0, latency_packed = 0;
  // K1L batches of at least this many files pack 4 files per wave (16-lane segments),
  // smaller ones take a wave per file (sd_cas_set_chunkpar_split)
  size_t seg16_sampled = 0, seg16_packed = 0;
  int chunkpar_seg(size_t n, bool sampled) const {
    return n >= (sampled ? seg16_sampled : seg16_packed) ? 16 : 64;
  }
  HostPool pool;  // I/O gather workers
  // the path gather's two window-slot events (persistent: creating them per call cost a
  // 100-file job step ~10 us)
  hipEvent_t gather_done[2] = {nullptr, nullptr};
  bool trace = false;  // SD_CAS_TRACE=1: per-phase host timestamps of host-buffer calls on stderr
  int numa_node = -1;  // the GPU's NUMA node (sysfs), -1 unknown; pool bound to it unless SD_CAS_POOL_NUMA=0
  uint32_t test_table_fill = 0;  // SD_CAS_TEST_TABLE_FILL (tests): region tables' overflow bound
  std::string err;
};

// Host phase timestamps of one blocking call (SD_CAS_TRACE=1): mark(name) after each phase,
// one stderr line at the end — "sd_cas_trace <call> n=<files> <phase>=<us> ...".
struct SdTrace {
  bool on;
  const char* call;
  size_t n;
  std::chrono::steady_clock::time_point t0, last;
  std::string line;
  SdTrace(bool on_, const char* call_, size_t n_) : on(on_), call(call_), n(n_) {
    if (on) t0 = last = std::chrono::steady_clock::now();
  }
  void note(const char* name, double v) {
    if (!on) return;
    char buf[64];
    snprintf(buf, sizeof buf, " %s=%.1f", name, v);
    line += buf;
  }
  void mark(const char* name) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    char buf[64];
    snprintf(buf, sizeof buf, " %s=%.1f", name,
             std::chrono::duration<double, std::micro>(t - last).count());
    line += buf;
    last = t;
  }
  ~SdTrace() {
    if (!on) return;
    fprintf(stderr, "sd_cas_trace %s n=%zu%s total=%.1f\n", call, n, line.c_str(),
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
};

// the NUMA node holding the page at p (get_mempolicy MPOL_F_NODE | MPOL_F_ADDR), -1 unknown
// (trace output only)
inline int sd_page_node(const void* p) {
  int node = -1;
  if (!p || syscall(SYS_get_mempolicy, &node, nullptr, 0UL, p, 3UL /* MPOL_F_NODE|MPOL_F_ADDR */) != 0)
    return -1;
  return node;
}

inline int sd_fail(sd_cas_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

#define HIP_TRY(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return sd_fail((ctx), SD_CAS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                    \
  } while (0)

// NULL = the HIP null (default) stream, exactly as in HIP itself: a caller on the
// default stream (torch's default) must be ordered with our kernels.
inline hipStream_t sd_pick(sd_cas_ctx*, void* s) { return (hipStream_t)s; }

// Order a use of the shared workspace (ws, d_scalar, gtotals) on stream s after the previous use
// on any other stream; release records this use.  Calls on one stream need no event wait
// (stream order), so the single-stream pipelines pay one event record per call.  Called by
// WsLease only.
inline hipError_t sd_ws_acquire(sd_cas_ctx* c, hipStream_t s) {
  if (c->ws_pending && c->ws_stream != s) return hipStreamWaitEvent(s, c->ws_ev, 0);
  return hipSuccess;
}
inline hipError_t sd_ws_release(sd_cas_ctx* c, hipStream_t s) {
  c->ws_stream = s;
  c->ws_pending = true;
  return hipEventRecord(c->ws_ev, s);
}
// One use of the shared workspace on a stream, as a scope: constructing it acquires (error()
// says how that went: a lease whose acquire failed holds nothing), release() records the use once
// and reports how, and a lease that goes out of scope unreleased (an early return) records it
// too, so that no path leaves work in ws that the next stream would not wait for.  Leases nest:
// an outer one around inner public calls that take their own.  Movable, so an object whose
// begin() acquires can keep it for its caller to release (validator_host.cpp QueueDev).
class WsLease {
 public:
  WsLease() = default;
  WsLease(sd_cas_ctx* c, hipStream_t s) : s_(s), err_(sd_ws_acquire(c, s)) { c_ = err_ == hipSuccess ? c : nullptr; }
  WsLease(WsLease&& o) noexcept { *this = std::move(o); }
  WsLease& operator=(WsLease&& o) noexcept {
    (void)release();
    c_ = o.c_;  s_ = o.s_;  err_ = o.err_;  o.c_ = nullptr;
    return *this;
  }
  ~WsLease() { (void)release(); }
  hipError_t error() const { return err_; }
  hipError_t release() {
    sd_cas_ctx* c = c_;  c_ = nullptr;
    return c ? sd_ws_release(c, s_) : hipSuccess;
  }

 private:
  sd_cas_ctx* c_ = nullptr;  hipStream_t s_ = nullptr;  hipError_t err_ = hipSuccess;
};
// a 32-byte digest as 64 lower-case hex digits and a NUL
inline void sd_hex32(const uint8_t d[32], char out[65]) {
  static const char* hx = "0123456789abcdef";
  for (int i = 0; i < 32; i++) { out[2 * i] = hx[d[i] >> 4]; out[2 * i + 1] = hx[d[i] & 15]; }
  out[64] = 0;
}

// Device allocations of a context.  The debug library (SD_DBG) ends each one in a
// patterned 4,096-B tail right after the 256-B round-up of the bytes asked for and keeps it in a
// process-wide list (sd_hip_cas.cpp): sd_cas_debug_violations() reads every tail back, and a tail
// is read once more before its buffer is freed, so a kernel that ran past the end of a layout is
// counted even when the buffer is gone by then.  `name` is what such a report calls the buffer.
#if SD_DBG
#define SD_DBG_TAIL_BYTES 4096
hipError_t sd_dbg_tail_malloc(void** p, size_t bytes, const char* name);
hipError_t sd_dbg_tail_free(void* p);  // synchronises the buffer's device, reads its tail, frees
uint64_t sd_dbg_tail_check_all(void);
inline hipError_t sd_dev_malloc(void** p, size_t bytes, const char* name) {
  return sd_dbg_tail_malloc(p, bytes, name);
}
inline hipError_t sd_dev_free(void* p) { return sd_dbg_tail_free(p); }
#else
inline hipError_t sd_dev_malloc(void** p, size_t bytes, const char*) { return hipMalloc(p, bytes); }
inline hipError_t sd_dev_free(void* p) { return hipFree(p); }
#endif
inline const char* sd_buf_name(const sd_cas_ctx* c, const DevBuf& b) {
  return &b == &c->ws ? "ws" : &b == &c->staging ? "staging" : &b == &c->small ? "small"
       : &b == &c->io ? "io" : &b == &c->inplace ? "inplace" : &b == &c->cvbuf ? "cvbuf" : &b == &c->dupv.buf ? "dupv"
       : &b == &c->exact ? "exact"
       : &b == &c->contents ? "contents"
       : &b == &c->regions.buf[0] ? "regions[0]" : &b == &c->regions.buf[1] ? "regions[1]" : "multi";
}

// Grow a device buffer (on the CURRENT device).  Growing synchronises the device: call
// outside hot loops / graph capture.  At least 1 MiB, except in the debug library, where the
// buffer is exactly what the largest layout so far asked for: that layout ends at the tail.
inline int sd_ensure(sd_cas_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.bytes) return SD_CAS_OK;
  if (b.p) {
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, sd_dev_free(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  size_t want = SD_DBG ? bytes : std::max(bytes, (size_t)1 << 20);
  if (sd_dev_malloc(&b.p, want, sd_buf_name(c, b)) != hipSuccess) {
    (void)hipGetLastError();
    return sd_fail(c, SD_CAS_ENOMEM, "hipMalloc(%zu) failed", want);
  }
  b.bytes = want;
  return SD_CAS_OK;
}

// The staging's host mapping.  SD_PINNED_MODE 0 = hipHostMallocDefault (the product), whose
// coherence follows HIP_HOST_COHERENT (unset = 0 = NON-coherent on ROCm); 1 = explicitly
// hipHostMallocNonCoherent; 2 = explicitly hipHostMallocCoherent.  Round 4's "coherent vs
// non-coherent" A/B compared modes 0 and 1 — with HIP_HOST_COHERENT unset both are the same
// non-coherent mapping, so it showed nothing; the three-arm A/B of round 5 with
// an explicit coherent arm is profiles/r05/ab_pinned_mode/ (DESIGN.md §2.2, f1).
#ifndef SD_PINNED_MODE
#define SD_PINNED_MODE 0
#endif
#define SD_PINNED_FLAGS                                                              \
  (SD_PINNED_MODE == 1 ? hipHostMallocNonCoherent                                    \
                       : SD_PINNED_MODE == 2 ? hipHostMallocCoherent : hipHostMallocDefault)

// K1 / K1L / K1+K1L by batch size (sd_hip_cas.cpp), shared with the host entry points
extern "C" hipError_t sd_dispatch_sampled(sd_cas_ctx* c, const uint8_t* content, uint64_t stride,
                                          const uint64_t* sizes, size_t n, uint64_t* keys,
                                          hipStream_t s);
// K2 / K1L by batch size over ragged whole files (sd_hip_cas.cpp); sorts in c->ws, which the
// caller has sized (sd_packed_workspace_bytes) and acquired
extern "C" hipError_t sd_dispatch_packed(sd_cas_ctx* c, const uint8_t* arena, const uint64_t* offs,
                                         const uint32_t* lens, const uint64_t* sizes, size_t n,
                                         uint64_t* keys, hipStream_t s);
extern "C" size_t sd_packed_workspace_bytes(const sd_cas_ctx* c, size_t n);

// Workspace layouts of the C-ABI translation units (host_paths.cpp's StagedLayout: byte offsets)
// (sd_ws.h; a null base measures).  Internal: exported only so tests/native/ws_layout_test.cpp links them.
struct PackedWs { uint64_t *lkeys, *skeys; uint32_t* order; void* sort_ws; size_t bytes; };
struct LinkStagingWs {
  uint32_t* rep; uint64_t* hkeys; uint32_t *hrows, *minrow; uint64_t* orphans;
  uint32_t *starts, *counts, *boff; uint64_t* tiles; uint32_t* filter; uint64_t* counters; size_t bytes;
};
struct LinkIoWs {
  uint64_t* keys; uint8_t* state; uint32_t *step, *object; uint8_t* action;
  uint64_t* seed_keys; uint32_t *seed_objects, *pre; size_t bytes;
};
struct StatsWs { uint64_t *shards, *totals; size_t bytes; };
struct TopWs {
  uint64_t *hist, *sel; uint32_t* scan; uint64_t* ckeys; uint32_t* cvals; uint64_t* skeys;
  uint32_t* svals; void* sort_ws; size_t bytes;
};
struct DupReportWs {
  uint64_t *keys, *sizes; uint32_t *rep, *copies; uint8_t* state; uint64_t* hkeys;
  uint32_t *hrows, *minrow; uint64_t* orphans; uint32_t* top_heads; uint64_t *top_waste, *counters; size_t bytes;
};
struct ExactWs { uint64_t* keys; uint32_t *ids, *counter; size_t bytes; };
struct ExactReportWs {
  uint64_t* ckeys; uint8_t* cdigests; uint32_t *crows, *prior, *crep; uint64_t* sizes; uint8_t* state;
  uint32_t *rep, *copies, *top_heads; uint64_t* top_waste; size_t bytes;
};
struct IndexIoWs { uint64_t* keys; uint32_t* objects; size_t bytes; };
struct StagedLayout { size_t packed, sizes, poffs, plens, keys, h2d_bytes, bytes; };
struct MultiBufs {
  uint64_t* skeys; uint32_t* sidx; uint64_t* gidx; uint64_t* splits; uint64_t* back;
  uint64_t* rkeys; uint64_t* ridx; uint64_t* k2; uint32_t* pos; uint32_t* rep_pos; uint64_t* repg; size_t bytes;
};
MultiBufs sd_multi_bufs_layout(void* base, size_t n, size_t m, int G);
extern "C" {
StagedLayout sd_staged_layout(size_t sampled_bytes, size_t packed_bytes, size_t ns, size_t np, size_t n);
PackedWs sd_packed_layout(void* ws, size_t n);
LinkStagingWs sd_link_staging_layout(void* base, size_t n, size_t n_seed, size_t steps_total, bool pre);
LinkIoWs sd_link_io_layout(void* base, size_t n, size_t n_seed, bool pre);
StatsWs sd_stats_layout(void* ws);
TopWs sd_top_layout(void* ws, uint64_t n, uint64_t m);
DupReportWs sd_dup_report_layout(void* base, size_t n, bool state, size_t k);
ExactWs sd_exact_layout(void* base, size_t n);
ExactReportWs sd_exact_report_layout(void* base, size_t n, size_t m, size_t k);
IndexIoWs sd_index_io_layout(void* base, size_t n);
}

inline int sd_ensure_pinned(sd_cas_ctx* c, size_t bytes) {
  if (bytes <= c->pinned_bytes) return SD_CAS_OK;
  if (c->pinned) {
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipHostFree(c->pinned));
    c->pinned = nullptr;
    c->pinned_bytes = 0;
  }
  size_t want = std::max(bytes, (size_t)1 << 22);
  if (hipHostMalloc(&c->pinned, want, SD_PINNED_FLAGS) != hipSuccess) {
    (void)hipGetLastError();
    return sd_fail(c, SD_CAS_ENOMEM, "hipHostMalloc(%zu) failed", want);
  }
  c->pinned_bytes = want;
  return SD_CAS_OK;
}

// The Object indexes of a context (object_index_host.cpp).  free_all: at context destruction (the
// device is idle).  lookup_min: d_inout[i] = min(d_inout[i], index[d_keys[i]]) on s, ordered with
// the other calls on that index — the link emission's read of it; SD_CAS_EINVAL on a bad handle.
void sd_index_free_all(sd_cas_ctx* c);
int sd_index_lookup_min(sd_cas_ctx* c, uint32_t index, const uint64_t* d_keys, uint64_t n,
                        uint32_t* d_inout, hipStream_t s);
bool sd_index_alive(const sd_cas_ctx* c, uint32_t index);

// short names for the shared helpers, as the C-ABI translation units write them
#define fail sd_fail
#define pick sd_pick
#define ensure sd_ensure
#define ensure_pinned sd_ensure_pinned
