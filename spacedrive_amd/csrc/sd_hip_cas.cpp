// sd_hip_cas.cpp — the core of the C ABI (include/sd_hip_cas.h) over the gfx950 kernels: the
// debug library's allocation tails, contexts and their setters, the hex helpers, the device-resident
// cas dispatch (K1 / K1L / K2 by batch size) and the synthetic inputs.  The other entry points:
// grouping and the fused chain in group_host.cpp, link emission in links_host.cpp, the Object index
// in object_index_host.cpp, statistics, reports and exact duplicates in reports_host.cpp, host
// buffers and paths in host_paths.cpp, the validator in validator_host.cpp, several devices in
// sd_multi.cpp.
//
// Host runtime for the batched drop-in of generate_cas_id (core/src/object/cas.rs:23-62),
// its batch caller identifier_job_step (core/src/object/file_identifier/mod.rs:98-350)
// and file_checksum (core/src/object/validation/hash.rs:11-25):
//   - a context per (thread, device): compute stream + copy (side) stream, a growable
//     device workspace and pinned staging, last-error string;
//   - host batches are gathered into pinned staging (pread at the cas.rs:27-58 offsets
//     for the path variant), copied with hipMemcpyAsync on the side stream, and hashed
//     on the compute stream after an event hand-off;
//   - no CPU hashing anywhere: every digest comes from the HIP kernels.
#include <ctype.h>

#include "ctx_internal.h"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_mix.h"
#include "sd_synth.h"

using namespace sdcas;

#if SD_DBG
namespace sdcas {
uint32_t sd_dbg_violations_group_hash();
uint32_t sd_dbg_violations_cas_hash();
uint32_t sd_dbg_violations_dup_verify();
uint32_t sd_dbg_violations_group();
uint32_t sd_dbg_violations_checksum();
uint32_t sd_dbg_violations_links();
uint32_t sd_dbg_violations_inplace();
uint32_t sd_dbg_violations_object_stats();
uint32_t sd_dbg_violations_exact_dups();
uint32_t sd_dbg_violations_content_compare();
uint32_t sd_dbg_violations_object_index();
}  // namespace sdcas
// debug library only (libsd_hip_cas_debug.so, not in the ABI header): invariant violations
// counted by the device checks of sd_debug.h since the library was loaded
// ... plus the allocation tails found changed (below)
extern "C" uint64_t sd_cas_debug_violations(void) {
  return (uint64_t)sd_dbg_violations_group_hash() + sd_dbg_violations_cas_hash() +
         sd_dbg_violations_dup_verify() + sd_dbg_violations_group() +
         sd_dbg_violations_checksum() + sd_dbg_violations_links() + sd_dbg_violations_inplace() +
         sd_dbg_violations_object_stats() + sd_dbg_violations_exact_dups() +
         sd_dbg_violations_content_compare() + sd_dbg_violations_object_index() + sd_dbg_tail_check_all();
}

// The allocation tails of ctx_internal.h: every device buffer of a context is followed by
// SD_DBG_TAIL_BYTES of a position-dependent pattern (no constant store reproduces it).  A tail
// found changed counts once, is reported with the buffer's name, the bytes that were asked for
// and the first changed offset, and is armed again.
namespace {
struct DbgTail { void* p; size_t bytes; std::string name; int device; };
std::mutex g_tail_mu;
std::vector<DbgTail> g_tails;
uint64_t g_tail_violations = 0;

inline uint8_t tail_byte(size_t i) { return (uint8_t)((i * 167u + 13u) ^ (i >> 8) ^ 0xA5u); }
const uint8_t* tail_pattern() {
  static uint8_t pat[SD_DBG_TAIL_BYTES];
  static bool made = false;
  if (!made) {
    for (size_t i = 0; i < sizeof pat; i++) pat[i] = tail_byte(i);
    made = true;
  }
  return pat;
}
// g_tail_mu held, t.device current and idle
void tail_check_one(const DbgTail& t, const char* when) {
  uint8_t got[SD_DBG_TAIL_BYTES];
  uint8_t* tail = (uint8_t*)t.p + up256(t.bytes);
  if (hipMemcpy(got, tail, sizeof got, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    ++g_tail_violations;
    printf("SD_CAS tail of %s (%zu bytes) could not be read (%s)\n", t.name.c_str(), t.bytes, when);
    fflush(stdout);
    return;
  }
  const uint8_t* pat = tail_pattern();
  if (memcmp(got, pat, sizeof got) == 0) return;
  size_t first = 0, changed = 0;
  for (size_t i = sizeof got; i-- > 0;)
    if (got[i] != pat[i]) { first = i; ++changed; }
  ++g_tail_violations;
  printf("SD_CAS workspace overrun (%s): buffer %s of %zu bytes, %zu tail bytes changed, the first "
         "at offset %zu past its 256-B round-up\n", when, t.name.c_str(), t.bytes, changed, first);
  fflush(stdout);
  (void)hipMemcpy(tail, pat, sizeof got, hipMemcpyHostToDevice);
}
}  // namespace

hipError_t sd_dbg_tail_malloc(void** p, size_t bytes, const char* name) {
  hipError_t e = hipMalloc(p, up256(bytes) + SD_DBG_TAIL_BYTES);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> g(g_tail_mu);
  e = hipMemcpy((uint8_t*)*p + up256(bytes), tail_pattern(), SD_DBG_TAIL_BYTES, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(*p);
    *p = nullptr;
    return e;
  }
  int dev = 0;
  (void)hipGetDevice(&dev);
  g_tails.push_back({*p, bytes, name, dev});
  return hipSuccess;
}

hipError_t sd_dbg_tail_free(void* p) {
  {
    std::lock_guard<std::mutex> g(g_tail_mu);
    for (size_t i = 0; i < g_tails.size(); i++) {
      if (g_tails[i].p != p) continue;
      int cur = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(g_tails[i].device);
      (void)hipDeviceSynchronize();
      tail_check_one(g_tails[i], "at free");
      (void)hipSetDevice(cur);
      g_tails.erase(g_tails.begin() + i);
      break;
    }
  }
  return hipFree(p);
}

uint64_t sd_dbg_tail_check_all(void) {
  std::lock_guard<std::mutex> g(g_tail_mu);
  int cur = 0;
  (void)hipGetDevice(&cur);
  int synced = -1;  // the list is in allocation order: mostly one device
  for (const DbgTail& t : g_tails) {
    if (t.device != synced) {
      (void)hipSetDevice(t.device);
      (void)hipDeviceSynchronize();
      synced = t.device;
    }
    tail_check_one(t, "at check");
  }
  (void)hipSetDevice(cur);
  return g_tail_violations;
}
#endif

extern "C" {

int sd_cas_abi_version(void) { return SD_CAS_ABI_VERSION; }

// why the calling thread's last sd_cas_ctx_create failed: sd_cas_last_error(NULL)
static thread_local std::string g_ctx_create_err;

// The gather pool's CPUs: the GPU's NUMA node (its PCI device's sysfs numa_node and the node's
// cpulist), intersected with the CPUs this process may use.  On a two-socket host a reader on
// the far socket copies page-cache bytes across the socket link into staging that the DMA then
// reads back across it again; round 6 measured the file path bimodal between processes (~52 vs
// ~40 GB/s, profiles/r06/validator/) before binding.  SD_CAS_POOL_NUMA=0 leaves the pool
// unbound (A/B); nothing is bound when the node or its CPUs cannot be read.
static void bind_pool_to_gpu_node(sd_cas_ctx* c) {
  const char* e = getenv("SD_CAS_POOL_NUMA");
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, c->device) != hipSuccess) return;
  for (char* q = bus; *q; ++q) *q = (char)tolower((unsigned char)*q);
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
  FILE* f = fopen(path, "r");
  int node = -1;
  if (f) {
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
  }
  c->numa_node = node;
  if (node < 0 || (e && strcmp(e, "0") == 0)) return;
  snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  f = fopen(path, "r");
  if (!f) return;
  char list[4096] = {0};
  const bool got = fgets(list, sizeof list, f) != nullptr;
  fclose(f);
  if (!got) return;
  cpu_set_t allowed, cpus;
  CPU_ZERO(&cpus);
  if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
  int n = 0;
  for (char* q = list; *q && *q != '\n';) {  // "0-63,128-191"
    char* end;
    long a = strtol(q, &end, 10), b = a;
    if (end == q) break;
    if (*end == '-') b = strtol(end + 1, &end, 10);
    for (long cpu = a; cpu <= b && cpu < CPU_SETSIZE; ++cpu)
      if (CPU_ISSET(cpu, &allowed)) { CPU_SET(cpu, &cpus); ++n; }
    q = *end == ',' ? end + 1 : end;
  }
  // bind only where the node offers the pool's 16 threads a CPU each (a process confined to a
  // few of the node's CPUs keeps its own placement)
  if (n >= 16) c->pool.set_cpus(cpus, n);
}

int sd_cas_ctx_create(int device, sd_cas_ctx** out) {
  if (!out) return SD_CAS_EINVAL;
  *out = nullptr;
  g_ctx_create_err.clear();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    g_ctx_create_err = "no HIP device " + std::to_string(device) + " (" + std::to_string(ndev) +
                       " visible)";
    return SD_CAS_ENODEV;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    g_ctx_create_err = "hipGetDeviceProperties(" + std::to_string(device) + ") failed";
    return SD_CAS_ENODEV;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {  // gfx950 only
    g_ctx_create_err = std::string("device ") + std::to_string(device) + " is " + prop.gcnArchName +
                       ", not gfx950 (MI355X)";
    return SD_CAS_ENODEV;
  }
  sd_cas_ctx* c = new sd_cas_ctx();
  c->device = device;
  bool failed = hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->copy2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->copy2_done, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->h2d_done, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->packed_h2d, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->packed_done, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming) != hipSuccess ||
      sd_dev_malloc((void**)&c->d_scalar, 64, "d_scalar") != hipSuccess ||
      hipHostMalloc((void**)&c->dupv.note, 64, hipHostMallocDefault) != hipSuccess ||
      sd_dev_malloc((void**)&c->gtotals, GROUP_TOTALS_WORDS * 4, "gtotals") != hipSuccess ||
      hipMemset(c->gtotals, 0, GROUP_TOTALS_WORDS * 4) != hipSuccess ||
      sd_dev_malloc((void**)&c->regions.cursors, 2 * REGION_SET_WORDS * 4, "gcursor") != hipSuccess ||
      hipMemset(c->regions.cursors, 0, 2 * REGION_SET_WORDS * 4) != hipSuccess;
  // per region set its two events, and the path gather's two window slots
  for (hipEvent_t* ev : {&c->regions.done[0], &c->regions.done[1], &c->regions.hashed[0], &c->regions.hashed[1],
                         &c->gather_done[0], &c->gather_done[1]})
    failed = failed || hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess;
  if (failed) {
    sd_cas_ctx_destroy(c);
    g_ctx_create_err = "stream/event/scratch creation failed on device " + std::to_string(device);
    return SD_CAS_EHIP;
  }
  memset(c->dupv.note, 0, 64);
  c->quantum = (size_t)prop.multiProcessorCount * 4 * 64;
  {
    const char* t = getenv("SD_CAS_TRACE");
    c->trace = t && *t && strcmp(t, "0") != 0;
    // test knob: a lower distinct-key bound for the fused chain's region tables, so that the
    // tables' overflow paths (a region's own global table, and a full region's regroup from
    // the whole key array) run on K1G output — uniform BLAKE3 keys never reach the real bound
    const char* f = getenv("SD_CAS_TEST_TABLE_FILL");
    c->test_table_fill = f && *f ? (uint32_t)strtoul(f, nullptr, 10) : 0u;
    //  results stay exact with it set, but every fused grouping then takes the
    // slow overflow paths: never silent
    if (c->test_table_fill)
      fprintf(stderr, "sd_hip_cas: SD_CAS_TEST_TABLE_FILL=%u (test knob): the fused grouping's "
              "region tables overflow at %u distinct keys (exact, much slower)\n",
              c->test_table_fill, c->test_table_fill);
    // the same binary runs either placement of the duplicate compares (A/B, and the fallback)
    const char* p = getenv("SD_CAS_DUP_PLACEMENT");
    if (p && *p) {
      if (strcmp(p, "cu") != 0 && strcmp(p, "static") != 0 && strcmp(p, "auto") != 0) {
        sd_cas_ctx_destroy(c);
        g_ctx_create_err = std::string("SD_CAS_DUP_PLACEMENT=") + p + ": static, cu or auto";
        return SD_CAS_EINVAL;
      }
      c->dupv.placement = !strcmp(p, "cu") ? DUP_PLACE_CU : !strcmp(p, "static") ? DUP_PLACE_STATIC : DUP_PLACE_AUTO;
    }
    // measurement knob: the Object indexes' maximum load (tools/bench_object_index.py sweeps it);
    // results are the same at every value, only table sizes and probe lengths differ
    const char* l = getenv("SD_CAS_INDEX_LOAD_PERCENT");
    const long lv = l && *l ? strtol(l, nullptr, 10) : 0;
    c->index_load_percent = lv >= 10 && lv <= 90 ? (uint32_t)lv : 0u;
  }
  bind_pool_to_gpu_node(c);
  // the pool's readers on private descriptor tables (HostPool::set_private_fds)
  const char* pf = getenv("SD_CAS_POOL_PRIVATE_FDS");
  const bool private_fds = !(pf && pf[0] == '0');
  c->pool.set_private_fds(private_fds);
  if (c->trace)
    fprintf(stderr, "sd_cas_trace ctx device=%d numa_node=%d pool_cpus=%d private_fds=%d\n", device,
            c->numa_node, c->pool.bound_cpus(), (int)private_fds);
  sd_cas_set_latency_threshold(c, SD_CAS_THRESHOLD_DEFAULT, SD_CAS_THRESHOLD_DEFAULT);
  sd_cas_set_chunkpar_split(c, SD_CAS_THRESHOLD_DEFAULT, SD_CAS_THRESHOLD_DEFAULT);
  *out = c;
  return SD_CAS_OK;
}

// Defaults = the measured crossovers on MI355X (profiles/r01_k1l_seg_sweep.log,
// r02_latency_sweep.log): K1L (four files per wave) wins below ~0.75 of a batch quantum for
// sampled messages (49,152 files: 1.11 vs 1.15 ms; 65,536: 1.47 vs 1.19) and below ~2
// quanta for ragged whole files (98,304: 2.47 vs 2.80 ms; 131,072: 3.28 vs 3.24; 163,840:
// 4.08 vs 3.96 — round 2's K2 fast path moved this from ~3 quanta), where the lane-per-file
// K2 waits for the 101-chunk latency of its longest files.
void sd_cas_set_latency_threshold(sd_cas_ctx* c, size_t sampled_files, size_t packed_files) {
  if (!c) return;
  const size_t q = sd_cas_batch_quantum(c);
  c->latency_sampled = sampled_files == SD_CAS_THRESHOLD_DEFAULT ? q * 3 / 4 : sampled_files;
  c->latency_packed = packed_files == SD_CAS_THRESHOLD_DEFAULT ? q * 2 : packed_files;
}

// Defaults = the measured crossovers between the two K1L shapes (profiles/
// r01_k1l_seg_sweep.log): a wave per file while the batch cannot fill the chip's SIMDs,
// four files per wave once the lower wave-compression count per file wins.
void sd_cas_set_chunkpar_split(sd_cas_ctx* c, size_t sampled_files, size_t packed_files) {
  if (!c) return;
  // sampled: crossover between 2,048 (0.078 vs 0.116 ms) and 4,096 files (0.139 vs 0.120);
  // ragged whole files (visited by chunk count, so a wave's 4 files share a chunks-per-lane
  // class; the sort costs ~15 us): between 4,096 (0.216 vs 0.247) and 8,192 (0.364 vs 0.324)
  const size_t q = sd_cas_batch_quantum(c);
  c->seg16_sampled = sampled_files == SD_CAS_THRESHOLD_DEFAULT ? q * 3 / 64 : sampled_files;
  c->seg16_packed = packed_files == SD_CAS_THRESHOLD_DEFAULT ? q * 3 / 32 : packed_files;
}

void sd_cas_ctx_destroy(sd_cas_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  sd_index_free_all(c);
  for (DevBuf* b : {&c->ws, &c->staging, &c->small, &c->cvbuf, &c->io, &c->inplace, &c->dupv.buf, &c->exact,
                    &c->contents})
    if (b->p) (void)sd_dev_free(b->p);
  if (c->dupv.note) (void)hipHostFree(c->dupv.note);
  if (c->d_scalar) (void)sd_dev_free(c->d_scalar);
  if (c->gtotals) (void)sd_dev_free(c->gtotals);
  if (c->regions.cursors) (void)sd_dev_free(c->regions.cursors);
  for (int k = 0; k < 2; k++) {
    if (c->regions.buf[k].p) (void)sd_dev_free(c->regions.buf[k].p);
    for (hipEvent_t ev : {c->regions.done[k], c->regions.hashed[k]})
      if (ev) (void)hipEventDestroy(ev);
  }
  for (hipEvent_t ev : c->gather_done)
    if (ev) (void)hipEventDestroy(ev);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->h2d_done) (void)hipEventDestroy(c->h2d_done);
  if (c->packed_h2d) (void)hipEventDestroy(c->packed_h2d);
  if (c->packed_done) (void)hipEventDestroy(c->packed_done);
  if (c->ws_ev) (void)hipEventDestroy(c->ws_ev);
  if (c->copy) (void)hipStreamDestroy(c->copy);
  if (c->copy2) (void)hipStreamDestroy(c->copy2);
  if (c->copy2_done) (void)hipEventDestroy(c->copy2_done);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* sd_cas_last_error(const sd_cas_ctx* c) {
  return c ? c->err.c_str() : g_ctx_create_err.empty() ? "null context" : g_ctx_create_err.c_str();
}

void* sd_cas_ctx_stream(sd_cas_ctx* c) { return c ? (void*)c->stream : nullptr; }

size_t sd_cas_batch_quantum(const sd_cas_ctx* c) { return c ? c->quantum : 0; }

int sd_cas_set_group_method(sd_cas_ctx* c, int method, uint64_t bucket_target) {
  if (!c) return SD_CAS_EINVAL;
  if (method < SD_CAS_GROUP_AUTO || method > SD_CAS_GROUP_SORT || (bucket_target && bucket_target < 16))
    return fail(c, SD_CAS_EINVAL, "set_group_method: method %d, bucket_target %llu", method,
                (unsigned long long)bucket_target);
  c->group_method = method;
  c->group_target = bucket_target;
  return SD_CAS_OK;
}

int sd_cas_set_dup_verify(sd_cas_ctx* c, int on) {
  if (!c) return SD_CAS_EINVAL;
  if (on != 0 && on != 1) return fail(c, SD_CAS_EINVAL, "set_dup_verify: %d (0 or 1)", on);
  c->dupv.on = on != 0;
  // the next call probes, whatever earlier batches held
  c->dupv.skip = 0;
  c->dupv.seen = ((volatile uint32_t*)c->dupv.note)[0];
  return SD_CAS_OK;
}

int sd_cas_synchronize(sd_cas_ctx* c) {
  if (!c) return SD_CAS_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SD_CAS_OK;
}

int sd_cas_alloc_pinned(sd_cas_ctx* c, size_t bytes, void** out) {
  if (!c || !out) return SD_CAS_EINVAL;
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SD_CAS_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
  }
  return SD_CAS_OK;
}

int sd_cas_free_pinned(sd_cas_ctx* c, void* p) {
  if (!c) return SD_CAS_EINVAL;
  HIP_TRY(c, hipHostFree(p));
  return SD_CAS_OK;
}

// ---- device-resident cas ----------------------------------------------------------

// Sampled batch dispatch.  Below the latency threshold: K1L.  Otherwise K1 over whole batch
// quanta (one file per lane fills every SIMD's wave slots exactly) and the remainder r:
// with K1 as well when r >= the threshold, else K1L after it — a partial K1 wave round
// costs a whole K1 latency however few files it holds (profiles/r01_k1l_seg_sweep.log:
// 98,304 files 2.34 ms on K1 alone vs 1.26 + 0.76 ms split).
hipError_t sd_dispatch_sampled(sd_cas_ctx* c, const uint8_t* content, uint64_t stride,
                               const uint64_t* sizes, size_t n, uint64_t* keys, hipStream_t s) {
  if (n < c->latency_sampled)
    return hash_chunkpar(content, nullptr, stride, nullptr, SAMPLED_CONTENT_LEN, sizes, n, keys,
                         c->chunkpar_seg(n, true), s);
  const size_t q = c->quantum;
  const size_t r = n % q;
  const uint32_t cus = (uint32_t)(q / 256);
  if (n < q || r == 0 || r >= c->latency_sampled) return hash_sampled(content, stride, sizes, n, keys, s, cus);
  const size_t full = n - r;
  hipError_t e = hash_sampled(content, stride, sizes, full, keys, s, cus);
  if (e != hipSuccess) return e;
  return hash_chunkpar(content + full * stride, nullptr, stride, nullptr, SAMPLED_CONTENT_LEN,
                       sizes + full, r, keys + full, c->chunkpar_seg(r, true), s);
}

// Whole-file batch dispatch.  Small batches: K1L, a wave per file, no sort.  Otherwise K2,
// or K1L with 4 files per wave: the files are visited by descending chunk count (one stable
// radix pass) so the lanes of a wave (K2) / the files of a wave (K1L) match.
// workspace: length keys | sorted keys | order | sort workspace
PackedWs sd_packed_layout(void* ws, size_t n) {
  WsCarve w(ws);  PackedWs L;
  L.lkeys = w.take<uint64_t>(n);  L.skeys = w.take<uint64_t>(n);  L.order = w.take<uint32_t>(n);
  L.sort_ws = w.nest(sort_workspace_bytes(n));
  L.bytes = w.bytes();  return L;
}
size_t sd_packed_workspace_bytes(const sd_cas_ctx* c, size_t n) {
  if (n < c->latency_packed && c->chunkpar_seg(n, false) == 64) return 0;
  return sd_packed_layout(nullptr, n).bytes;
}

hipError_t sd_dispatch_packed(sd_cas_ctx* c, const uint8_t* arena, const uint64_t* offs,
                              const uint32_t* lens, const uint64_t* sizes, size_t n, uint64_t* keys,
                              hipStream_t s) {
  const bool k1l = n < c->latency_packed;
  if (k1l && c->chunkpar_seg(n, false) == 64)
    return hash_chunkpar(arena, offs, 0, lens, 0, sizes, n, keys, 64, s);
  // intended aliasing: the start of c->ws, whichever call's part of it the caller acquired
  const PackedWs L = sd_packed_layout(c->ws.p, n);
  hipError_t e = length_keys(lens, n, L.lkeys, s);
  if (e == hipSuccess)
    e = radix_sort_pairs(L.lkeys, nullptr, L.skeys, L.order, n, 0, length_key_bits(n), L.sort_ws, s);
  if (e != hipSuccess) return e;
  if (k1l) return hash_chunkpar(arena, offs, 0, lens, 0, sizes, n, keys, 16, s, L.order);
  return hash_packed(arena, offs, lens, sizes, L.order, n, keys, s);
}

int sd_cas_hash_sampled_dev(sd_cas_ctx* c, const void* d_content, uint64_t stride,
                            const uint64_t* d_sizes, size_t n, uint64_t* d_keys, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!d_content || !d_sizes || !d_keys || stride < SAMPLED_CONTENT_LEN || (stride & 15) ||
      ((uintptr_t)d_content & 15))
    return fail(c, SD_CAS_EINVAL, "hash_sampled: bad content/stride (stride=%llu)",
                (unsigned long long)stride);
  HIP_TRY(c, sd_dispatch_sampled(c, (const uint8_t*)d_content, stride, d_sizes, n, d_keys,
                              pick(c, stream)));
  return SD_CAS_OK;
}

int sd_cas_hash_packed_dev(sd_cas_ctx* c, const void* d_arena, const uint64_t* d_offs,
                           const uint32_t* d_lens, const uint64_t* d_sizes, size_t n,
                           uint64_t* d_keys, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!d_arena || !d_offs || !d_lens || !d_sizes || !d_keys || ((uintptr_t)d_arena & 15) ||
      n >= (1ull << 32))
    return fail(c, SD_CAS_EINVAL, "hash_packed: bad arguments");
  hipStream_t s = pick(c, stream);
  const size_t wsb = sd_packed_workspace_bytes(c, n);
  if (wsb == 0) {  // small batch: no sort, no workspace
    HIP_TRY(c, sd_dispatch_packed(c, (const uint8_t*)d_arena, d_offs, d_lens, d_sizes, n, d_keys, s));
    return SD_CAS_OK;
  }
  int rc = ensure(c, c->ws, wsb);
  if (rc) return rc;
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, sd_dispatch_packed(c, (const uint8_t*)d_arena, d_offs, d_lens, d_sizes, n, d_keys, s));
  HIP_TRY(c, ws.release());
  return SD_CAS_OK;
}

// ---- hex helpers ---------------------------------------------------------------------

void sd_cas_key_to_hex(uint64_t key, char out[17]) {
  static const char* hx = "0123456789abcdef";
  for (int i = 0; i < 16; i++) out[i] = hx[(key >> (60 - 4 * i)) & 15];
  out[16] = 0;
}

static int hex_nibble(char ch) {
  return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10
       : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
}

int sd_cas_digest_from_hex(const char* hex, uint8_t out[32]) {
  if (!hex || !out) return SD_CAS_EINVAL;
  uint8_t d[32];
  for (int i = 0; i < 32; i++) {  // stops at the first byte that is no hex digit (a NUL included)
    const int hi = hex_nibble(hex[2 * i]);
    if (hi < 0) return SD_CAS_EINVAL;
    const int lo = hex_nibble(hex[2 * i + 1]);
    if (lo < 0) return SD_CAS_EINVAL;
    d[i] = (uint8_t)(hi << 4 | lo);
  }
  if (hex[64] != 0) return SD_CAS_EINVAL;
  memcpy(out, d, 32);
  return SD_CAS_OK;
}

void sd_cas_digest_to_hex(const uint8_t digest[32], char out[65]) { sd_hex32(digest, out); }

// ---- synthetic inputs ----------------------------------------------------------------

int sd_cas_synth_sampled_dev(sd_cas_ctx* c, uint64_t seed, uint64_t file0, size_t n,
                             uint32_t dup_permille, void* d_content, uint64_t stride,
                             uint64_t* d_sizes, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!d_content || !d_sizes || stride < SAMPLED_CONTENT_LEN || (stride & 15) || dup_permille > 1000)
    return fail(c, SD_CAS_EINVAL, "synth_sampled: bad arguments");
  HIP_TRY(c, synth_sampled(seed, file0, n, dup_permille, (uint8_t*)d_content, stride, d_sizes,
                           pick(c, stream)));
  return SD_CAS_OK;
}

int sd_cas_synth_small_dev(sd_cas_ctx* c, uint64_t seed, uint64_t file0, size_t n,
                           uint32_t dup_permille, uint64_t* d_sizes, uint32_t* d_lens,
                           uint64_t* d_offs, void* d_arena, uint64_t* out_arena_bytes,
                           void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (!d_sizes || !d_lens || !d_offs || dup_permille > 1000)
    return fail(c, SD_CAS_EINVAL, "synth_small: bad arguments");
  hipStream_t s = pick(c, stream);
  if (n == 0) { if (out_arena_bytes) *out_arena_bytes = 16; return SD_CAS_OK; }
  HIP_TRY(c, synth_small_sizes(seed, file0, n, dup_permille, d_sizes, d_lens, s));
  // offsets: 128-B aligned packing (see up128), computed on the host from the lens
  std::vector<uint32_t> lens(n);
  HIP_TRY(c, hipMemcpyAsync(lens.data(), d_lens, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  std::vector<uint64_t> offs(n);
  uint64_t o = 0;
  for (size_t i = 0; i < n; i++) { offs[i] = o; o += up128(lens[i]); }
  o += 16;
  if (out_arena_bytes) *out_arena_bytes = o;
  HIP_TRY(c, hipMemcpyAsync(d_offs, offs.data(), n * 8, hipMemcpyHostToDevice, s));
  if (d_arena) HIP_TRY(c, synth_small_content(seed, file0, n, dup_permille, d_offs, d_lens,
                                              (uint8_t*)d_arena, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

int sd_cas_synth_small_content_dev(sd_cas_ctx* c, uint64_t seed, uint64_t file0, size_t n,
                                   uint32_t dup_permille, const uint64_t* d_offs,
                                   const uint32_t* d_lens, void* d_arena, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (!d_offs || !d_lens || !d_arena || dup_permille > 1000 || ((uintptr_t)d_arena & 15))
    return fail(c, SD_CAS_EINVAL, "synth_small_content: bad arguments");
  if (n == 0) return SD_CAS_OK;
  HIP_TRY(c, synth_small_content(seed, file0, n, dup_permille, d_offs, d_lens,
                                 (uint8_t*)d_arena, pick(c, stream)));
  return SD_CAS_OK;
}

int sd_cas_synth_stream_dev(sd_cas_ctx* c, uint64_t seed, uint64_t file, uint64_t byte_off,
                            uint64_t len, void* d_out, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (len && (!d_out || (byte_off & 7) || ((uintptr_t)d_out & 7)))
    return fail(c, SD_CAS_EINVAL, "synth_stream: bad arguments");
  HIP_TRY(c, synth_stream(seed, file, byte_off, len, (uint8_t*)d_out, pick(c, stream)));
  return SD_CAS_OK;
}

int sd_cas_synth_roots_dev(sd_cas_ctx* c, uint64_t seed, uint64_t file0, size_t n,
                           uint32_t dup_permille, uint64_t* d_roots, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n && !d_roots) return fail(c, SD_CAS_EINVAL, "synth_roots: null");
  HIP_TRY(c, synth_roots(seed, file0, n, dup_permille, d_roots, pick(c, stream)));
  return SD_CAS_OK;
}

}  // extern "C"
