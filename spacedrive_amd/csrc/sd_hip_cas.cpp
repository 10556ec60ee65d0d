// sd_hip_cas.cpp — the C ABI (include/sd_hip_cas.h) over the gfx950 kernels: contexts,
// device-resident cas, grouping, the fused chain, link emission, synthetic inputs (the
// host-buffer/path entry points are in host_paths.cpp, the validator's in validator_host.cpp).
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
#include <errno.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "sd_checksum.h"
#include "sd_content_compare.h"
#include "sd_exact_dups.h"
#include "sd_group.h"
#include "sd_dup_runs.h"
#include "sd_kernels.h"
#include "sd_links.h"
#include "sd_mix.h"
#include "sd_object_stats.h"
#include "sd_synth.h"

using namespace sdcas;

#include "sd_debug.h"
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
}  // namespace sdcas
// debug library only (libsd_hip_cas_debug.so, not in the ABI header): invariant violations
// counted by the device checks of sd_debug.h since the library was loaded
// ... plus the allocation tails found changed (below)
#include "ctx_internal.h"
extern "C" uint64_t sd_cas_debug_violations(void) {
  return (uint64_t)sd_dbg_violations_group_hash() + sd_dbg_violations_cas_hash() +
         sd_dbg_violations_dup_verify() + sd_dbg_violations_group() +
         sd_dbg_violations_checksum() + sd_dbg_violations_links() + sd_dbg_violations_inplace() +
         sd_dbg_violations_object_stats() + sd_dbg_violations_exact_dups() +
         sd_dbg_violations_content_compare() + sd_dbg_tail_check_all();
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

#include "ctx_internal.h"

// short local names for the shared helpers
#define fail sd_fail
#define pick sd_pick
#define ensure sd_ensure
#define ensure_pinned sd_ensure_pinned

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
  if (hipSetDevice(device) != hipSuccess ||
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
      sd_dev_malloc((void**)&c->gcursor, 2 * REGION_SET_WORDS * 4, "gcursor") != hipSuccess ||
      hipMemset(c->gcursor, 0, 2 * REGION_SET_WORDS * 4) != hipSuccess ||
      hipEventCreateWithFlags(&c->region_done[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->region_done[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->region_hashed[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->region_hashed[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->gather_done[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->gather_done[1], hipEventDisableTiming) != hipSuccess) {
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
  if (c->ws.p) (void)sd_dev_free(c->ws.p);
  if (c->staging.p) (void)sd_dev_free(c->staging.p);
  if (c->small.p) (void)sd_dev_free(c->small.p);
  if (c->cvbuf.p) (void)sd_dev_free(c->cvbuf.p);
  if (c->io.p) (void)sd_dev_free(c->io.p);
  if (c->inplace.p) (void)sd_dev_free(c->inplace.p);
  if (c->dupv.buf.p) (void)sd_dev_free(c->dupv.buf.p);
  if (c->exact.p) (void)sd_dev_free(c->exact.p);
  if (c->contents.p) (void)sd_dev_free(c->contents.p);
  if (c->dupv.note) (void)hipHostFree(c->dupv.note);
  if (c->d_scalar) (void)sd_dev_free(c->d_scalar);
  if (c->gtotals) (void)sd_dev_free(c->gtotals);
  if (c->gcursor) (void)sd_dev_free(c->gcursor);
  for (int k = 0; k < 2; k++) {
    if (c->regions[k].p) (void)sd_dev_free(c->regions[k].p);
    if (c->region_done[k]) (void)hipEventDestroy(c->region_done[k]);
    if (c->region_hashed[k]) (void)hipEventDestroy(c->region_hashed[k]);
  }
  for (int b = 0; b < 2; b++)
    if (c->gather_done[b]) (void)hipEventDestroy(c->gather_done[b]);
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

void sd_cas_key_to_hex(uint64_t key, char out[17]) {
  static const char* hx = "0123456789abcdef";
  for (int i = 0; i < 16; i++) out[i] = hx[(key >> (60 - 4 * i)) & 15];
  out[16] = 0;
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
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, sd_dispatch_packed(c, (const uint8_t*)d_arena, d_offs, d_lens, d_sizes, n, d_keys, s));
  HIP_TRY(c, sd_ws_release(c, s));
  return SD_CAS_OK;
}

// ---- grouping -----------------------------------------------------------------------

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
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, radix_sort_pairs(d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, begin_bit, end_bit,
                              c->ws.p, s));
  HIP_TRY(c, sd_ws_release(c, s));
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
  if (c->use_hash_group(n)) {  // K4h/K5h: bucket partition + LDS hash min (no full sort)
    int rc = ensure(c, c->ws, hash_group_workspace_bytes(n, c->group_target));
    if (rc) return rc;
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, hash_group_min(d_keys, nullptr, n, d_rep, c->d_scalar, c->ws.p, c->gtotals, s,
                              c->group_target));
  } else {  // beyond the hash grouping's range: LSD radix sort + run heads (K4 + K5)
    int rc = ensure(c, c->ws, group_workspace_bytes(n));
    if (rc) return rc;
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, group_keys(d_keys, n, d_rep, c->d_scalar, c->ws.p, s));
  }
  HIP_TRY(c, sd_ws_release(c, s));
  c->region_obj_set = -1;
  if (out_objects) {
    HIP_TRY(c, hipMemcpyAsync(out_objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SD_CAS_OK;
}

// ---- the fused hash + group chain -------------------------------------------------
static bool fused_eligible(const sd_cas_ctx* c, size_t n) {
  return n && n % c->quantum == 0 && region_group_supported(n) &&
         (c->group_method == SD_CAS_GROUP_AUTO || c->group_method == SD_CAS_GROUP_HASH) &&
         c->group_target == 0;
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
  const int k = (c->region_cur + 1) & 1;
  // set k was last grouped two batches ago: its tables must be done before it is refilled;
  // a batch hashed into it but never grouped: its K1G (on whatever stream) must be done
  if (c->region_pending[k]) HIP_TRY(c, hipStreamWaitEvent(s, c->region_done[k], 0));
  if (!c->region_grouped[k]) {
    HIP_TRY(c, hipStreamWaitEvent(s, c->region_hashed[k], 0));
    // its cursors and spill count were left counted: clear them
    HIP_TRY(c, hipMemsetAsync(c->gcursor + REGION_SET_WORDS * k, 0, REGION_SET_WORDS * 4, s));
  }
  if (c->region_obj_set == k) {
    // set k holds the Object count of the context's last grouping, which this refill's K1G
    // zeroes: keep it in d_scalar for sd_cas_copy_objects_dev
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_scalar, region_group_layout(c->regions[k].p, c->region_n[k]).objects, 8,
                              hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, sd_ws_release(c, s));
    c->region_obj_set = -1;
  }
  c->region_n[k] = n;  // sizes the layout (ensure below grows the set if needed)
  int rc = ensure(c, c->regions[k], region_group_workspace_bytes(n));
  if (rc) return rc;
  uint32_t* cur = c->gcursor + REGION_SET_WORDS * k;
  const RegionOut ro = region_out(region_group_layout(c->regions[k].p, c->region_n[k]), cur,
                                  region_capacity(n), d_rep, d_overflow);
  const uint32_t cus = (uint32_t)(c->quantum / 256);
  hipError_t e;
  if (dup_verify_this_call(c->dupv)) {  // K1V: duplicate contents are compared, not hashed
    DupVerifyState& v = c->dupv;
    if ((rc = ensure(c, v.buf, dup_verify_workspace_bytes(n)))) return rc;
    if ((rc = ensure(c, c->ws, hash_group_workspace_bytes(n)))) return rc;
    // the last call's lists, on another stream: after its chain (the other set's event)
    if (v.n && v.stream != s && c->region_cur >= 0)
      HIP_TRY(c, hipStreamWaitEvent(s, c->region_hashed[c->region_cur], 0));
    const DupVerifyWs D = dup_verify_layout(v.buf.p, n);
    HIP_TRY(c, sd_ws_acquire(c, s));  // the probes' grouping runs in ws / gtotals
    e = dup_candidates((const uint8_t*)d_content, stride, d_sizes, n, D, c->ws.p, c->gtotals, s);
    HIP_TRY(c, sd_ws_release(c, s));
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
  HIP_TRY(c, hipEventRecord(c->region_hashed[k], s));
  c->region_keys[k] = d_keys;
  c->region_cur = k;
  c->region_grouped[k] = false;
  return SD_CAS_OK;
}

// the counters of the context's last hash_regions call (zeros when it did not verify duplicates)
static int dup_verify_words(sd_cas_ctx* c, uint32_t (&h)[DUP_COUNTERS]) {
  if (c->dupv.n && c->region_cur >= 0) {  // the last hash_regions call verified duplicates
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->region_hashed[c->region_cur], 0));
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
  const int k = c->region_cur;
  if (k < 0 || c->region_grouped[k] || c->region_n[k] != n || !d_rep)
    return fail(c, SD_CAS_EINVAL, "group_regions: no ungrouped hash_regions batch of %zu files", n);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick(c, stream);
  const RegionGroupWs L = region_group_layout(c->regions[k].p, c->region_n[k]);
  uint32_t* cur = c->gcursor + REGION_SET_WORDS * k;
  HIP_TRY(c, hipStreamWaitEvent(s, c->region_hashed[k], 0));  // after its K1G, whatever stream
  hipError_t e = region_group_min(L, region_out(L, cur, region_capacity(n), d_rep, nullptr), c->region_keys[k], n,
                                  c->test_table_fill, s);
  if (e != hipSuccess) {
    (void)hipMemsetAsync(cur, 0, REGION_SET_WORDS * 4, s);
    return fail(c, SD_CAS_EHIP, "group_regions: %s", hipGetErrorString(e));
  }
  HIP_TRY(c, hipEventRecord(c->region_done[k], s));
  c->region_pending[k] = true;
  c->region_grouped[k] = true;
  c->region_obj_set = k;
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

int sd_cas_group_min_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint32_t* d_vals, size_t n,
                         uint32_t* d_out, uint64_t* out_objects, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n >= (1ull << 32) || (n && (!d_keys || !d_out)))
    return fail(c, SD_CAS_EINVAL, "group_min: bad arguments");
  if (c->group_method == SD_CAS_GROUP_HASH && !hash_group_supported(n))
    return fail(c, SD_CAS_EINVAL, "group_min: %zu keys exceed the hash grouping's range", n);
  hipStream_t s = pick(c, stream);
  if (c->use_hash_group(n)) {
    int rc = ensure(c, c->ws, hash_group_workspace_bytes(n, c->group_target));
    if (rc) return rc;
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, hash_group_min(d_keys, d_vals, n, d_out, c->d_scalar, c->ws.p, c->gtotals, s,
                              c->group_target));
  } else {  // beyond the hash grouping's range: stable LSD sort of (key, val) + run minima
    int rc = ensure(c, c->ws, group_min_sorted_workspace_bytes(n));
    if (rc) return rc;
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, group_min_by_sort(d_keys, d_vals, n, d_out, c->d_scalar, c->ws.p, s));
  }
  HIP_TRY(c, sd_ws_release(c, s));
  c->region_obj_set = -1;
  if (out_objects) {
    HIP_TRY(c, hipMemcpyAsync(out_objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SD_CAS_OK;
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
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, partition_range(d_keys, n, parts, d_keys_out, d_pos_out, d_counts, c->ws.p, s));
  HIP_TRY(c, sd_ws_release(c, s));
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
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, group_sorted(d_sorted_keys, d_sorted_vals, n, d_rep, c->d_scalar, c->ws.p, s));
  HIP_TRY(c, sd_ws_release(c, s));
  c->region_obj_set = -1;
  if (out_objects) {
    HIP_TRY(c, hipMemcpyAsync(out_objects, c->d_scalar, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return SD_CAS_OK;
}

int sd_cas_group_chunked_dev(sd_cas_ctx* c, const uint32_t* d_rep, size_t n, uint32_t chunk,
                             uint32_t* d_rep_chunked, uint64_t* out_created,
                             uint64_t* out_linked, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (chunk == 0 || n >= (1ull << 32) || (n && (!d_rep || !d_rep_chunked)))
    return fail(c, SD_CAS_EINVAL, "group_chunked: bad arguments");
  hipStream_t s = pick(c, stream);
  uint64_t* d_created = c->d_scalar + 1;
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, hipMemsetAsync(d_created, 0, 8, s));
  HIP_TRY(c, group_chunked(d_rep, n, chunk, d_rep_chunked, d_created, s));
  HIP_TRY(c, sd_ws_release(c, s));
  uint64_t created = 0;
  HIP_TRY(c, hipMemcpyAsync(&created, d_created, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (out_created) *out_created = created;
  if (out_linked) *out_linked = n - created;
  return SD_CAS_OK;
}

// ---- Object-link emission (file_identifier_job.rs:180-236, mod.rs:98-350) -------------

static_assert(SD_CAS_ROW_HASHED == SD_LINKS_HASHED && SD_CAS_ROW_NO_CAS == SD_LINKS_NO_CAS &&
                  SD_CAS_ROW_ERROR == SD_LINKS_ERROR && SD_CAS_LINK_CREATED == SD_LINKS_CREATED &&
                  SD_CAS_LINK_LINKED == SD_LINKS_LINKED && SD_CAS_LINK_DROPPED == SD_LINKS_DROPPED &&
                  SD_CAS_LINK_NOT_REACHED == SD_LINKS_NOT_REACHED &&
                  SD_CAS_LINK_EXISTING == SD_LINKS_EXISTING &&
                  SD_CAS_NO_STEP == SD_LINKS_NO_STEP && SD_CAS_NO_OBJECT == SD_LINKS_NO_OBJECT,
              "link constants");

size_t sd_cas_identifier_max_steps(size_t n, uint32_t chunk) {
  return chunk ? (n + chunk - 1) / chunk : 0;
}

// the link emission's staging: rep | hkeys | hrows | minrow | orphans | starts | counts |
// [event block offsets | scan tiles | key filter] | 4 counters (hashed rows, orphan rows, waves
// with a bad Object id, events); the seeded grouping runs over the n hashed rows + the n_seed
// existing Objects' keys.  The bracketed sections serve rows with pre-existing Objects (pre) and
// take no room without them; such rows reuse the grouping's buffers once it is done: events
// (hkeys / hrows), sorted events (orphans / minrow), scan elements (hkeys).
LinkStagingWs sd_link_staging_layout(void* base, size_t n, size_t n_seed, size_t steps_total, bool pre) {
  const size_t m = n + n_seed;
  WsCarve w(base);  LinkStagingWs L;
  L.rep = w.take<uint32_t>(n);  L.hkeys = w.take<uint64_t>(m);
  L.hrows = w.take<uint32_t>(m);  L.minrow = w.take<uint32_t>(m);
  L.orphans = w.take<uint64_t>(n);  L.starts = w.take<uint32_t>(steps_total + 1);
  L.counts = w.take<uint32_t>(2 * steps_total);  L.boff = w.take<uint32_t>(pre ? pre_blocks(n) : 0);
  L.tiles = w.take<uint64_t>(pre ? segmin_tiles_bytes(n) / 8 : 0);
  L.filter = w.take<uint32_t>(pre ? pre_filter_bytes() / 4 : 0);  L.counters = w.take<uint64_t>(4);
  L.bytes = w.bytes();  return L;
}
// the host forms' device copies of their arrays (c->io)
LinkIoWs sd_link_io_layout(void* base, size_t n, size_t n_seed, bool pre) {
  WsCarve w(base);  LinkIoWs L;
  L.keys = w.take<uint64_t>(n);  L.state = w.take<uint8_t>(n);
  L.step = w.take<uint32_t>(n);  L.object = w.take<uint32_t>(n);
  L.action = w.take<uint8_t>(n);  L.seed_keys = w.take<uint64_t>(n_seed);
  L.seed_objects = w.take<uint32_t>(n_seed);  L.pre = pre ? w.take<uint32_t>(n) : nullptr;
  L.bytes = w.bytes();  return L;
}

int sd_cas_identifier_links_ex_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                   size_t n, uint32_t chunk, const uint64_t* d_seed_keys,
                                   const uint32_t* d_seed_objects, size_t n_seed,
                                   const uint32_t* d_pre_objects, uint32_t* d_step,
                                   uint32_t* d_object, uint8_t* d_action, uint64_t* h_step_counts,
                                   size_t max_steps, uint64_t* out_steps, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  const size_t steps_total = sd_cas_identifier_max_steps(n, chunk);
  if (chunk == 0 || n >= (1ull << 32) || !out_steps || max_steps < steps_total ||
      (n && (!d_keys || !d_step || !d_object || !d_action || !h_step_counts)) ||
      (n_seed && (!d_seed_keys || !d_seed_objects)))
    return fail(c, SD_CAS_EINVAL, "identifier_links: bad arguments");
  // a seeded grouping tags rows with LINKS_ROW_FLAG: rows and Object ids below 2^31 (rows
  // that already own an Object run the seeded grouping too)
  const bool seeded = n_seed > 0 || d_pre_objects;
  if (seeded && (n >= LINKS_ROW_FLAG || n_seed >= LINKS_ROW_FLAG || n + n_seed >= (1ull << 32)))
    return fail(c, SD_CAS_EINVAL, "identifier_links: %zu rows + %zu existing Objects exceed 2^31",
                n, n_seed);
  *out_steps = 0;
  for (size_t k = 0; k < 2 * steps_total; k++) h_step_counts[k] = 0;
  if (n == 0) return SD_CAS_OK;
  hipStream_t s = pick(c, stream);
  // (this call is blocking)
  int rc = ensure(c, c->staging,
                  sd_link_staging_layout(nullptr, n, n_seed, steps_total, d_pre_objects != nullptr).bytes);
  if (rc) return rc;
  const LinkStagingWs L = sd_link_staging_layout(c->staging.p, n, n_seed, steps_total, d_pre_objects != nullptr);
  // 1. grouping over the hashed rows (rep = the key's first row; seeded: the lowest existing
  //    Object id when the key has one — mod.rs:180-198 finds Objects by cas over the whole
  //    library), and the rows that stay orphan after being processed (they steer the cursor)
  std::vector<uint64_t> stay;  // row << 8 | state, ascending
  if (d_state || seeded) {
    uint64_t cnt[3] = {0, 0, 0};
    HIP_TRY(c, hipMemsetAsync(L.counters, 0, 32, s));
    HIP_TRY(c, links_check_ids(d_seed_objects, n_seed, false, L.counters + 2, s));
    if (d_pre_objects) HIP_TRY(c, links_check_ids(d_pre_objects, n, true, L.counters + 2, s));
    HIP_TRY(c, links_split(d_keys, d_state, n, L.hkeys, L.hrows, L.counters, L.orphans, L.counters + 1,
                           seeded ? LINKS_ROW_FLAG : 0u, s));
    HIP_TRY(c, hipMemcpyAsync(cnt, L.counters, 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (cnt[2])
      return fail(c, SD_CAS_EINVAL, "identifier_links: an existing Object id is >= 2^31");
    stay.resize(cnt[1]);
    if (cnt[1]) {
      HIP_TRY(c, hipMemcpyAsync(stay.data(), L.orphans, cnt[1] * 8, hipMemcpyDeviceToHost, s));
    }
    if (n_seed) {  // the existing Objects' (cas key, id) pairs after the hashed rows
      HIP_TRY(c, hipMemcpyAsync(L.hkeys + cnt[0], d_seed_keys, n_seed * 8, hipMemcpyDeviceToDevice, s));
      HIP_TRY(c, hipMemcpyAsync(L.hrows + cnt[0], d_seed_objects, n_seed * 4, hipMemcpyDeviceToDevice, s));
    }
    if (cnt[0]) {
      if ((rc = sd_cas_group_min_dev(c, L.hkeys, L.hrows, cnt[0] + n_seed, L.minrow, nullptr, s))) return rc;
      HIP_TRY(c, links_scatter(L.minrow, L.hrows, cnt[0], L.rep, seeded ? LINKS_ROW_FLAG : 0u, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    std::sort(stay.begin(), stay.end());
  } else {
    if ((rc = sd_cas_group_dev(c, d_keys, n, L.rep, nullptr, s))) return rc;
  }
  // 2. the cursor walk (host; O(steps + orphans)): step k covers [start, start + chunk);
  //    the next cursor is its last row, which the next query returns again iff it is
  //    still orphan; an empty query ends the job
  // the rows asked about only increase (each step's last row), so one forward pointer into
  // the sorted orphan list answers them all: O(steps + orphans) (a binary search per step
  // cost ~2 ms of a 10 M-row job)
  size_t sp = 0;
  auto stays = [&](uint64_t row, uint8_t* st) {
    while (sp < stay.size() && (stay[sp] >> 8) < row) ++sp;
    if (sp == stay.size() || (stay[sp] >> 8) != row) return false;
    *st = (uint8_t)(stay[sp] & 0xFF);
    return true;
  };
  std::vector<uint32_t> h_starts;
  h_starts.reserve(steps_total + 1);
  std::vector<uint64_t> extra(steps_total, 0);  // re-queried empty rows: one creation per step
  uint64_t start = 0, reached = 0;
  for (size_t k = 0; k < steps_total && start < n; k++) {
    h_starts.push_back((uint32_t)start);
    const uint64_t end = std::min<uint64_t>(start + chunk, n), last = end - 1;
    reached = end;
    uint8_t st = 0;
    if (stays(last, &st)) {
      if (st == SD_CAS_ROW_NO_CAS && k + 1 < steps_total) extra[k] += 1;
      start = last;
    } else {
      start = end;
    }
  }
  const size_t nsteps = h_starts.size();
  h_starts.push_back(0xFFFFFFFFu);  // sentinel
  HIP_TRY(c, hipMemcpyAsync(L.starts, h_starts.data(), h_starts.size() * 4, hipMemcpyHostToDevice, s));
  // 3. rows that already own an Object (links.hip, sd_links_pre_*): the events — hashed rows
  //    of the reached steps that hold an Object — compacted in row order, sorted stably by key,
  //    and scanned; each hashed row then looks its key up in the decision kernel
  uint64_t n_ev = 0;
  if (d_pre_objects) {
    HIP_TRY(c, links_pre_count(d_state, d_pre_objects, reached, L.boff, L.counters + 3, s));
    HIP_TRY(c, hipMemcpyAsync(&n_ev, L.counters + 3, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  if (n_ev) {
    HIP_TRY(c, hipMemsetAsync(L.filter, 0, pre_filter_bytes(), s));
    HIP_TRY(c, links_pre_emit(d_keys, d_state, d_pre_objects, reached, L.boff, L.hkeys, L.hrows, L.filter, s));
    uint64_t* skeys = L.orphans;
    uint32_t* srows = L.minrow;
    if ((rc = sd_cas_sort_pairs_dev(c, L.hkeys, L.hrows, n_ev, skeys, srows, 0, 64, s))) return rc;
    HIP_TRY(c, links_pre_scan(skeys, srows, d_pre_objects, n_ev, L.starts, (uint32_t)nsteps, L.hkeys,
                              L.tiles, s));
  }
  // 4. per-row decisions + per-step counts (device)
  HIP_TRY(c, hipMemsetAsync(L.counts, 0, std::max<size_t>(nsteps, 1) * 8, s));
  HIP_TRY(c, links_decide(d_state, L.rep, n, L.starts, (uint32_t)nsteps, reached, d_step, d_object,
                          d_action, L.counts, seeded, d_keys, L.orphans, L.minrow, L.hkeys, L.filter, n_ev,
                          (uint32_t)chunk, s));
  std::vector<uint32_t> hc(2 * std::max<size_t>(nsteps, 1));
  HIP_TRY(c, hipMemcpyAsync(hc.data(), L.counts, hc.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  for (size_t k = 0; k < nsteps; k++) {
    h_step_counts[2 * k] = hc[2 * k] + extra[k];
    h_step_counts[2 * k + 1] = hc[2 * k + 1];
  }
  *out_steps = nsteps;
  return SD_CAS_OK;
}

int sd_cas_identifier_links_seeded_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                       size_t n, uint32_t chunk, const uint64_t* d_seed_keys,
                                       const uint32_t* d_seed_objects, size_t n_seed, uint32_t* d_step,
                                       uint32_t* d_object, uint8_t* d_action, uint64_t* h_step_counts,
                                       size_t max_steps, uint64_t* out_steps, void* stream) {
  return sd_cas_identifier_links_ex_dev(c, d_keys, d_state, n, chunk, d_seed_keys, d_seed_objects,
                                        n_seed, nullptr, d_step, d_object, d_action, h_step_counts,
                                        max_steps, out_steps, stream);
}

int sd_cas_identifier_links_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                size_t n, uint32_t chunk, uint32_t* d_step, uint32_t* d_object,
                                uint8_t* d_action, uint64_t* h_step_counts, size_t max_steps,
                                uint64_t* out_steps, void* stream) {
  return sd_cas_identifier_links_seeded_dev(c, d_keys, d_state, n, chunk, nullptr, nullptr, 0, d_step,
                                            d_object, d_action, h_step_counts, max_steps, out_steps,
                                            stream);
}

int sd_cas_identifier_links_ex(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                               size_t n, uint32_t chunk, const uint64_t* h_seed_keys,
                               const uint32_t* h_seed_objects, size_t n_seed,
                               const uint32_t* h_pre_objects, uint32_t* h_step, uint32_t* h_object,
                               uint8_t* h_action, uint64_t* h_step_counts, size_t max_steps,
                               uint64_t* out_steps) {
  if (!c) return SD_CAS_EINVAL;
  if ((n && (!h_keys || !h_step || !h_object || !h_action)) ||
      (n_seed && (!h_seed_keys || !h_seed_objects)))
    return fail(c, SD_CAS_EINVAL, "identifier_links: bad arguments");
  for (size_t j = 0; j < n_seed; j++)
    if (h_seed_objects[j] >= LINKS_ROW_FLAG)
      return fail(c, SD_CAS_EINVAL, "identifier_links: existing Object id %u >= 2^31", h_seed_objects[j]);
  if (h_pre_objects)
    for (size_t i = 0; i < n; i++)
      if (h_pre_objects[i] >= LINKS_ROW_FLAG && h_pre_objects[i] != SD_CAS_NO_OBJECT)
        return fail(c, SD_CAS_EINVAL, "identifier_links: row %zu's Object id %u >= 2^31", i,
                    h_pre_objects[i]);
  if (n == 0 || n >= (1ull << 32))
    return sd_cas_identifier_links_dev(c, nullptr, nullptr, n, chunk, nullptr, nullptr, nullptr,
                                       h_step_counts, max_steps, out_steps, c->stream);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure(c, c->io, sd_link_io_layout(nullptr, n, n_seed, h_pre_objects != nullptr).bytes);
  if (rc) return rc;
  const LinkIoWs L = sd_link_io_layout(c->io.p, n, n_seed, h_pre_objects != nullptr);
  uint8_t* d_state = h_state ? L.state : nullptr;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(L.keys, h_keys, n * 8, hipMemcpyHostToDevice, s));
  if (h_state) HIP_TRY(c, hipMemcpyAsync(d_state, h_state, n, hipMemcpyHostToDevice, s));
  if (n_seed) {
    HIP_TRY(c, hipMemcpyAsync(L.seed_keys, h_seed_keys, n_seed * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(L.seed_objects, h_seed_objects, n_seed * 4, hipMemcpyHostToDevice, s));
  }
  if (L.pre) HIP_TRY(c, hipMemcpyAsync(L.pre, h_pre_objects, n * 4, hipMemcpyHostToDevice, s));
  rc = sd_cas_identifier_links_ex_dev(c, L.keys, d_state, n, chunk, L.seed_keys, L.seed_objects,
                                      n_seed, L.pre, L.step, L.object, L.action, h_step_counts,
                                      max_steps, out_steps, s);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(h_step, L.step, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(h_object, L.object, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(h_action, L.action, n, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

int sd_cas_identifier_links_seeded(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                                   size_t n, uint32_t chunk, const uint64_t* h_seed_keys,
                                   const uint32_t* h_seed_objects, size_t n_seed, uint32_t* h_step,
                                   uint32_t* h_object, uint8_t* h_action, uint64_t* h_step_counts,
                                   size_t max_steps, uint64_t* out_steps) {
  return sd_cas_identifier_links_ex(c, h_keys, h_state, n, chunk, h_seed_keys, h_seed_objects, n_seed,
                                    nullptr, h_step, h_object, h_action, h_step_counts, max_steps,
                                    out_steps);
}

int sd_cas_identifier_links(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                            size_t n, uint32_t chunk, uint32_t* h_step, uint32_t* h_object,
                            uint8_t* h_action, uint64_t* h_step_counts, size_t max_steps,
                            uint64_t* out_steps) {
  return sd_cas_identifier_links_seeded(c, h_keys, h_state, n, chunk, nullptr, nullptr, 0, h_step,
                                        h_object, h_action, h_step_counts, max_steps, out_steps);
}

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
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, object_stats(d_rep, d_sizes, d_state, n, d_copies, d_totals, L.shards, s));
  if (out_totals)
    HIP_TRY(c, hipMemcpyAsync(out_totals, d_totals, SD_CAS_STAT_COUNT * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, sd_ws_release(c, s));
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
  HIP_TRY(c, sd_ws_acquire(c, s));
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
  HIP_TRY(c, sd_ws_release(c, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  *out_found = found;
  return SD_CAS_OK;
}

int sd_cas_duplicate_report(sd_cas_ctx* c, const uint64_t* h_keys, const uint64_t* h_sizes,
                            const uint8_t* h_state, size_t n, uint32_t* h_rep, uint32_t* h_copies,
                            uint64_t out_totals[8], size_t k, uint32_t* h_top_heads,
                            uint64_t* h_top_waste, uint64_t* out_found) {
  if (!c) return SD_CAS_EINVAL;
  const bool want_top = h_top_heads && h_top_waste;
  if (n >= (1ull << 32) || (n && (!h_keys || !h_sizes)) || (!h_top_heads != !h_top_waste) ||
      (want_top && !out_found))
    return fail(c, SD_CAS_EINVAL, "duplicate_report: bad arguments");
  if (want_top && k > SD_CAS_TOP_MAX)
    return fail(c, SD_CAS_EINVAL, "duplicate_report: k = %zu exceeds SD_CAS_TOP_MAX", k);
  if (out_found) *out_found = 0;
  if (out_totals)
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++) out_totals[j] = 0;
  if (n == 0) {
    if (want_top)
      for (size_t j = 0; j < k; j++) { h_top_heads[j] = SD_CAS_NO_OBJECT; h_top_waste[j] = 0; }
    return SD_CAS_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t kk = want_top ? k : 0;
  int rc = ensure(c, c->io, sd_dup_report_layout(nullptr, n, h_state != nullptr, kk).bytes);
  if (rc) return rc;
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
  uint64_t totals[SD_CAS_STAT_COUNT];
  if ((rc = object_stats_impl(c, L.rep, L.sizes, L.state, n, L.copies, nullptr, totals, s))) return rc;
  if (out_totals)
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++) out_totals[j] = totals[j];
  if (want_top) {
    if ((rc = sd_cas_top_duplicates_dev(c, L.rep, L.sizes, L.copies, n, k, L.top_heads, L.top_waste, out_found, s)))
      return rc;
    if (k) {
      HIP_TRY(c, hipMemcpyAsync(h_top_heads, L.top_heads, k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipMemcpyAsync(h_top_waste, L.top_waste, k * 8, hipMemcpyDeviceToHost, s));
    }
  }
  if (h_rep) HIP_TRY(c, hipMemcpyAsync(h_rep, L.rep, n * 4, hipMemcpyDeviceToHost, s));
  if (h_copies) HIP_TRY(c, hipMemcpyAsync(h_copies, L.copies, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
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
  if (n == 0) {  // no Objects: the context's count is 0 (a memset, no launch)
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, hipMemsetAsync(c->d_scalar, 0, 8, s));
    HIP_TRY(c, sd_ws_release(c, s));
    c->region_obj_set = -1;
    if (out_objects) *out_objects = 0;
    return SD_CAS_OK;
  }
  int rc = ensure(c, c->exact, sd_exact_layout(nullptr, n).bytes);
  if (rc) return rc;
  const ExactWs L = sd_exact_layout(c->exact.p, n);
  HIP_TRY(c, sd_ws_acquire(c, s));  // c->exact is ordered with ws: the inner groupings use both
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
  HIP_TRY(c, sd_ws_release(c, s));
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
extern "C" void sd_content_tasks_constants(uint64_t out[4]) {
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
  if (n == 0) {  // no Objects: the context's count is 0 (a memset, no launch)
    HIP_TRY(c, sd_ws_acquire(c, s));
    HIP_TRY(c, hipMemsetAsync(c->d_scalar, 0, 8, s));
    HIP_TRY(c, sd_ws_release(c, s));
    c->region_obj_set = -1;
    if (out_objects) *out_objects = 0;
    return SD_CAS_OK;
  }
  int rc = ensure(c, c->contents, sd_content_compare_layout(nullptr, n).bytes);
  if (rc) return rc;
  const ContentCompareWs L = sd_content_compare_layout(c->contents.p, n);
  const uint8_t* arena = (const uint8_t*)d_arena;
  HIP_TRY(c, sd_ws_acquire(c, s));  // c->contents is ordered with ws: the inner calls use both
  // the bounds verdict first: a batch that breaks them is not read and writes nothing
  uint32_t bad = 0;
  HIP_TRY(c, ct_check_bounds(arena_bytes, d_offs, d_lens, n, L.counters, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, L.counters + CT_BAD, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad) {
    (void)sd_ws_release(c, s);
    return fail(c, SD_CAS_EINVAL, "group_exact_contents: %s",
                (bad & 1) ? "a content is longer than 64 GiB" : "a content is misaligned or extends past arena_bytes");
  }
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
  HIP_TRY(c, sd_ws_release(c, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  c->region_obj_set = -1;
  if (out_objects) *out_objects = objects;
  return SD_CAS_OK;
}

int sd_cas_duplicate_report_exact(sd_cas_ctx* c, const uint64_t* h_keys, const uint64_t* h_sizes,
                                  const char* h_hex, const uint8_t* h_state, size_t n, uint32_t* h_rep,
                                  uint32_t* h_rep_exact, uint32_t* h_copies_exact, uint64_t out_totals[8],
                                  uint64_t out_totals_exact[8], uint64_t* out_unconfirmed, size_t k,
                                  uint32_t* h_top_heads, uint64_t* h_top_waste, uint64_t* out_found) {
  if (!c) return SD_CAS_EINVAL;
  const bool want_top = h_top_heads && h_top_waste;
  if (n >= (1ull << 32) || (n && (!h_keys || !h_sizes || !h_hex)) || (!h_top_heads != !h_top_waste) ||
      (want_top && !out_found))
    return fail(c, SD_CAS_EINVAL, "duplicate_report_exact: bad arguments");
  if (want_top && k > SD_CAS_TOP_MAX)
    return fail(c, SD_CAS_EINVAL, "duplicate_report_exact: k = %zu exceeds SD_CAS_TOP_MAX", k);
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
  int rc;
  if (h_rep || out_totals)
    if ((rc = sd_cas_duplicate_report(c, h_keys, h_sizes, h_state, n, h_rep, nullptr, out_totals, 0,
                                      nullptr, nullptr, nullptr)))
      return rc;
  if (out_found) *out_found = 0;
  if (out_unconfirmed) *out_unconfirmed = unconfirmed;
  if (out_totals_exact)
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++) out_totals_exact[j] = 0;
  if (n == 0) {
    if (want_top)
      for (size_t j = 0; j < k; j++) { h_top_heads[j] = SD_CAS_NO_OBJECT; h_top_waste[j] = 0; }
    return SD_CAS_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t kk = want_top ? k : 0;
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
  uint64_t totals[SD_CAS_STAT_COUNT];
  if ((rc = object_stats_impl(c, L.rep, L.sizes, L.state, n, L.copies, nullptr, totals, s))) return rc;
  if (out_totals_exact)
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++) out_totals_exact[j] = totals[j];
  if (want_top) {
    if ((rc = sd_cas_top_duplicates_dev(c, L.rep, L.sizes, L.copies, n, k, L.top_heads, L.top_waste, out_found, s)))
      return rc;
    if (k) {
      HIP_TRY(c, hipMemcpyAsync(h_top_heads, L.top_heads, k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipMemcpyAsync(h_top_waste, L.top_waste, k * 8, hipMemcpyDeviceToHost, s));
    }
  }
  if (h_rep_exact) HIP_TRY(c, hipMemcpyAsync(h_rep_exact, L.rep, n * 4, hipMemcpyDeviceToHost, s));
  if (h_copies_exact) HIP_TRY(c, hipMemcpyAsync(h_copies_exact, L.copies, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

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
