// sd_kernels.h — internal constants shared by the HIP kernels and the C-ABI layer.
#pragma once
#include <stdint.h>

namespace sdcas {

// core/src/object/cas.rs:10-15
constexpr uint64_t SAMPLE_COUNT = 4;
constexpr uint64_t SAMPLE_SIZE = 1024 * 10;
constexpr uint64_t HEADER_OR_FOOTER_SIZE = 1024 * 8;
constexpr uint64_t MINIMUM_FILE_SIZE = 1024 * 100;
constexpr uint32_t SAMPLED_CONTENT_LEN =
    (uint32_t)(2 * HEADER_OR_FOOTER_SIZE + SAMPLE_COUNT * SAMPLE_SIZE);  // 57,344
// cas.rs:18 const_assert!((HEADER_OR_FOOTER_SIZE * 2 + SAMPLE_COUNT * SAMPLE_SIZE) < MINIMUM_FILE_SIZE)
static_assert(2 * HEADER_OR_FOOTER_SIZE + SAMPLE_COUNT * SAMPLE_SIZE < MINIMUM_FILE_SIZE, "cas.rs:18");
// cas.rs:21 const_assert!(SAMPLE_SIZE > HEADER_OR_FOOTER_SIZE)
static_assert(SAMPLE_SIZE > HEADER_OR_FOOTER_SIZE, "cas.rs:21");

// The packed (whole-file) kernel keeps a 6-deep CV stack: messages of <= 104 chunks
// (a whole file is <= 102,400 + 8 bytes = 101 chunks).
constexpr uint32_t MAX_PACKED_CONTENT_LEN = 104u * 1024u - 8u;

}  // namespace sdcas

#include <hip/hip_runtime.h>
namespace sdcas {
// cus = the device's CU count: batches of fewer 512-lane workgroups than CUs take the
// 256-lane grid (one wave per SIMD instead of half the CUs at two)
hipError_t hash_sampled(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                        uint64_t n, uint64_t* keys, hipStream_t s, uint32_t cus);
// the 512-lane or the 256-lane grid of the sampled kernels for n files (cas_hash.hip)
bool sampled_grid_is_narrow(uint64_t n, uint32_t cus);
// Where K1G and K1V put a batch's rows: the fixed-capacity regions of one region set (sd_group.h).
// A kernel argument: the field order and types are the kernels' ABI.
struct RegionOut {
  uint64_t* rkeys;     // [REGIONS][cap] mixed keys
  uint32_t* rfile;     // [REGIONS][cap] file index
  uint32_t* cursor;    // [REGION_SET_WORDS] rows reserved per region, then the spill count and
                       // the full-region count at REGION_SPILL_WORD; zero on entry (the bucket
                       // tables re-zero them)
  uint64_t cap;
  uint64_t* spill_keys;   // rows past their region's capacity (mixed key, file), unordered
  uint32_t* spill_file;
  uint32_t* rep;       // rep[f] = f: the bucket tables store only where a key's minimum differs
  uint32_t* overflow;  // set when a region is full
  // objects[0]: zeroed here, the bucket tables add the distinct keys; objects[1]: zeroed
  // here, the tables' carve cursor for the global tables of overflowed regions
  unsigned long long* objects;
};

// K1G: K1 + the grouping partition in its epilogue (cas_hash.hip): keys, rep[f] = f, and
// each key's (mix64(key), f) row in the region of its coarse bucket; *overflow |= 1 when a
// region is full; objects[0] = 0 (the bucket tables count).
hipError_t hash_sampled_regions(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                                uint64_t n, uint64_t* keys, const RegionOut& ro, hipStream_t s,
                                uint32_t cus);
// K1V: the same outputs as hash_sampled_regions with duplicate contents verified by comparison
// instead of hashed (dup_verify.hip).  A buffer of the context's own (dup_verify_workspace_bytes(n))
// holds the probes, cand (the smallest file with the same probe), the hash and candidate lists,
// the verified flags, the arrays that order the candidates by original (cnt, first, rank, the
// scan's partial sums), counters[DUP_COUNTERS] (the words named below) and cu[DUP_CU_SLOTS], the
// compare workgroups resident per CU (sd_dup_runs.h), zeroed with the counters.
// dup_candidates fills probes and cand (the hash grouping: group_ws, totals as hash_group_min);
// hash_sampled_regions_verify is the rest of the chain and needs neither.  note (pinned host
// memory, 3 u32, or nullptr): the mixed kernel stores {seq, candidates, n} there, seq last, so
// the host can see without a sync how many candidates an earlier call found.  cu_roles: the main
// kernel's workgroups take their roles at run time (SD_CAS_DUP_PLACEMENT=cu) instead of from the
// static tile map.
constexpr uint32_t DUP_COUNTERS = 16;
// counters: files to hash, candidates, verified, rehashed, the mixed kernel's task queue,
// groups (originals with a candidate), tasks run, reference rows read (one per run of a task);
// run-time roles: the hash-tile queue, compare workgroups started; the debug library's conservation
// check: hash tiles run, and how many the launched grid shape has
constexpr uint32_t DUP_N_HASH = 0, DUP_N_CAND = 1, DUP_VERIFIED = 2, DUP_REHASHED = 3, DUP_QUEUE = 4,
                   DUP_GROUPS = 5, DUP_TASKS = 6, DUP_REFS = 7, DUP_HASH_QUEUE = 8, DUP_COMPARE_WGS = 9,
                   DUP_TILES_RUN = 10, DUP_TILES_WANT = 11;
static_assert(DUP_TILES_RUN < DUP_TILES_WANT && DUP_TILES_WANT < DUP_COUNTERS, "counters");
struct DupVerifyWs {
  uint64_t* probes; uint32_t *cand, *list_h, *list_c, *same, *cnt, *first, *rank, *partial, *counters, *cu;
  uint64_t* objects; size_t bytes;
};
DupVerifyWs dup_verify_layout(void* ws, uint64_t n);  // ws == nullptr: measure only (sd_ws.h)
size_t dup_verify_workspace_bytes(uint64_t n);
hipError_t dup_candidates(const uint8_t* content, uint64_t stride, const uint64_t* sizes, uint64_t n,
                          const DupVerifyWs& L, void* group_ws, uint32_t* totals, hipStream_t s);
hipError_t hash_sampled_regions_verify(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                                       uint64_t n, uint64_t* keys, const RegionOut& ro,
                                       const DupVerifyWs& L, uint32_t* note, uint32_t seq,
                                       hipStream_t s, uint32_t cus, bool cu_roles);
// pinned host -> device copy by a kernel (16-B aligned; else hipMemcpyAsync)
hipError_t pull_host(void* dst, const void* src, uint64_t bytes, hipStream_t s);
hipError_t hash_packed(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                       const uint64_t* sizes, const uint32_t* order, uint64_t n, uint64_t* keys,
                       hipStream_t s);
hipError_t length_keys(const uint32_t* lens, uint64_t n, uint64_t* out, hipStream_t s);
// K1L: a file per `seg`-lane segment (64: one wave per file, lane per chunk; 16: four files
// per wave, 4+ chunks per lane) (offs == nullptr: strided, fixed_len bytes each)
hipError_t hash_chunkpar(const uint8_t* arena, const uint64_t* offs, uint64_t stride,
                         const uint32_t* lens, uint32_t fixed_len, const uint64_t* sizes,
                         uint64_t n, uint64_t* keys, int seg, hipStream_t s,
                         const uint32_t* order = nullptr);
int length_key_bits(uint64_t n);  // significant bits of the length_keys sort key
// cas_ids from whole contents in place (cas_inplace.hip).  classify: the bounds verdict and
// the routing of n contents (arena + offs[i], lens[i] bytes, u64) into ws
// (inplace_workspace_bytes(n)): counters[0] = the checksum chain's bad flags (1: over 64 GiB,
// 4: misaligned or past arena_bytes), counters[1] = sampled files, lens32[i] = lens[i] for a
// whole file (<= 100 KiB) and 0 for a sampled or rejected one, sampled_idx = the sampled
// files.  hash_inplace_sampled = K1P over such a list: keys[idx[k]] for k < n_idx.
struct InplaceWs { uint32_t *counters, *lens32, *sampled_idx; size_t bytes; };
InplaceWs inplace_layout(void* ws, uint64_t n);  // ws == nullptr: measure only (sd_ws.h)
size_t inplace_workspace_bytes(uint64_t n);
hipError_t inplace_classify(uint64_t arena_bytes, const uint64_t* offs, const uint64_t* lens,
                            uint64_t n, void* ws, hipStream_t s);
hipError_t hash_inplace_sampled(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens,
                                const uint32_t* idx, uint64_t n_idx, uint64_t* keys,
                                hipStream_t s);
}  // namespace sdcas
