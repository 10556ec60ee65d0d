// object_index.hip — the library-resident Object index on gfx950: the library's (cas_id -> Object)
// relation kept in HBM between calls, so that a job step finds the Objects of its cas_ids
// (find_many by cas_id, file_identifier/mod.rs:181-188; the watcher's find_first,
// location/manager/watcher/utils.rs:249-257) without the caller handing every existing Object in
// again.
//
// A power-of-two table of 16-B slots {u64 key, u32 id, u32 pad}, linear probing from
// home(key) = mix64(key) >> (64 - log2 slots), one lane per key.  Two key-word values mean EMPTY
// and TOMBSTONE; the two real keys of those values have a side id each in the counter block.
//   insert  claims the first EMPTY slot of the probe sequence with a 64-bit CAS on the key word
//           (its return value is the probe's read), then atomicMin on the id word.  A cleared
//           slot's id is 0xFFFFFFFF, so claim and minimum need no order between them.  A
//           tombstone is never reused: a key has at most one slot, and a probe may stop at the
//           first match or EMPTY.
//   erase   CAS key -> TOMBSTONE.
//   rehash  every live slot into a fresh table (grown, or the same size to drop tombstones).
// The L2s of the eight XCDs are not coherent for plain accesses, so in the kernels that write a
// table (insert, erase, rehash's destination) every slot access is a device-scope atomic; plain
// 16-B slot loads appear only where the table was written by EARLIER kernels (lookup, export,
// rehash's source).  The library orders the calls on one index (object_index_host.cpp).
// Counters are summed per wave (ballots) before the one global atomic, the longest probe is one
// atomicMax per wave.  Integer work bound by random 16-B reads: nothing here is a GEMM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_debug.h"
#include "sd_mix.h"
#include "sd_object_index.h"

namespace sdcas {

typedef unsigned long long ull;
constexpr int INDEX_THREADS = 256;

__device__ __forceinline__ uint64_t index_home(uint64_t key, uint32_t log2_slots) {
  return mix64(key) >> (64u - log2_slots);
}
__device__ __forceinline__ uint32_t* index_side(const IndexTable& t, uint64_t key) {
  return (uint32_t*)(t.ctr + INDEX_CTR_SIDE) + (key == INDEX_EMPTY ? 0 : 1);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
// one atomicMax per wave: op << 32 | the wave's longest probe
__device__ __forceinline__ void note_probe(const IndexTable& t, uint32_t probes, uint32_t op) {
  const uint32_t m = wave_max(probes);
  if ((threadIdx.x & 63u) == 0 && m) atomicMax((ull*)(t.ctr + INDEX_CTR_PROBE), ((ull)op << 32) | m);
}
__device__ __forceinline__ void note_full(const IndexTable& t, uint64_t key) {
  SD_DBG_CHECK(false, "object index: key %llx probed all %llu slots", (ull)key, 1ull << t.log2_slots);
  atomicMax((ull*)(t.ctr + INDEX_CTR_FULL), 1ull);
}

// Claim or find key's slot and lower its id.  Returns true when the slot was claimed (a new key).
__device__ __forceinline__ bool index_put(const IndexTable& t, uint64_t key, uint32_t id, uint32_t* probes) {
  const uint64_t mask = (1ull << t.log2_slots) - 1ull;
  uint64_t slot = index_home(key, t.log2_slots);
  for (uint64_t p = 0; p <= mask; ++p) {
    *probes = (uint32_t)min(p + 1, (uint64_t)0xFFFFFFFFu);
    const uint64_t prev = atomicCAS((ull*)&t.slots[slot].key, (ull)INDEX_EMPTY, (ull)key);
    if (prev == INDEX_EMPTY || prev == key) {
      atomicMin(&t.slots[slot].id, id);
      return prev == INDEX_EMPTY;
    }
    slot = (slot + 1) & mask;
  }
  note_full(t, key);
  return false;
}

extern "C" __global__ void __launch_bounds__(INDEX_THREADS)
sd_index_insert(IndexTable t, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ids,
                uint64_t n, uint32_t op) {
  const uint64_t i = (uint64_t)blockIdx.x * INDEX_THREADS + threadIdx.x;
  bool claimed = false;
  uint32_t probes = 0;
  if (i < n) {
    const uint64_t key = keys[i];
    const uint32_t id = ids[i];
    if (key >= INDEX_TOMB) claimed = atomicMin(index_side(t, key), id) == INDEX_NO_ID;
    else claimed = index_put(t, key, id, &probes);
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(claimed));
  if ((threadIdx.x & 63u) == 0 && c) atomicAdd((ull*)(t.ctr + INDEX_CTR_ENTRIES), (ull)c);
  note_probe(t, probes, op);
}

extern "C" __global__ void __launch_bounds__(INDEX_THREADS)
sd_index_erase(IndexTable t, const uint64_t* __restrict__ keys, uint64_t n, uint32_t op) {
  const uint64_t i = (uint64_t)blockIdx.x * INDEX_THREADS + threadIdx.x;
  const uint64_t mask = (1ull << t.log2_slots) - 1ull;
  bool buried = false, side_gone = false;
  uint32_t probes = 0;
  if (i < n) {
    const uint64_t key = keys[i];
    if (key >= INDEX_TOMB) {
      side_gone = atomicExch(index_side(t, key), INDEX_NO_ID) != INDEX_NO_ID;
    } else {
      uint64_t slot = index_home(key, t.log2_slots);
      for (uint64_t p = 0; p <= mask; ++p) {
        probes = (uint32_t)min(p + 1, (uint64_t)0xFFFFFFFFu);
        const uint64_t cur = __hip_atomic_load((ull*)&t.slots[slot].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) {  // a repeat of the key in this batch may bury it first: one of them counts
          buried = atomicCAS((ull*)&t.slots[slot].key, (ull)key, (ull)INDEX_TOMB) == key;
          break;
        }
        if (cur == INDEX_EMPTY) break;
        slot = (slot + 1) & mask;
      }
    }
  }
  const uint32_t b = (uint32_t)__popcll(__ballot(buried)), g = (uint32_t)__popcll(__ballot(side_gone));
  if ((threadIdx.x & 63u) == 0) {
    if (b + g) atomicAdd((ull*)(t.ctr + INDEX_CTR_ENTRIES), (ull)0 - (ull)(b + g));
    if (b) atomicAdd((ull*)(t.ctr + INDEX_CTR_TOMBS), (ull)b);
  }
  note_probe(t, probes, op);
}

// The table is read-only here and was written by earlier kernels: one plain 16-B load per probe.
template <bool MIN_INTO>
__global__ void __launch_bounds__(INDEX_THREADS)
sd_index_lookup(IndexTable t, const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ out,
                uint32_t op) {
  const uint64_t i = (uint64_t)blockIdx.x * INDEX_THREADS + threadIdx.x;
  const uint64_t mask = (1ull << t.log2_slots) - 1ull;
  uint32_t probes = 0;
  if (i < n) {
    const uint64_t key = keys[i];
    uint32_t id = INDEX_NO_ID;
    if (key >= INDEX_TOMB) {
      id = *index_side(t, key);
    } else {
      uint64_t slot = index_home(key, t.log2_slots);
      for (uint64_t p = 0; p <= mask; ++p) {
        probes = (uint32_t)min(p + 1, (uint64_t)0xFFFFFFFFu);
        const ulonglong2 v = *(const ulonglong2*)&t.slots[slot];
        if (v.x == key) { id = (uint32_t)v.y; break; }
        if (v.x == INDEX_EMPTY) break;
        slot = (slot + 1) & mask;
      }
    }
    out[i] = MIN_INTO ? min(out[i], id) : id;
  }
  note_probe(t, probes, op);
}

extern "C" __global__ void __launch_bounds__(INDEX_THREADS)
sd_index_rehash(IndexTable from, IndexTable to) {
  const uint64_t i = (uint64_t)blockIdx.x * INDEX_THREADS + threadIdx.x;
  if (i >> from.log2_slots) return;
  const ulonglong2 v = *(const ulonglong2*)&from.slots[i];
  uint32_t probes = 0;
  if (v.x < INDEX_TOMB) (void)index_put(to, v.x, (uint32_t)v.y, &probes);
}

extern "C" __global__ void __launch_bounds__(INDEX_THREADS)
sd_index_export(IndexTable t, uint64_t* __restrict__ keys, uint32_t* __restrict__ ids, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * INDEX_THREADS + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  ull* cursor = (ull*)(t.ctr + INDEX_CTR_EXPORT);
  ulonglong2 v = make_ulonglong2(INDEX_EMPTY, 0);
  if (!(i >> t.log2_slots)) v = *(const ulonglong2*)&t.slots[i];
  const bool live = v.x < INDEX_TOMB;
  const uint64_t m = __ballot(live);
  uint32_t lo = 0, hi = 0;
  if (lane == 0 && m) {
    const ull base = atomicAdd(cursor, (ull)__popcll(m));
    lo = (uint32_t)base;  hi = (uint32_t)(base >> 32);
  }
  const uint64_t base = ((uint64_t)(uint32_t)__shfl((int)hi, 0) << 32) | (uint32_t)__shfl((int)lo, 0);
  if (live) {
    const uint64_t d = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (d < cap) { keys[d] = v.x;  ids[d] = (uint32_t)v.y; }
  }
  if (i == 0) {  // the two keys that live beside the table
    for (int k = 0; k < 2; ++k) {
      const uint32_t id = ((const uint32_t*)(t.ctr + INDEX_CTR_SIDE))[k];
      if (id == INDEX_NO_ID) continue;
      const uint64_t d = atomicAdd(cursor, 1ull);
      if (d < cap) { keys[d] = k == 0 ? INDEX_EMPTY : INDEX_TOMB;  ids[d] = id; }
    }
  }
}

static uint32_t index_grid(uint64_t n) { return (uint32_t)((n + INDEX_THREADS - 1) / INDEX_THREADS); }

hipError_t index_insert(IndexTable t, const uint64_t* keys, const uint32_t* ids, uint64_t n, uint32_t op,
                        hipStream_t s) {
  if (n == 0) return hipSuccess;
  sd_index_insert<<<index_grid(n), INDEX_THREADS, 0, s>>>(t, keys, ids, n, op);
  return hipGetLastError();
}

hipError_t index_lookup(IndexTable t, const uint64_t* keys, uint64_t n, uint32_t* out, bool min_into,
                        uint32_t op, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (min_into) sd_index_lookup<true><<<index_grid(n), INDEX_THREADS, 0, s>>>(t, keys, n, out, op);
  else sd_index_lookup<false><<<index_grid(n), INDEX_THREADS, 0, s>>>(t, keys, n, out, op);
  return hipGetLastError();
}

hipError_t index_erase(IndexTable t, const uint64_t* keys, uint64_t n, uint32_t op, hipStream_t s) {
  if (n == 0) return hipSuccess;
  sd_index_erase<<<index_grid(n), INDEX_THREADS, 0, s>>>(t, keys, n, op);
  return hipGetLastError();
}

hipError_t index_rehash(IndexTable from, IndexTable to, hipStream_t s) {
  sd_index_rehash<<<index_grid(1ull << from.log2_slots), INDEX_THREADS, 0, s>>>(from, to);
  return hipGetLastError();
}

hipError_t index_export(IndexTable t, uint64_t* keys, uint32_t* ids, uint64_t cap, hipStream_t s) {
  sd_index_export<<<index_grid(1ull << t.log2_slots), INDEX_THREADS, 0, s>>>(t, keys, ids, cap);
  return hipGetLastError();
}

SD_DBG_ACCESSOR(sd_dbg_violations_object_index)

}  // namespace sdcas
