// dup_verify.hip — K1V: the fused chain's sampled hashing with duplicate contents verified by
// comparison instead of hashed (K1G: cas_hash.hip; the lane program and the region epilogue they
// share: cas_sampled.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cas_sampled.hpp"
#include "dup_slice.hpp"
#include "sd_debug.h"
#include "sd_dup_probe.h"
#include "sd_dup_runs.h"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_ws.h"

namespace sdcas {

// ---- K1V: K1G with duplicate contents verified by comparison, not hashed -----------------
// Two files of equal size and equal 57,344 content bytes have the same message, so the same
// key: the second one's 953 compressions buy nothing.  Proving the bytes equal costs one more
// read of the copy's row, one read of the original's row per run of its copies, and ~40 VALU
// instructions per 128-B line against 1,360 to hash it.
//   1. sd_dup_probe_kernel: a 64-bit probe per file (sd_dup_probe.h: size, first and last 32 B);
//      the hash grouping gives cand[f] = the smallest file with f's probe.  cand[f] == f: hash
//      f.  Otherwise f is a candidate duplicate of cand[f] (which is hashed: cand[cand[f]] ==
//      cand[f]).
//   2. sd_dup_compact_kernel: list H (to hash), and each candidate's rank among the candidates
//      of its original (cnt[cand[f]]++); exclusive_scan_u32 of cnt gives every original's first
//      slot and sd_dup_order_kernel writes list C, the candidates ordered by original.  The
//      order inside a group is the atomics' (no result depends on it); the counts stay on the
//      device.
//   3. sd_cas_dup_mixed_kernel, K1G's grid + 1 workgroup: hash tiles run K1G's lane program and
//      epilogue on H[tile * B + lane]; compare tiles take a wave per task, a window of
//      DUP_RUN_K entries of list C (sd_dup_runs.h), read the original once per run of its
//      copies and write same[f].  Compare tiles lie among the hash tiles, so their loads run
//      beside the hash waves' VALU work, and at the grid's end, where they fill the last hash
//      round's drain.  Which workgroup does what is either fixed before launch (dup_tile_of) or,
//      for large grids, taken at run time by each workgroup as it starts: at most one compare
//      workgroup of one wave per SIMD on a CU, the others hashing (sd_dup_runs.h).
//   4. sd_cas_dup_finish_kernel over C: a verified file takes keys[cand[f]]; an unverified one
//      (a probe collision) is hashed here, under a wave-level branch; every C file then gets
//      rep[f] = f and its region row through the same epilogue.
// The bucket tables after it see the same rows as after K1G, in another order.
struct DupLists {
  const uint32_t* cand;  // [n] smallest file with the same probe
  uint32_t* list_h;      // [n] files to hash (counters[0] of them)
  uint32_t* list_c;      // [n] candidates (counters[1]), the copies of one original consecutive
  uint32_t* same;        // [n] same[f] = 1: f's size and bytes equal cand[f]'s (C files only)
  uint32_t* cnt;         // [n] cnt[g] = candidates of original g (zeroed by the probe kernel)
  uint32_t* first;       // [n] first[g] = list C slot of g's first candidate (cnt's scan)
  uint32_t* rank;        // [n] rank[f] = f's place among cand[f]'s candidates (C files only)
  uint32_t* counters;    // DUP_COUNTERS words (named in sd_kernels.h)
  uint32_t* cu;          // DUP_CU_SLOTS words: compare workgroups resident per CU (run-time roles)
  uint32_t tail_tiles;   // compare tiles at the grid's end (the mixed kernel), >= 1; 0: roles are
                         // taken at run time (sd_dup_runs.h)
  uint32_t slots;        // workgroups of the main kernel that the chip holds at once
  // the host's view of this call, in pinned host memory: {seq, candidates, files}, seq stored last
  volatile uint32_t* note;
  uint32_t seq, files;
};

extern "C" __global__ void __launch_bounds__(256)
sd_dup_probe_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                    const uint64_t* __restrict__ sizes, uint64_t n, uint64_t* __restrict__ probes,
                    uint32_t* __restrict__ counters, uint32_t* __restrict__ cu,
                    uint32_t* __restrict__ cnt) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < DUP_COUNTERS) counters[threadIdx.x] = 0;
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < DUP_CU_SLOTS; i += 256) cu[i] = 0;
  if (f < n) {
    probes[f] = dup_probe(sizes[f], content + f * stride);
    cnt[f] = 0;
  }
}

// One reservation per workgroup for list H, which keeps the file order inside a workgroup's run.
// wcnt rows: files to hash, candidates, groups (candidates of rank 0).
extern "C" __global__ void __launch_bounds__(256)
sd_dup_compact_kernel(uint64_t n, DupLists dl) {
  __shared__ uint32_t wcnt[3][4], base;
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const bool live = f < n;
  const uint32_t g = live ? dl.cand[f] : 0u;
  const bool h = live && g == (uint32_t)f;
  const bool c = live && !h;
  uint32_t r = 1;
  if (c) {
    r = atomicAdd(&dl.cnt[g], 1u);
    dl.rank[f] = r;
  }
  const uint64_t bh = __ballot(h), bc = __ballot(c), bg = __ballot(r == 0);
  const uint64_t below = (1ull << lane) - 1ull;
  if (lane == 0) {
    wcnt[0][w] = (uint32_t)__popcll(bh);
    wcnt[1][w] = (uint32_t)__popcll(bc);
    wcnt[2][w] = (uint32_t)__popcll(bg);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    constexpr uint32_t word[3] = {DUP_N_HASH, DUP_N_CAND, DUP_GROUPS};
    const uint32_t t = wcnt[threadIdx.x][0] + wcnt[threadIdx.x][1] + wcnt[threadIdx.x][2] +
                       wcnt[threadIdx.x][3];
    const uint32_t b = t ? atomicAdd(&dl.counters[word[threadIdx.x]], t) : 0u;
    if (threadIdx.x == 0) base = b;
  }
  __syncthreads();
  uint32_t oh = base + (uint32_t)__popcll(bh & below);
  for (uint32_t i = 0; i < w; ++i) oh += wcnt[0][i];
  if (h) dl.list_h[oh] = (uint32_t)f;
}

// list C: candidate f goes to its original's first slot + its rank (< counters[DUP_N_CAND])
extern "C" __global__ void __launch_bounds__(256)
sd_dup_order_kernel(uint64_t n, DupLists dl) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const uint32_t g = dl.cand[f];
  if (g != (uint32_t)f) dl.list_c[dl.first[g] + dl.rank[f]] = (uint32_t)f;
}

// One wave runs task t: entries [first, first + m) of list C, entry e in lane e.  Sizes are
// compared once per entry; then, slice by slice (sd_dup_runs.h: 8 KiB, 8 quads per lane), the
// wave holds the current original's slice in registers and streams the slices of the entries
// still alive against it, the next entry's loads issued before the current one is compared.
// The reference is loaded again only where cand changes among the alive entries, and a refuted
// entry is not read again.  Returns the task's runs (reference rows); writes same[f].  Nothing
// is read past a row's 57,344th byte: the largest offset is dup_slice_quad_offset(6, 7, 63) + 16.
// A lane is known by its byte offset in a 1-KiB load (voff = 16 lane) alone, and the lane number
// is derived from it afresh where a task needs it (dup_lane_of: opaque to the optimizer, which
// would otherwise keep both in registers over the loop and take the kernel past K1G's 101 VGPRs).
// (DupSlice, dup_slices_differ and dup_first_bit: dup_slice.hpp)
// row is wave-uniform.  The loads go through a buffer descriptor of the row's 57,344 bytes: a
// lane's address is its one 32-bit offset, each quad's offset in the row is scalar, and the
// hardware bounds every load to the row.
typedef uint32_t dup_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dup_load_slice(DupSlice& d, const uint8_t* __restrict__ content,
                                               uint64_t stride, uint32_t file, uint32_t s, uint32_t voff) {
  const uint64_t a = (uint64_t)content + (uint64_t)file * stride;
  const uint64_t row = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, (int)DUP_ROW_BYTES, 0x00020000);
#pragma unroll
  for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u) {
    const dup_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff,
                                                              (int)dup_slice_quad_offset(s, u, 0), 0);
    d.q[u] = make_uint4(v.x, v.y, v.z, v.w);
  }
}
__device__ __forceinline__ uint32_t dup_lane_of(uint32_t voff) {
  uint32_t lane;
  asm volatile("v_lshrrev_b32 %0, 4, %1" : "=v"(lane) : "v"(voff));
  return lane;
}

__device__ __forceinline__ uint32_t dup_compare_task(const uint8_t* __restrict__ content, uint64_t stride,
                                                     const uint64_t* __restrict__ sizes,
                                                     const DupLists& dl, uint32_t t, uint32_t n_cand,
                                                     uint32_t voff) {
  uint32_t lane = dup_lane_of(voff);
  const uint32_t first = dup_task_first(t), m = dup_task_entries(t, n_cand);
  uint32_t f = 0, g = 0;
  bool ok = false;
  if (lane < m) {
    f = dl.list_c[first + lane];
    g = dl.cand[f];
    ok = sizes[f] == sizes[g];
  }
  // a run starts at the window's first entry and at an original's first slot of list C
  bool head = lane < m;
  if (head && lane) head = dl.first[g] == first + lane;
  const uint32_t heads = (uint32_t)__ballot(head);  // (uniform) bit e: entry e starts a run
  const uint32_t runs = (uint32_t)__builtin_popcount(heads);
  uint32_t alive = (uint32_t)__ballot(ok);  // entries not refuted yet (uniform; m <= 32)
#pragma unroll 1
  for (uint32_t s = 0; s < DUP_SLICES && alive; ++s) {
    DupSlice ref, cur, nxt;
    uint32_t left = alive;
    uint32_t e = dup_first_bit(left);
    // e's run is the number of heads up to e; its original is read from cand[] where the run
    // changes, so the lanes keep their entry's file and not its original over the loop
    uint32_t fe = (uint32_t)__builtin_amdgcn_readlane((int)f, (int)e);
    uint32_t loaded = (uint32_t)__builtin_popcount(heads & ((2u << e) - 1u));
    dup_load_slice(ref, content, stride, (uint32_t)__builtin_amdgcn_readfirstlane((int)dl.cand[fe]), s, voff);
    dup_load_slice(cur, content, stride, fe, s, voff);
#pragma unroll 1
    for (;;) {
      left &= left - 1u;
      uint32_t e2 = 0;
      if (left) {  // (uniform) the next alive entry's slice, in flight during this compare
        e2 = dup_first_bit(left);
        fe = (uint32_t)__builtin_amdgcn_readlane((int)f, (int)e2);
        dup_load_slice(nxt, content, stride, fe, s, voff);
      }
      if (dup_slices_differ(ref, cur)) alive &= ~(1u << e);
      if (!left) break;
      e = e2;
      cur = nxt;
      const uint32_t run = (uint32_t)__builtin_popcount(heads & ((2u << e) - 1u));
      if (run != loaded) {  // (uniform) the window's next original
        loaded = run;
        dup_load_slice(ref, content, stride, (uint32_t)__builtin_amdgcn_readfirstlane((int)dl.cand[fe]), s, voff);
      }
    }
  }
  lane = dup_lane_of(voff);
  if (lane < m) dl.same[f] = (alive >> lane) & 1u;
  return runs;
}

// The CU this wave runs on, as a slot of DupLists::cu.
__device__ __forceinline__ uint32_t dup_this_cu_slot() {
  constexpr int HW_REG_HW_ID = 4, HW_REG_XCC_ID = 20, WHOLE = 31 << 11;  // simm16: id | offset << 6 | (size - 1) << 11
  return dup_cu_slot(__builtin_amdgcn_s_getreg(HW_REG_XCC_ID | WHOLE),
                     __builtin_amdgcn_s_getreg(HW_REG_HW_ID | WHOLE));
}

template <int B>
__device__ __forceinline__ void dup_mixed_kernel_body(const uint8_t* __restrict__ content,
                                                      uint64_t stride,
                                                      const uint64_t* __restrict__ sizes,
                                                      uint64_t* __restrict__ keys, RegionOut ro,
                                                      DupLists dl) {
  __shared__ uint32_t stack_lds[SAMPLED_DEPTH][8][B];
  const uint32_t n_hash = dl.counters[DUP_N_HASH], n_cand = dl.counters[DUP_N_CAND];
  // the grid is n / B + 1 workgroups: TH hash tiles, and at least one compare tile
  const uint32_t G = gridDim.x;
  const uint32_t TH = (n_hash + B - 1) / B;
  // The last tail_tiles workgroups of the grid are compare tiles that run until the task queue
  // is empty: they start as the last round of hash tiles drains and fill the slots it frees
  // (a hash tile is one indivisible ~4 ms; a task is a few hundred us at most).  The other
  // compare tiles lie evenly among the hash tiles and take one tile's worth of entries each (a
  // lane's worth per lane: dup_tile_wave_tasks), so compare loads run beside the hashing from
  // the start (dup_tile_of, sd_dup_runs.h).
  DupTile tile;
  uint32_t quota = dup_tile_wave_tasks();
  bool leaves_cu = false;  // (uniform) a compare workgroup that is counted in its CU's slot
  const bool roles = B == (int)DUP_ROLE_BLOCK && dl.tail_tiles == 0;  // (uniform)
  if (roles) {
    // Roles taken at run time (sd_dup_runs.h): lane 0 decides, and the workgroup reads the role
    // from a stack word that is dead until the hashing starts (hence the second barrier).
    const uint32_t n_tasks = dup_task_count(n_cand);
    if (threadIdx.x == 0) {
      uint32_t role = DUP_ROLE_COMPARE;
      bool compare = dup_wants_compare(
          __hip_atomic_load(&dl.counters[DUP_QUEUE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), n_tasks,
          __hip_atomic_load(&dl.counters[DUP_HASH_QUEUE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), TH);
      if (compare) {
        const uint32_t slot = dup_this_cu_slot();
        compare = dup_cu_has_room(atomicAdd(&dl.cu[slot], 1u)) &&
                  atomicAdd(&dl.counters[DUP_COMPARE_WGS], 1u) < dup_compare_budget(G, TH);
        if (!compare) atomicSub(&dl.cu[slot], 1u);
        stack_lds[0][0][1] = slot;  // a compare workgroup never touches the stack: kept for its exit
      }
      if (!compare) {
        role = atomicAdd(&dl.counters[DUP_HASH_QUEUE], 1u);
        if (role >= TH) role = DUP_ROLE_DRAIN;  // no hash tile left: the drain fills itself
      }
      stack_lds[0][0][0] = role;
    }
    __syncthreads();
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)stack_lds[0][0][0]);
    __syncthreads();
    // (a compare workgroup of a grid that is resident all at once has no quota: sd_dup_runs.h)
    tile = DupTile{role >= DUP_ROLE_COMPARE, role == DUP_ROLE_DRAIN || !dup_compare_has_quota(G, dl.slots), role};
    quota = dup_role_wave_tasks();
    leaves_cu = role == DUP_ROLE_COMPARE;
  } else {
    tile = dup_tile_of(blockIdx.x, G, TH, dl.tail_tiles);
  }
#if SD_DBG
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) dl.counters[DUP_TILES_WANT] = TH;
    if (!tile.compare) atomicAdd(&dl.counters[DUP_TILES_RUN], 1u);
  }
#endif
  if (blockIdx.x == 0 && threadIdx.x < 2) ro.objects[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && dl.note) {
    dl.note[1] = n_cand;
    dl.note[2] = dl.files;
    __threadfence_system();
    dl.note[0] = dl.seq;
  }
  if (!tile.compare) {  // a hash tile: K1G's lane program on list H
    const uint32_t i = tile.hash_tile * B + threadIdx.x;
    const bool live = i < n_hash;
    uint64_t f = 0, key = 0;
    if (live) {
      f = dl.list_h[i];
      LdsStack<B> stk{stack_lds, threadIdx.x};
      const uint4* q = reinterpret_cast<const uint4*>(content + f * stride);
      key = cas_lane_sampled<B>(q, sizes[f], stk);
    }
    region_epilogue<B>(stack_lds, live, f, key, keys, ro);
  } else {  // compare tile: a wave per task, handed out from one queue over list C's windows
    const uint32_t voff = dup_slice_quad_offset(0, 0, threadIdx.x & 63u);
    const uint32_t n_tasks = dup_task_count(n_cand);
    uint32_t done = 0, refs = 0;
    for (uint32_t k = 0; tile.tail || k < quota; ++k) {
      uint32_t t = 0;
      if (voff == 0) t = atomicAdd(&dl.counters[DUP_QUEUE], 1u);
      t = __builtin_amdgcn_readfirstlane(t);
      if (t >= n_tasks) break;
      refs += dup_compare_task(content, stride, sizes, dl, t, n_cand, voff);
      ++done;
    }
    if (voff == 0 && done) {
      atomicAdd(&dl.counters[DUP_TASKS], done);
      atomicAdd(&dl.counters[DUP_REFS], refs);
    }
    if (leaves_cu) {  // its CU may hold another compare workgroup
      __syncthreads();
      if (threadIdx.x == 0) atomicSub(&dl.cu[stack_lds[0][0][1]], 1u);
    }
  }
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK)
sd_cas_dup_mixed_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                        const uint64_t* __restrict__ sizes, uint64_t* __restrict__ keys,
                        RegionOut ro, DupLists dl) {
  dup_mixed_kernel_body<SAMPLED_BLOCK>(content, stride, sizes, keys, ro, dl);
}

extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK_NARROW)
sd_cas_dup_mixed_kernel_256(const uint8_t* __restrict__ content, uint64_t stride,
                            const uint64_t* __restrict__ sizes, uint64_t* __restrict__ keys,
                            RegionOut ro, DupLists dl) {
  dup_mixed_kernel_body<SAMPLED_BLOCK_NARROW>(content, stride, sizes, keys, ro, dl);
}

// The grid covers n files; the workgroups past list C's end leave at once.
extern "C" __global__ void __launch_bounds__(SAMPLED_BLOCK_NARROW)
sd_cas_dup_finish_kernel(const uint8_t* __restrict__ content, uint64_t stride,
                         const uint64_t* __restrict__ sizes, uint64_t* __restrict__ keys,
                         RegionOut ro, DupLists dl) {
  constexpr int B = SAMPLED_BLOCK_NARROW;
  __shared__ uint32_t stack_lds[SAMPLED_DEPTH][8][B];
  const uint32_t n_cand = dl.counters[DUP_N_CAND];
#if SD_DBG
  // conservation of the main kernel's work, whichever way its workgroups got their roles
  if (blockIdx.x == 0) {
    SD_DBG_CHECK(threadIdx.x != 0 || dl.counters[DUP_TILES_RUN] == dl.counters[DUP_TILES_WANT],
                 "dup roles: %u hash tiles run of %u", dl.counters[DUP_TILES_RUN], dl.counters[DUP_TILES_WANT]);
    SD_DBG_CHECK(threadIdx.x != 0 || dl.counters[DUP_TASKS] == dup_task_count(n_cand),
                 "dup roles: %u tasks run of %u", dl.counters[DUP_TASKS], dup_task_count(n_cand));
    for (uint32_t i = threadIdx.x; i < DUP_CU_SLOTS; i += B)
      SD_DBG_CHECK(dl.cu[i] == 0, "dup roles: CU slot %u left at %u", i, dl.cu[i]);
  }
#endif
  if (blockIdx.x * B >= n_cand) return;  // (uniform)
  const uint32_t i = blockIdx.x * B + threadIdx.x;
  const bool live = i < n_cand;
  uint64_t f = 0, key = 0;
  bool ok = false;
  if (live) {
    f = dl.list_c[i];
    ok = dl.same[f] != 0;
    if (ok) key = keys[dl.cand[f]];  // written by the mixed kernel's hash tiles
  }
  const uint64_t verified = __ballot(ok), failed = __ballot(live && !ok);
  if ((threadIdx.x & 63u) == 0) {
    if (verified) atomicAdd(&dl.counters[DUP_VERIFIED], (uint32_t)__popcll(verified));
    if (failed) atomicAdd(&dl.counters[DUP_REHASHED], (uint32_t)__popcll(failed));
  }
  if (failed) {  // (wave-uniform) a probe collision in this wave: those lanes hash their file
    if (live && !ok) {
      LdsStack<B> stk{stack_lds, threadIdx.x};
      const uint4* q = reinterpret_cast<const uint4*>(content + f * stride);
      key = cas_lane_sampled<B>(q, sizes[f], stk);
    }
  }
  region_epilogue<B>(stack_lds, live, f, key, keys, ro);
}

SD_DBG_ACCESSOR(sd_dbg_violations_dup_verify)

// ---- host launchers ----------------------------------------------------------------
DupVerifyWs dup_verify_layout(void* ws, uint64_t n) {
  WsCarve w(ws);  DupVerifyWs L;
  L.probes = w.take<uint64_t>(n);  L.cand = w.take<uint32_t>(n);
  L.list_h = w.take<uint32_t>(n);  L.list_c = w.take<uint32_t>(n);  L.same = w.take<uint32_t>(n);
  L.cnt = w.take<uint32_t>(n);  L.first = w.take<uint32_t>(n);  L.rank = w.take<uint32_t>(n);
  L.partial = w.take<uint32_t>(n / 4096 + 1);  // exclusive_scan_u32's scratch
  L.counters = w.take<uint32_t>(DUP_COUNTERS);  L.cu = w.take<uint32_t>(DUP_CU_SLOTS);
  L.objects = w.take<uint64_t>(1);
  L.bytes = w.bytes();  return L;
}
size_t dup_verify_workspace_bytes(uint64_t n) { return dup_verify_layout(nullptr, n).bytes; }

// tail compare tiles = slots x NUM / DEN (hash_sampled_regions_verify; a build-time knob for the sweep)
#ifndef SD_DUP_TAIL_NUM
#define SD_DUP_TAIL_NUM 5u
#define SD_DUP_TAIL_DEN 7u
#endif

hipError_t dup_candidates(const uint8_t* content, uint64_t stride, const uint64_t* sizes, uint64_t n,
                          const DupVerifyWs& L, void* group_ws, uint32_t* totals, hipStream_t s) {
  if (n == 0) return hipSuccess;
  sd_dup_probe_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(content, stride, sizes, n, L.probes,
                                                                  L.counters, L.cu, L.cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hash_group_min(L.probes, nullptr, n, L.cand, L.objects, group_ws, totals, s);
}

hipError_t hash_sampled_regions_verify(const uint8_t* content, uint64_t stride, const uint64_t* sizes,
                                       uint64_t n, uint64_t* keys, const RegionOut& ro,
                                       const DupVerifyWs& L, uint32_t* note, uint32_t seq,
                                       hipStream_t s, uint32_t cus, bool cu_roles) {
  if (n == 0) return hipSuccess;
  // static placement: the grid choice of hash_sampled.  Run-time roles (sd_dup_runs.h): 256-lane
  // workgroups for every batch shape, so a compare workgroup is one wave on each SIMD of its CU
  const bool narrow = cu_roles || sampled_grid_is_narrow(n, cus);
  // Static placement's tail compare tiles: the last round of hash tiles frees the chip's workgroup
  // slots one by one over a tile's time, half the slots x that time in all, and a compare tile of B pairs
  // took ~0.7 of a hash tile's time beside hash tiles (profiles/dup_verify/): slots / 2 / 0.7.
  // A tile of B entries in runs reads ~0.8 of the rows a tile of B pairs did, which would put
  // the count near 0.9 slots; the sweep on the run kernel (profiles/dup_groups/: 1 / 192 / 365 /
  // 448 / 512 / all 768 tail tiles: 22.55 / 21.3 / 20.9 / 21.15 / 20.75 / 22.55 ms) is flat from
  // 365 to 512 within the process-to-process spread, so 5/7 stays.
  const uint32_t slots = (cus ? cus : 256u) * (narrow ? 4u : 2u);
  const uint32_t tail_tiles = cu_roles ? 0u : slots * SD_DUP_TAIL_NUM / SD_DUP_TAIL_DEN;  // (static: >= 1)
  const DupLists dl{L.cand, L.list_h, L.list_c, L.same, L.cnt, L.first, L.rank, L.counters, L.cu,
                    tail_tiles, slots, note, seq, (uint32_t)n};
  const uint32_t nb256 = (uint32_t)((n + 255) / 256);
  sd_dup_compact_kernel<<<nb256, 256, 0, s>>>(n, dl);
  hipError_t e = exclusive_scan_u32(L.cnt, L.first, n, L.partial, s);
  if (e != hipSuccess) return e;
  sd_dup_order_kernel<<<nb256, 256, 0, s>>>(n, dl);
  if (narrow) {
    static_assert(SAMPLED_BLOCK_NARROW == (int)DUP_ROLE_BLOCK, "dup_role_grid is this grid");
    sd_cas_dup_mixed_kernel_256<<<dup_role_grid(n), SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride, sizes,
                                                                                 keys, ro, dl);
  } else {
    const uint64_t blocks = (n + SAMPLED_BLOCK - 1) / SAMPLED_BLOCK;
    sd_cas_dup_mixed_kernel<<<(uint32_t)blocks + 1, SAMPLED_BLOCK, 0, s>>>(content, stride, sizes, keys,
                                                                          ro, dl);
  }
  const uint64_t fb = (n + SAMPLED_BLOCK_NARROW - 1) / SAMPLED_BLOCK_NARROW;
  sd_cas_dup_finish_kernel<<<(uint32_t)fb, SAMPLED_BLOCK_NARROW, 0, s>>>(content, stride, sizes, keys,
                                                                        ro, dl);
  return hipGetLastError();
}

}  // namespace sdcas
