// content_compare.hip — split a grouping by comparing whole contents where they lie, on gfx950.
//
//   rep_exact[i] = min{ j : class[j] == class[i] && content j == content i },
//   class[i] = (rep[i] as a value, lens[i])
// for ragged contents of an arena (content i = arena + offs[i], lens[i] bytes, the layout of
// sd_cas_checksums_dev).  K1V's compare (dup_verify.hip) at whole-file scale: no digest is taken;
// the members of a class are compared with each other.
//
// Rounds.  Every unresolved row has a pivot, at first its class's first row.  A round compares
// each unresolved row with its pivot; an equal row takes rep_exact = pivot; among the unequal
// rows of one pivot the smallest becomes a head and the pivot of the others (an atomicMin into a
// slot per pivot, then a second pass).  By induction a pivot is the first row of its content.
//
// The compare.  The entry list is sorted by pivot (the library's sort), a task is one 64-KiB piece
// of up to CT_RUN_K consecutive entries (sd_content_tasks.h).  One wave runs a task: entry e in
// lane e; slice by slice it holds the pivot's slice in registers (dup_slice.hpp, shared with K1V)
// and streams the slices of the entries still alive against it, the next entry's loads issued
// before the current compare.  The pivot is read again only where the run changes; an entry once
// refuted is not read again, in this task or in a later piece (its flag, a relaxed read when a
// piece starts).  Waves take tasks from one atomic counter until it is exhausted.  No wave waits
// for another: every loop is bounded by the task count or the piece's length, the flag is only
// ever set during a round, and a stale read of it costs a piece's loads, never correctness.
//
// Loads.  Every wave-load is 64 lanes x 16 B contiguous (global_load_dwordx4), both sides 16-B
// aligned by the layout's rule.  A content is readable to the 16-B round-up of its end and no
// further: a slice's loads are bounded to ct_slice_limit bytes by the lane's own predicate (a
// uniform branch picks the unpredicated loads for a full slice), and in a content's last slice the
// padding bytes of the last quad are masked out (ct_last_quad_mask): they differ between equal
// files.  A content of length 0 has no piece, so nothing of it is read and its offset is never
// formed into an address.  All offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dup_slice.hpp"
#include "sd_content_compare.h"
#include "sd_debug.h"
#include "sd_group.h"

namespace sdcas {

constexpr int CT_THREADS = 256;

extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_check_bounds(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ lens, uint64_t n,
                   uint64_t arena_bytes, uint32_t* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * CT_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = offs[i], len = lens[i];
  const bool ok = (off & 15) == 0 && len <= arena_bytes && off <= arena_bytes - len && len <= CT_MAX_LEN;
  if (!ok) atomicOr(&counters[CT_BAD], len > CT_MAX_LEN ? 1u : 4u);
}

extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_first_entries(const uint32_t* __restrict__ cls, uint64_t n, uint32_t* __restrict__ rep_exact,
                    uint64_t* __restrict__ ekey_in, uint32_t* __restrict__ erow_in,
                    uint32_t* __restrict__ neq) {
  const uint64_t i = (uint64_t)blockIdx.x * CT_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = cls[i];
  const bool head = h == (uint32_t)i;
  if (head) rep_exact[i] = (uint32_t)i;
  ekey_in[i] = head ? n : (uint64_t)h;
  erow_in[i] = (uint32_t)i;
  neq[i] = 0;
}

// a window's pieces (one thread per window); the round's queue, flags and slots made ready
extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_windows(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ erow,
              const uint64_t* __restrict__ lens, uint32_t m, uint32_t* __restrict__ wpieces,
              uint32_t* __restrict__ slot, unsigned long long* __restrict__ tasks) {
  const uint32_t w = blockIdx.x * CT_THREADS + threadIdx.x;
  const uint32_t n_win = ct_window_count(m);
  uint32_t most = 0;
  if (w < n_win) {
    const uint32_t first = ct_window_first(w), k = ct_window_entries(w, m);
    for (uint32_t e = 0; e < k; ++e) {
      const uint32_t p = ct_pieces(lens[erow[first + e]]);
      most = p > most ? p : most;
      slot[(uint32_t)ekey[first + e]] = 0xFFFFFFFFu;  // (every writer stores this value)
    }
    wpieces[w] = most;
  }
  // the exact total, in 64 bits: one atomic per wave
  uint64_t sum = most;
#pragma unroll
  for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(tasks, (unsigned long long)sum);
}

// ---- the compare ---------------------------------------------------------------------------
// a slice's loads from p (wave-uniform, 16-B aligned), bounded to `limit` readable bytes; voff =
// 16 lane
__device__ __forceinline__ void ct_load_slice(DupSlice& d, const uint8_t* __restrict__ p, uint32_t limit,
                                              uint32_t voff) {
  const uint4* __restrict__ q = (const uint4*)(p + voff);
  if (limit == CT_SLICE_BYTES) {  // (uniform)
#pragma unroll
    for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u) d.q[u] = q[u * DUP_WAVE];
  } else {
#pragma unroll
    for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u) {
      d.q[u] = make_uint4(0u, 0u, 0u, 0u);
      if (voff + u * DUP_WAVE * 16u < limit) d.q[u] = q[u * DUP_WAVE];
    }
  }
}
// the compare of a content's last slice: quad `last` holds its last bytes, masked by mask4; the
// quads after it were not loaded (zero on both sides)
__device__ __forceinline__ bool ct_tail_slices_differ(const DupSlice& a, const DupSlice& b, uint32_t last,
                                                      uint4 mask4, uint32_t lane) {
  uint32_t d = 0;
#pragma unroll
  for (uint32_t u = 0; u < DUP_SLICE_QUADS; ++u) {
    const bool is_last = u * DUP_WAVE + lane == last;
    const uint4 m = is_last ? mask4 : make_uint4(~0u, ~0u, ~0u, ~0u);
    d |= ((a.q[u].x ^ b.q[u].x) & m.x) | ((a.q[u].y ^ b.q[u].y) & m.y) | ((a.q[u].z ^ b.q[u].z) & m.z) |
         ((a.q[u].w ^ b.q[u].w) & m.w);
  }
  return __builtin_amdgcn_ballot_w64(d != 0) != 0;  // (wave-uniform)
}
__device__ __forceinline__ uint64_t ct_readlane64(uint64_t v, uint32_t e) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)e);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)e);
  return ((uint64_t)hi << 32) | lo;
}

extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_compare(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
              const uint64_t* __restrict__ lens, const uint64_t* __restrict__ ekey,
              const uint32_t* __restrict__ erow, uint32_t m, const uint32_t* __restrict__ wstart,
              const unsigned long long* __restrict__ tasks, uint32_t* __restrict__ neq,
              uint32_t* __restrict__ counters) {
  const unsigned long long total64 = *tasks;
  if (total64 >= (1ull << 32)) {  // (uniform over the grid: nobody compares, the resolve passes stand still)
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[CT_OVERFLOW] = 1u;
    return;
  }
  const uint32_t total = (uint32_t)total64, n_win = ct_window_count(m);
  const uint32_t lane = threadIdx.x & 63u, voff = lane * 16u;
#pragma unroll 1
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&counters[CT_QUEUE], 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (t >= total) break;
    const CtTask task = ct_task_of(wstart, n_win, t);
    const uint32_t first = ct_window_first(task.window), k = ct_window_entries(task.window, m);
    const uint32_t p = task.piece;
    uint32_t f = 0, g = 0, g_before = 0;
    uint64_t len = 0, off = 0;
    bool live = false;
    if (lane < k) {
      f = erow[first + lane];
      g = (uint32_t)ekey[first + lane];
      g_before = lane ? (uint32_t)ekey[first + lane - 1] : 0u;
      len = lens[f];
      off = offs[f];
      // a refuted entry is not read again (relaxed: a stale 0 costs this piece's loads)
      live = ct_entry_in_piece(len, p) && __atomic_load_n(&neq[f], __ATOMIC_RELAXED) == 0u;
    }
    const uint32_t heads = (uint32_t)__ballot(lane < k && ct_run_starts(lane, g, g_before));
    const uint32_t started = (uint32_t)__ballot(live);
    uint32_t alive = started;  // entries not refuted yet (uniform; k <= 32)
    const uint32_t n_slices = live ? ct_slices(ct_piece_bytes(len, p)) : 0u;
    const uint64_t piece0 = (uint64_t)p * CT_PIECE_BYTES;
#pragma unroll 1
    for (uint32_t s = 0; s < CT_PIECE_SLICES; ++s) {
      uint32_t left = alive & (uint32_t)__ballot(s < n_slices);  // the entries that reach slice s
      if (!left) break;
      const uint64_t from = piece0 + (uint64_t)s * CT_SLICE_BYTES;
      DupSlice ref, cur, nxt;
      uint32_t e = dup_first_bit(left);
      uint64_t len_e = ct_readlane64(len, e);
      uint32_t loaded = ct_run_of(heads, e);
      // an entry and its pivot are of one class: one length, so one limit and one tail for both
      uint32_t limit = ct_slice_limit(len_e, from);
      ct_load_slice(ref, arena + offs[(uint32_t)__builtin_amdgcn_readlane((int)g, (int)e)] + from, limit, voff);
      ct_load_slice(cur, arena + ct_readlane64(off, e) + from, limit, voff);
#pragma unroll 1
      for (;;) {
        left &= left - 1u;
        uint32_t e2 = 0, limit2 = 0;
        uint64_t len_e2 = 0;
        if (left) {  // (uniform) the next alive entry's slice, in flight during this compare
          e2 = dup_first_bit(left);
          len_e2 = ct_readlane64(len, e2);
          limit2 = ct_slice_limit(len_e2, from);
          ct_load_slice(nxt, arena + ct_readlane64(off, e2) + from, limit2, voff);
        }
        bool differ;
        if (from + CT_SLICE_BYTES < len_e) {  // (uniform) not the content's last slice
          differ = dup_slices_differ(ref, cur);
        } else {
          const uint4 mask4 = make_uint4(ct_last_quad_mask(len_e, 0), ct_last_quad_mask(len_e, 1),
                                         ct_last_quad_mask(len_e, 2), ct_last_quad_mask(len_e, 3));
          differ = ct_tail_slices_differ(ref, cur, ct_last_quad(len_e, from), mask4, lane);
        }
        if (differ) alive &= ~(1u << e);
        if (!left) break;
        e = e2;
        len_e = len_e2;
        limit = limit2;
        cur = nxt;
        const uint32_t run = ct_run_of(heads, e);
        if (run != loaded) {  // (uniform) the window's next pivot
          loaded = run;
          ct_load_slice(ref, arena + offs[(uint32_t)__builtin_amdgcn_readlane((int)g, (int)e)] + from, limit, voff);
        }
      }
    }
    const uint32_t refuted = started & ~alive;
    if (lane < k && ((refuted >> lane) & 1u)) __atomic_store_n(&neq[f], 1u, __ATOMIC_RELAXED);
  }
}

// ---- the resolve passes ----------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_resolve_equal(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ erow, uint32_t m,
                    const uint32_t* __restrict__ neq, uint32_t* __restrict__ slot,
                    uint32_t* __restrict__ rep_exact, uint32_t* __restrict__ counters) {
  if (counters[CT_OVERFLOW]) return;
  const uint32_t j = blockIdx.x * CT_THREADS + threadIdx.x;
  bool unequal = false;
  if (j < m) {
    const uint32_t f = erow[j], g = (uint32_t)ekey[j];
    unequal = neq[f] != 0u;
    if (unequal) atomicMin(&slot[g], f);
    else rep_exact[f] = g;
  }
  const uint64_t votes = __ballot(unequal);
  if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(&counters[CT_UNEQUAL], (uint32_t)__popcll(votes));
}

extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_resolve_unequal(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ erow, uint32_t m,
                      uint64_t n, uint32_t* __restrict__ neq, const uint32_t* __restrict__ slot,
                      uint32_t* __restrict__ rep_exact, uint64_t* __restrict__ ekey_in,
                      uint32_t* __restrict__ erow_in, uint32_t* __restrict__ counters) {
  const uint32_t j = blockIdx.x * CT_THREADS + threadIdx.x;
  const bool stand_still = counters[CT_OVERFLOW] != 0u;
  bool unresolved = false;
  if (j < m) {
    const uint32_t f = erow[j], g = (uint32_t)ekey[j];
    uint64_t key = n;  // resolved
    if (stand_still) {
      key = g;
      unresolved = true;
    } else if (neq[f] != 0u) {
      const uint32_t h = slot[g];  // the smallest unequal row of pivot g
      if (h == f) {
        rep_exact[f] = f;  // a head, and the others' pivot
      } else {
        key = h;
        unresolved = true;
      }
      neq[f] = 0u;
    }
    ekey_in[j] = key;
    erow_in[j] = f;
  }
  const uint64_t votes = __ballot(unresolved);
  if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(&counters[CT_UNRESOLVED], (uint32_t)__popcll(votes));
}

// ---- the digest finish -----------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_mark(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ erow, uint32_t m,
           uint32_t* __restrict__ pval) {
  const uint32_t j = blockIdx.x * CT_THREADS + threadIdx.x;
  if (j >= m) return;
  const uint32_t g = (uint32_t)ekey[j];
  pval[erow[j]] = g;
  pval[g] = g;  // (a pivot is resolved, so no entry of its own writes it; every writer stores g)
}
extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_mark_keys(const uint32_t* __restrict__ pval, uint64_t n, uint64_t* __restrict__ skeys,
                uint32_t* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * CT_THREADS + threadIdx.x;
  const bool marked = i < n && pval[i] != 0xFFFFFFFFu;
  if (i < n) skeys[i] = marked ? 0ull : 1ull;
  const uint64_t votes = __ballot(marked);
  if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(&counters[CT_MARKED], (uint32_t)__popcll(votes));
}
extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_gather(const uint32_t* __restrict__ order, const uint32_t* __restrict__ pval,
             const uint64_t* __restrict__ offs, const uint64_t* __restrict__ lens, uint32_t marked,
             uint64_t* __restrict__ coffs, uint64_t* __restrict__ clens, uint32_t* __restrict__ cpiv) {
  const uint32_t j = blockIdx.x * CT_THREADS + threadIdx.x;
  if (j >= marked) return;
  const uint32_t r = order[j];
  coffs[j] = offs[r];
  clens[j] = lens[r];
  cpiv[j] = pval[r];
}

extern "C" __global__ void __launch_bounds__(CT_THREADS)
sd_ct_count_heads(const uint32_t* __restrict__ rep, const uint64_t* __restrict__ lens,
                  const uint32_t* __restrict__ rep_exact, uint64_t n, unsigned long long* __restrict__ objects) {
  const uint64_t i = (uint64_t)blockIdx.x * CT_THREADS + threadIdx.x;
  bool head = false;
  if (i < n) {
    const uint32_t h = rep_exact[i];
    head = h == (uint32_t)i;
#if SD_DBG
    SD_DBG_CHECK(h <= i, "group_exact_contents: row %llu has rep_exact %u after it", (unsigned long long)i, h);
    if (h < i)
      SD_DBG_CHECK(rep_exact[h] == h && rep[h] == rep[i] && lens[h] == lens[i],
                   "group_exact_contents: row %llu's rep_exact %u is not a head of its class",
                   (unsigned long long)i, h);
#endif
  }
  const uint64_t votes = __ballot(head);
  if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(objects, (unsigned long long)__popcll(votes));
}

// ---- launchers -------------------------------------------------------------------------------
static inline uint32_t ct_grid(uint64_t n) { return (uint32_t)((n + CT_THREADS - 1) / CT_THREADS); }
static inline bool ct_ok(uint64_t n) { return n > 0 && n <= CT_MAX_ROWS; }

hipError_t ct_check_bounds(uint64_t arena_bytes, const uint64_t* offs, const uint64_t* lens, uint64_t n,
                           uint32_t* counters, hipStream_t s) {
  if (!ct_ok(n)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counters, 0, CT_COUNTERS * 4, s);
  if (e != hipSuccess) return e;
  sd_ct_check_bounds<<<ct_grid(n), CT_THREADS, 0, s>>>(offs, lens, n, arena_bytes, counters);
  return hipGetLastError();
}

hipError_t ct_first_entries(const uint32_t* cls, uint64_t n, uint32_t* rep_exact, uint64_t* ekey_in,
                            uint32_t* erow_in, uint32_t* neq, hipStream_t s) {
  if (!ct_ok(n)) return hipErrorInvalidValue;
  sd_ct_first_entries<<<ct_grid(n), CT_THREADS, 0, s>>>(cls, n, rep_exact, ekey_in, erow_in, neq);
  return hipGetLastError();
}

hipError_t ct_round(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens, uint64_t n,
                    uint32_t m, const ContentCompareWs& L, uint32_t* rep_exact, uint32_t grid,
                    hipStream_t s) {
  if (!ct_ok(n) || m == 0 || m > n || grid == 0) return hipErrorInvalidValue;
  const uint32_t n_win = ct_window_count(m);
  hipError_t e = hipMemsetAsync(L.tasks, 0, 8, s);
  // the queue and the round's unresolved count start at 0; CT_UNEQUAL accumulates over the call
  if (e == hipSuccess) e = hipMemsetAsync(L.counters + CT_UNRESOLVED, 0, (CT_QUEUE + 1 - CT_UNRESOLVED) * 4, s);
  if (e != hipSuccess) return e;
  sd_ct_windows<<<ct_grid(n_win), CT_THREADS, 0, s>>>(L.ekey, L.erow, lens, m, L.wpieces, L.slot, L.tasks);
  if ((e = exclusive_scan_u32(L.wpieces, L.wstart, n_win, L.scan, s)) != hipSuccess) return e;
  sd_ct_compare<<<grid, CT_THREADS, 0, s>>>(arena, offs, lens, L.ekey, L.erow, m, L.wstart, L.tasks, L.neq,
                                            L.counters);
  sd_ct_resolve_equal<<<ct_grid(m), CT_THREADS, 0, s>>>(L.ekey, L.erow, m, L.neq, L.slot, rep_exact, L.counters);
  sd_ct_resolve_unequal<<<ct_grid(m), CT_THREADS, 0, s>>>(L.ekey, L.erow, m, n, L.neq, L.slot, rep_exact,
                                                          L.ekey_in, L.erow_in, L.counters);
  return hipGetLastError();
}

hipError_t ct_mark(const ContentCompareWs& L, uint32_t m, uint64_t n, hipStream_t s) {
  if (!ct_ok(n) || m == 0 || m > n) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(L.pval, 0xFF, n * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(L.counters + CT_MARKED, 0, 4, s);
  if (e != hipSuccess) return e;
  sd_ct_mark<<<ct_grid(m), CT_THREADS, 0, s>>>(L.ekey, L.erow, m, L.pval);
  sd_ct_mark_keys<<<ct_grid(n), CT_THREADS, 0, s>>>(L.pval, n, L.skeys, L.counters);
  return hipGetLastError();
}

hipError_t ct_gather(const ContentCompareWs& L, const uint64_t* offs, const uint64_t* lens,
                     uint32_t marked, hipStream_t s) {
  if (marked == 0) return hipErrorInvalidValue;
  sd_ct_gather<<<ct_grid(marked), CT_THREADS, 0, s>>>(L.order, L.pval, offs, lens, marked, L.coffs, L.clens,
                                                      L.cpiv);
  return hipGetLastError();
}

hipError_t ct_count_heads(const uint32_t* rep, const uint64_t* lens, const uint32_t* rep_exact, uint64_t n,
                          uint64_t* d_objects, hipStream_t s) {
  if (!ct_ok(n)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_objects, 0, 8, s);
  if (e != hipSuccess) return e;
  sd_ct_count_heads<<<ct_grid(n), CT_THREADS, 0, s>>>(rep, lens, rep_exact, n, (unsigned long long*)d_objects);
  return hipGetLastError();
}

SD_DBG_ACCESSOR(sd_dbg_violations_content_compare)

}  // namespace sdcas
