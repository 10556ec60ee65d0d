// cas_inplace.hip — cas_ids from WHOLE file contents resident in HBM (K1P + the routing).
//
// The cas_id kernels of cas_hash.hip want a sampled file (size > 100 KiB, cas.rs:31-58)
// already gathered into a 57,344-B row.  A caller that holds the whole file in device memory
// — the validator's windows do: every byte goes to HBM for file_checksum — gets its cas_id
// here straight from the file's six segments, with no gather row and no second read.
//
//   classify  one pass over (offs, lens): the bounds verdict (like the checksum batch chain),
//             a u32 length array in which sampled and rejected files count as empty, and the
//             index list of the sampled files.  Whole files (<= 100 KiB) then run in place
//             through the packed dispatcher (K2 / K1L) over that length array and keys land
//             at their own index; the list feeds K1P, which runs after it on the stream and
//             writes the sampled files' keys.
//   K1P       K1L's wave-per-file shape: lane c hashes chunk c of the 57-chunk message
//             M = le64(len) || header || 4 samples || footer, reading its 1,016 body bytes and
//             its 8 carry bytes where they lie in the file (sd_inplace_plan.h), and the lanes'
//             CVs merge across lanes with segment_merge (blake3_tree.hpp).  Sample and footer
//             offsets have any byte alignment (k*j and len are arbitrary), so a lane loads 4-B
//             aligned dwords (dwordx4 runs plus one per 128-B line) and realigns them in registers
//             with v_alignbyte_b32 by its own byte shift: ~256 alignbytes on top of a chunk's
//             ~10,900 VALU instructions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake3_lane.hpp"
#include "blake3_tree.hpp"
#include "sd_debug.h"
#include "sd_inplace_plan.h"
#include "sd_kernels.h"
#include "sd_ws.h"

namespace sdcas {

constexpr uint64_t INPLACE_MAX_LEN = 64ull << 30;  // the checksum batch chain's bound

// ---- classify ---------------------------------------------------------------------------
// counters[0] |= 1 for a buffer over 64 GiB, 4 for one misaligned or outside the arena (the
// flags of the checksum batch chain); counters[1] += sampled files.  A rejected buffer is
// never read: it classifies as an empty whole file and the call fails before any hash runs.
extern "C" __global__ void __launch_bounds__(256)
sd_cas_inplace_classify(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ lens,
                        uint64_t n, uint64_t arena_bytes, uint32_t* __restrict__ lens32,
                        uint32_t* __restrict__ sampled_idx, uint32_t* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool sampled = false;
  if (i < n) {
    const uint64_t off = offs[i], len = lens[i];
    const bool ok = (off & 15) == 0 && len <= arena_bytes && off <= arena_bytes - len &&
                    len <= INPLACE_MAX_LEN;
    if (!ok) atomicOr(&counters[0], len > INPLACE_MAX_LEN ? 1u : 4u);
    sampled = ok && len > MINIMUM_FILE_SIZE;
    lens32[i] = ok && !sampled ? (uint32_t)len : 0u;
  }
  // one atomic per wave: its sampled files take consecutive list entries
  const uint64_t votes = __ballot(sampled);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0 && votes) base = atomicAdd(&counters[1], (uint32_t)__popcll(votes));
  base = __shfl(base, 0, 64);
  if (sampled) {
    const uint32_t slot = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    SD_DBG_CHECK(slot < n, "sampled list slot %u >= n %llu", slot, (unsigned long long)n);
    sampled_idx[slot] = (uint32_t)i;
  }
}

// ---- K1P ----------------------------------------------------------------------------------
struct __attribute__((aligned(4))) Quad4 {  // a dwordx4 load from a 4-B aligned address
  uint32_t x, y, z, w;
};

__device__ __forceinline__ uint32_t shifted(uint32_t hi, uint32_t lo, uint32_t sh) {
  return __builtin_amdgcn_alignbyte(hi, lo, sh);  // bytes [sh, sh + 4) of lo | hi << 32
}

// Line P (128 B) of a chunk body that starts `sh` bytes into the dword at w: eight dwordx4
// from the aligned address, the one dword after them, and 32 alignbytes.  The chunk's last
// line (more == false) takes no dword after it: its two last words belong to the next chunk
// (never used here), and at the footer that dword would lie past the file's 16-B round-up.
__device__ __forceinline__ void load_line_shifted(const uint32_t* __restrict__ w, uint32_t P,
                                                  uint32_t sh, bool more, uint4 (&buf)[8]) {
  const Quad4* q = reinterpret_cast<const Quad4*>(w) + 8u * P;
  Quad4 r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = q[i];
  const uint32_t after = w[more ? 32u * P + 32u : 32u * P];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    buf[i].x = shifted(r[i].y, r[i].x, sh);
    buf[i].y = shifted(r[i].z, r[i].y, sh);
    buf[i].z = shifted(r[i].w, r[i].z, sh);
    buf[i].w = shifted(i < 7 ? r[(i + 1) & 7].x : after, r[i].w, sh);
  }
}

// One wave per sampled file; lane c < 56 hashes message chunk c, lane 56 the 8-byte tail
// chunk.  Lanes 56..63 walk the loop over the file's header with the others (no divergence;
// the wave takes the longest lane's time anyway): lane 56 keeps the CV of its first block,
// the others' CVs are never read (57 items enter the merge).
extern "C" __global__ void __launch_bounds__(64)
sd_cas_inplace_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                      const uint64_t* __restrict__ lens, const uint32_t* __restrict__ idx,
                      uint64_t n_idx, uint64_t* __restrict__ keys) {
  const uint32_t lane = threadIdx.x;
  const uint32_t f = idx[blockIdx.x];
  const uint64_t len = lens[f];
  const uint8_t* file = arena + offs[f];
  SD_DBG_CHECK(blockIdx.x < n_idx && len > MINIMUM_FILE_SIZE && len <= INPLACE_MAX_LEN &&
                   (offs[f] & 15) == 0,
               "K1P file %u: len %llu off %llu", f, (unsigned long long)len,
               (unsigned long long)offs[f]);
  const bool body = lane < INPLACE_CHUNKS - 1;
  const bool tail = lane == INPLACE_CHUNKS - 1;
  const uint32_t c = lane;
  // the body: 1,016 bytes of one segment (+ the 8 after them, the next chunk's carry)
  const uint64_t bo = body ? inplace_body_off(len, c) : 0ull;
  const uint32_t sh = (uint32_t)bo & 3u;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(file + (bo - sh));
  SD_DBG_CHECK(bo + 1024u <= len, "K1P file %u chunk %u: body %llu past len %llu", f, c,
               (unsigned long long)bo, (unsigned long long)len);
  // the carry: le64(len) for chunk 0, else the 8 bytes before the body in gathered order
  uint32_t c0 = (uint32_t)len, c1 = (uint32_t)(len >> 32);
  if (c > 0 && (body || tail)) {
    const uint64_t co = inplace_carry_off(len, c);
    const uint32_t cs = (uint32_t)co & 3u;
    const uint32_t* cw = reinterpret_cast<const uint32_t*>(file + (co - cs));
    SD_DBG_CHECK(co + 8u <= len, "K1P file %u chunk %u: carry %llu past len %llu", f, c,
                 (unsigned long long)co, (unsigned long long)len);
    const uint32_t a = cw[0], b = cw[1], d = cw[cs ? 2 : 1];  // no third dword when aligned:
    c0 = shifted(b, a, cs);                                   // at the footer it would lie
    c1 = shifted(d, b, cs);                                   // past the file's round-up
  }
  uint4 A[8], B[8];
  uint32_t cv[8], first[8];
  set_iv(cv);
  load_line_shifted(w, 0, sh, true, A);
#pragma unroll 1
  for (uint32_t pp = 0; pp < 4; ++pp) {
    load_line_shifted(w, 2u * pp + 1u, sh, pp < 3, B);
    {  // line 2pp: the chunk's first block carries CHUNK_START, and is all of the tail chunk
      uint32_t m[16];
      words_lo<PREFIXED>(m, A, c0, c1);
      uint32_t blen = BLOCK_LEN, fl = pp == 0 ? (uint32_t)CHUNK_START : 0u;
      if (pp == 0 && tail) {
#pragma unroll
        for (int k = 2; k < 16; ++k) m[k] = 0u;
        blen = 8u;
        fl |= CHUNK_END;
      }
      compress(cv, m, c, 0u, blen, fl);
      if (pp == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) first[k] = cv[k];
      }
      compress_hi<PREFIXED>(cv, A, c, 0u);
      c0 = A[7].z;
      c1 = A[7].w;
    }
    if (pp < 3) load_line_shifted(w, 2u * pp + 2u, sh, true, A);
    // line 2pp + 1: CHUNK_END on the chunk's 16th block
    compress_line<PREFIXED>(cv, B, c0, c1, c, 0u, pp == 3 ? (uint32_t)CHUNK_END : 0u);
  }
  if (tail) {
#pragma unroll
    for (int k = 0; k < 8; ++k) cv[k] = first[k];
  }
  uint32_t count = INPLACE_CHUNKS;
  segment_merge<64, 1u>(cv, lane, count);  // ROOT on the last pair
  if (lane == 0) keys[f] = key_of(cv);
}

// ---- host launchers -------------------------------------------------------------------------
// workspace: counters (256 B) | lens32 [n] | sampled_idx [n]
InplaceWs inplace_layout(void* ws, uint64_t n) {
  WsCarve w(ws);  InplaceWs L;
  L.counters = w.take<uint32_t>(64);  L.lens32 = w.take<uint32_t>(n);  L.sampled_idx = w.take<uint32_t>(n);
  L.bytes = w.bytes();  return L;
}
size_t inplace_workspace_bytes(uint64_t n) { return inplace_layout(nullptr, n).bytes; }

hipError_t inplace_classify(uint64_t arena_bytes, const uint64_t* offs, const uint64_t* lens,
                            uint64_t n, void* ws, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n >= (1ull << 32)) return hipErrorInvalidValue;
  const InplaceWs L = inplace_layout(ws, n);
  hipError_t e = hipMemsetAsync(L.counters, 0, 8, s);
  if (e != hipSuccess) return e;
  sd_cas_inplace_classify<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(
      offs, lens, n, arena_bytes, L.lens32, L.sampled_idx, L.counters);
  return hipGetLastError();
}

hipError_t hash_inplace_sampled(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens,
                                const uint32_t* idx, uint64_t n_idx, uint64_t* keys,
                                hipStream_t s) {
  if (n_idx == 0) return hipSuccess;
  if (n_idx >= (1ull << 31)) return hipErrorInvalidValue;
  sd_cas_inplace_kernel<<<(uint32_t)n_idx, 64, 0, s>>>(arena, offs, lens, idx, n_idx, keys);
  return hipGetLastError();
}

SD_DBG_ACCESSOR(sd_dbg_violations_inplace)

}  // namespace sdcas
