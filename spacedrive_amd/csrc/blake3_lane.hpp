// blake3_lane.hpp — one lane walks one BLAKE3 message: everything around compress()
// (blake3_device.hpp) that K1, K2, K1L, K1P and the validator's lane kernel share, each piece
// once.  A lane streams its message in 128-B lines (a block pair, 8 x global_load_dwordx4)
// one line ahead, builds the 16 message words of each block, masks the final block, sets
// CHUNK_START / CHUNK_END / ROOT, and keeps the chaining values of the left-balanced tree's
// pending subtrees on a stack column of its own.
//
// Two message layouts:
//   PLAIN     message = content (file_checksum, hash.rs:11-25);
//   PREFIXED  message = le64(size) || content (generate_cas_id, cas.rs:23-62): the prefix
//             shifts the content by exactly two 32-bit words, which is register renaming
//             (a 2-word carry c0, c1 = the tail of the previous line), not byte shuffling.
// Everything is a force-inlined template over the same expressions, and compiles for the
// host too: tests/native/lane_walker_test.cpp walks both layouts on the CPU against the
// oracle under sanitizers.
#pragma once
#include "blake3_device.hpp"

namespace sdcas {

#if !defined(__HIPCC__)
struct uint4 {  // HIP's 16-B quad
  uint32_t x, y, z, w;
};
#endif

enum Layout : uint32_t { PLAIN = 0u, PREFIXED = 8u };  // the value: the prefix's bytes

// Zero the message words past the block's first blen bytes.
SD_B3_HD void mask_tail(uint32_t (&m)[16], uint32_t blen) {
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const int vb = (int)blen - 4 * w;
    m[w] &= vb >= 4 ? 0xFFFFFFFFu : (vb <= 0 ? 0u : ((1u << (8 * vb)) - 1u));
  }
}

// ---- line -> the 16 message words of its low and its high block -------------------------
SD_B3_HD void quads_to_words(uint32_t (&m)[16], const uint4& a0, const uint4& a1, const uint4& a2,
                             const uint4& a3) {
  m[0] = a0.x;  m[1] = a0.y;  m[2] = a0.z;  m[3] = a0.w;
  m[4] = a1.x;  m[5] = a1.y;  m[6] = a1.z;  m[7] = a1.w;
  m[8] = a2.x;  m[9] = a2.y;  m[10] = a2.z; m[11] = a2.w;
  m[12] = a3.x; m[13] = a3.y; m[14] = a3.z; m[15] = a3.w;
}
// PREFIXED: words 0 and 1 of the low block are the carry, and the high block starts at A[3].z.
template <Layout L>
SD_B3_HD void words_lo(uint32_t (&m)[16], const uint4 (&A)[8], uint32_t c0 = 0u, uint32_t c1 = 0u) {
  if (L == PLAIN) {
    quads_to_words(m, A[0], A[1], A[2], A[3]);
  } else {
    m[0] = c0;      m[1] = c1;      m[2] = A[0].x;  m[3] = A[0].y;
    m[4] = A[0].z;  m[5] = A[0].w;  m[6] = A[1].x;  m[7] = A[1].y;
    m[8] = A[1].z;  m[9] = A[1].w;  m[10] = A[2].x; m[11] = A[2].y;
    m[12] = A[2].z; m[13] = A[2].w; m[14] = A[3].x; m[15] = A[3].y;
  }
}
template <Layout L>
SD_B3_HD void words_hi(uint32_t (&m)[16], const uint4 (&A)[8]) {
  if (L == PLAIN) {
    quads_to_words(m, A[4], A[5], A[6], A[7]);
  } else {
    m[0] = A[3].z;  m[1] = A[3].w;  m[2] = A[4].x;  m[3] = A[4].y;
    m[4] = A[4].z;  m[5] = A[4].w;  m[6] = A[5].x;  m[7] = A[5].y;
    m[8] = A[5].z;  m[9] = A[5].w;  m[10] = A[6].x; m[11] = A[6].y;
    m[12] = A[6].z; m[13] = A[6].w; m[14] = A[7].x; m[15] = A[7].y;
  }
}
// a full 64-B block of chunk `ctr`: the low and the high block of the line in A
template <Layout L>
SD_B3_HD void compress_lo(uint32_t (&cv)[8], const uint4 (&A)[8], uint32_t c0, uint32_t c1,
                          uint32_t ctr, uint32_t f) {
  uint32_t m[16];
  words_lo<L>(m, A, c0, c1);
  compress(cv, m, ctr, 0u, BLOCK_LEN, f);
}
template <Layout L>
SD_B3_HD void compress_hi(uint32_t (&cv)[8], const uint4 (&A)[8], uint32_t ctr, uint32_t f) {
  uint32_t m[16];
  words_hi<L>(m, A);
  compress(cv, m, ctr, 0u, BLOCK_LEN, f);
}
// both back to back; the carry moves on to the line's tail (dead code for PLAIN)
template <Layout L>
SD_B3_HD void compress_line(uint32_t (&cv)[8], const uint4 (&A)[8], uint32_t& c0, uint32_t& c1,
                            uint32_t ctr, uint32_t f0, uint32_t f1) {
  compress_lo<L>(cv, A, c0, c1, ctr, f0);
  compress_hi<L>(cv, A, ctr, f1);
  c0 = A[7].z;
  c1 = A[7].w;
}

// ---- line loads ---------------------------------------------------------------------------
// Line P (quads 8P..8P+7) of the lane's content: 8 x dwordx4 issued back to back, all in bounds.
SD_B3_HD void line(const uint4* __restrict__ q, uint32_t P, uint4 (&buf)[8]) {
  const uint4* p = q + 8u * P;
#pragma unroll
  for (int i = 0; i < 8; ++i) buf[i] = p[i];
}
// Always 8 x 16-B loads: a quad at or past the 16-B round-up of len is re-pointed at quad 0
// (in bounds: line_clamped is never asked for a line of a content without a readable quad 0)
// instead of being predicated off — a `cond ? q[i] : 0` load is lowered to four dword loads
// per quad.  Its garbage can only reach the message's final block, which mask_tail() zeroes
// past the end.
SD_B3_HD void line_clamped(const uint4* __restrict__ q, uint32_t P, uint32_t len, uint4 (&buf)[8]) {
  const uint32_t b0 = P << 7;
#pragma unroll
  for (int i = 0; i < 8; ++i) buf[i] = q[(b0 + 16u * i < len) ? 8u * P + i : 0u];
}

// ---- the chaining-value stack -------------------------------------------------------------
// A lane's pending subtree CVs in an LDS column of its own, word-major [depth][word][thread]
// so every push/pop is a conflict-free dword access.  BOTTOM_IN_REGS keeps the bottom entry
// (the largest subtree, touched least) in VGPRs, which saves one LDS level.  Without it the
// stack has no such member at all (a dead one changed K1's register assignment).
template <bool BOTTOM_IN_REGS>
struct CvBottom {
  uint32_t bottom[8];
};
template <>
struct CvBottom<false> {};
template <int BLOCK, bool BOTTOM_IN_REGS>
struct CvStack : CvBottom<BOTTOM_IN_REGS> {
  uint32_t (*s)[8][BLOCK];
  uint32_t t;
  uint32_t sp = 0;
  SD_B3_HD CvStack(uint32_t (*lds)[8][BLOCK], uint32_t thread) : s(lds), t(thread) {}
  SD_B3_HD void push(const uint32_t (&cv)[8]) {
    if constexpr (BOTTOM_IN_REGS) {
      if (sp == 0) {
#pragma unroll
        for (int w = 0; w < 8; ++w) this->bottom[w] = cv[w];
      } else {
        store(sp - 1, cv);
      }
    } else {
      store(sp, cv);
    }
    ++sp;
  }
  SD_B3_HD void pop(uint32_t (&out)[8]) {
    --sp;
    if constexpr (BOTTOM_IN_REGS) {
      if (sp == 0) {
#pragma unroll
        for (int w = 0; w < 8; ++w) out[w] = this->bottom[w];
      } else {
        load(sp - 1, out);
      }
    } else {
      load(sp, out);
    }
  }
  SD_B3_HD void store(uint32_t d, const uint32_t (&cv)[8]) {
#pragma unroll
    for (int w = 0; w < 8; ++w) s[d][w][t] = cv[w];
  }
  SD_B3_HD void load(uint32_t d, uint32_t (&out)[8]) {
#pragma unroll
    for (int w = 0; w < 8; ++w) out[w] = s[d][w][t];
  }
};

// Left-balanced tree: cv is the CV of the total-th completed chunk (counted from 1) — merge
// while the count has trailing zeros, then push.  A parent that empties the stack takes
// bottom_flag (ROOT where the caller knows that parent to be the message's root).
template <class Stack>
SD_B3_HD void merge_push(Stack& stk, uint32_t (&cv)[8], uint32_t total, uint32_t bottom_flag = 0u) {
  while ((total & 1u) == 0u) {
    uint32_t left[8];
    stk.pop(left);
    parent(cv, left, cv, stk.sp == 0 ? bottom_flag : 0u);
    total >>= 1;
  }
  stk.push(cv);
}
// cv is the rightmost subtree: pop and parent until the stack is empty
template <class Stack>
SD_B3_HD void fold(Stack& stk, uint32_t (&cv)[8], uint32_t bottom_flag) {
  while (stk.sp > 0) {
    uint32_t left[8];
    stk.pop(left);
    parent(cv, left, cv, stk.sp == 0 ? bottom_flag : 0u);
  }
}

// ---- chunks ---------------------------------------------------------------------------------
// One FULL 1 KiB chunk c (not the message's last): 16 blocks of 64 B with the chunk flags on
// blocks 0 and 15 — none of last_chunk's per-block length, mask and flag logic, and unclamped
// loads for the chunk's own lines (a full chunk's content quads are readable: the message
// runs past the chunk, so the content's 16-B round-up does too).  A holds line 8c on entry
// and line 8(c+1) on exit.  K1's ping-pong schedule (no register moves): lines 0..5 in the
// loop, 6 and 7 peeled so that the clamped prefetch of the next chunk's first line (that
// chunk may be the partial last one) does not merge with the unclamped loads into per-dword
// select loads (that merge measured 2.8x slower).
template <Layout L>
SD_B3_HD void full_chunk(const uint4* __restrict__ q, uint32_t len, uint32_t c, uint32_t (&cv)[8],
                         uint4 (&A)[8], uint4 (&B)[8], uint32_t& c0, uint32_t& c1) {
  set_iv(cv);
#pragma unroll 1
  for (uint32_t pp = 0; pp < 3; ++pp) {
    const uint32_t P = 8u * c + 2u * pp;
    line(q, P + 1, B);
    compress_line<L>(cv, A, c0, c1, c, pp == 0 ? (uint32_t)CHUNK_START : 0u, 0u);
    line(q, P + 2, A);
    compress_line<L>(cv, B, c0, c1, c, 0u, 0u);
  }
  line(q, 8u * c + 7u, B);
  compress_line<L>(cv, A, c0, c1, c, 0u, 0u);
  line_clamped(q, 8u * c + 8u, len, A);
  compress_line<L>(cv, B, c0, c1, c, 0u, CHUNK_END);
}

// The generic chunk: the first cblocks blocks of chunk c of a message of L + len bytes, with
// per-block length, tail mask, CHUNK_START / CHUNK_END and, when `root`, ROOT on the last
// block.  A holds line 8c and (c0, c1) its carry on entry.
template <Layout L>
SD_B3_HD void last_chunk(const uint4* __restrict__ q, uint32_t len, uint32_t c, uint32_t cblocks,
                         bool root, uint32_t (&cv)[8], uint4 (&A)[8], uint4 (&B)[8], uint32_t& c0,
                         uint32_t& c1) {
  const uint32_t mlen = len + L;
  set_iv(cv);
  for (uint32_t b = 0; b < cblocks; b += 2) {
    if (b + 2 < cblocks) line_clamped(q, 8u * c + (b >> 1) + 1u, len, B);
    const uint32_t j = 16u * c + b;  // global block index of the line's first block
    {
      uint32_t m[16];
      words_lo<L>(m, A, c0, c1);
      const uint32_t rem = mlen - (j << 6), blen = rem < 64u ? rem : 64u;
      if (blen < 64u) mask_tail(m, blen);
      const bool end = (b + 1 == cblocks);
      const uint32_t f = (b == 0 ? (uint32_t)CHUNK_START : 0u) | (end ? (uint32_t)CHUNK_END : 0u) |
                         (end && root ? (uint32_t)ROOT : 0u);
      compress(cv, m, c, 0u, blen, f);
    }
    if (b + 1 < cblocks) {
      uint32_t m[16];
      words_hi<L>(m, A);
      const uint32_t rem = mlen - ((j + 1) << 6), blen = rem < 64u ? rem : 64u;
      if (blen < 64u) mask_tail(m, blen);
      const bool end = (b + 2 == cblocks);
      const uint32_t f = (end ? (uint32_t)CHUNK_END : 0u) | (end && root ? (uint32_t)ROOT : 0u);
      compress(cv, m, c, 0u, blen, f);
    }
    c0 = A[7].z;
    c1 = A[7].w;
    if (b + 2 < cblocks) {  // the load's condition: B is never read unloaded (same device code)
#pragma unroll
      for (int i = 0; i < 8; ++i) A[i] = B[i];
    }
  }
}

// ---- the whole message --------------------------------------------------------------------
// cv <- the root CV of the message over content q[0, len) (PREFIXED: after le64(size)): the
// first line, full chunks with merge_push, the last chunk, the fold.  Quads are read up to
// the content's 16-B round-up, and quad 0 (PREFIXED: of an empty content too, see the ABI;
// a PLAIN 0-byte buffer reads nothing and hashes one empty block).
template <Layout L, class Stack>
SD_B3_HD void lane_message(const uint4* __restrict__ q, uint32_t len, uint64_t size, Stack& stk,
                           uint32_t (&cv)[8]) {
  const uint32_t mlen = len + L;
  const bool empty = L == PLAIN && len == 0;  // one empty block
  const uint32_t nblocks = empty ? 1u : (mlen + 63u) >> 6;
  const uint32_t nchunks = empty ? 1u : (mlen + 1023u) >> 10;
  uint32_t c0 = (uint32_t)size, c1 = (uint32_t)(size >> 32);
  uint4 A[8], B[8];
  if (!empty) {
    line_clamped(q, 0, len, A);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) A[i].x = A[i].y = A[i].z = A[i].w = 0u;
  }
  for (uint32_t c = 0; c + 1 < nchunks; ++c) {
    full_chunk<L>(q, len, c, cv, A, B, c0, c1);
    merge_push(stk, cv, c + 1);
  }
  const uint32_t c = nchunks - 1;
  last_chunk<L>(q, len, c, nblocks - 16u * c, c == 0, cv, A, B, c0, c1);
  fold(stk, cv, ROOT);
}

}  // namespace sdcas
