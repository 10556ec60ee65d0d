// Walks whole BLAKE3 messages on the CPU with blake3_lane.hpp's lane_message — the lane
// program of K2 (PREFIXED) and of the validator's lane kernel (PLAIN) — over a one-thread
// CvStack in a plain array.  No HIP runtime call.  One request per stdin line,
//   <mode> <len> <size>      mode p: PLAIN walk of X; x: PREFIXED walk of (X, size);
//                                 i: PLAIN walk of le64(size) || X
// with X = the len bytes of content_byte(len, i) below, and one output line
//   <mode> <len> <64 hex digits: the root CV>
// Every content sits in an allocation of exactly its 16-B round-up (PREFIXED: at least the
// one quad that the ABI keeps readable for an empty content), padded with 0xFF: a load past
// the round-up is an AddressSanitizer report, padding that reaches a block a wrong digest.
// tests/test_lane_walker_cpu.py compares the digests with the oracle.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "blake3_lane.hpp"

using namespace sdcas;

static uint8_t content_byte(uint32_t len, uint32_t i) {
  return (uint8_t)(((i + 1u) * 2654435761u + len * 0x9E3779B1u) >> 11);
}

int main() {
  char mode;
  uint32_t len;
  uint64_t size;
  while (scanf(" %c %" SCNu32 " %" SCNu64, &mode, &len, &size) == 3) {
    const uint32_t head = mode == 'i' ? 8u : 0u;  // le64(size) written into the buffer itself
    const uint32_t blen = head + len;
    size_t alloc = ((size_t)blen + 15u) / 16u * 16u;
    if (mode == 'x' && alloc == 0) alloc = 16;
    uint8_t* buf = (uint8_t*)malloc(alloc ? alloc : 1);  // 1: a 0-byte content has no quad
    if (!buf) return 2;
    memset(buf, 0xFF, alloc ? alloc : 1);
    for (uint32_t k = 0; k < head; ++k) buf[k] = (uint8_t)(size >> (8 * k));
    for (uint32_t i = 0; i < len; ++i) buf[head + i] = content_byte(len, i);
    uint32_t lds[8][8][1];  // <= 7 pending subtrees below 129 chunks, the bottom one in "VGPRs"
    CvStack<1, true> stk(lds, 0);
    uint32_t cv[8];
    const uint4* q = reinterpret_cast<const uint4*>(buf);
    if (mode == 'x')
      lane_message<PREFIXED>(q, len, size, stk, cv);
    else
      lane_message<PLAIN>(q, blen, 0, stk, cv);
    if (stk.sp != 0) return 3;
    printf("%c %" PRIu32 " ", mode, len);
    for (int w = 0; w < 8; ++w)
      for (int b = 0; b < 4; ++b) printf("%02x", (cv[w] >> (8 * b)) & 0xFFu);
    printf("\n");
    free(buf);
  }
  return 0;
}
