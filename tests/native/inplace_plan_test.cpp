// Prints, for every file size given on stdin (one decimal number per line), what
// sd_inplace_plan.h says about the sampled cas message inside the file:
//   <size> <6 x "off len"> <56 x body offset (chunks 0..55)> <56 x carry offset (chunks 1..56)>
// tests/test_inplace_cpu.py compares the lines with the oracle's literal plan of cas.rs:35-58.
#include <inttypes.h>
#include <stdio.h>

#include "sd_inplace_plan.h"

int main() {
  uint64_t len;
  while (scanf("%" SCNu64, &len) == 1) {
    printf("%" PRIu64, len);
    for (uint32_t s = 0; s < sdcas::INPLACE_SEGMENTS; s++)
      printf(" %" PRIu64 " %" PRIu64, sdcas::inplace_seg_start(len, s), sdcas::inplace_seg_len(s));
    for (uint32_t c = 0; c + 1 < sdcas::INPLACE_CHUNKS; c++)
      printf(" %" PRIu64, sdcas::inplace_body_off(len, c));
    for (uint32_t c = 1; c < sdcas::INPLACE_CHUNKS; c++)
      printf(" %" PRIu64, sdcas::inplace_carry_off(len, c));
    printf("\n");
  }
  return 0;
}
