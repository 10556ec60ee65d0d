// exact_layout_test.cpp — the workspace layouts of the exact duplicate grouping
// (sd_exact_layout, sd_exact_report_layout of libsd_hip_cas.so), printed for
// tests/test_exact_dups_cpu.py in the format of ws_layout_test.cpp.  Host only: never the GPU.
//   L <key> <total> <measured> m:off:need ...
// <total> is the layout carved at a dummy base, <measured> the same layout from a null base;
// every member is printed with its offset and the bytes its launcher indexes there.
#include <stdio.h>

#include "ctx_internal.h"

static char* const BASE = (char*)((uintptr_t)1 << 44);  // never dereferenced

struct Line {
  Line(const char* key, size_t total, size_t measured) {
    printf("L %s %llu %llu", key, (unsigned long long)total, (unsigned long long)measured);
  }
  ~Line() { printf("\n"); }
  Line& m(const char* name, const void* p, unsigned long long need) {
    printf(" %s:%llu:%llu", name, (unsigned long long)((const char*)p - BASE), need);
    return *this;
  }
};
#define M(x, need) m(#x, L.x, (unsigned long long)(need))

int main() {
  char key[96];
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)65537, (uint64_t)1441792}) {
    {
      const ExactWs L = sd_exact_layout(BASE, n);
      snprintf(key, sizeof key, "exact(%llu)", (unsigned long long)n);
      Line(key, L.bytes, sd_exact_layout(nullptr, n).bytes).M(keys, n * 8).M(ids, n * 4).M(counter, 4);
    }
    for (uint64_t m : {(uint64_t)0, n / 2, n})
      for (uint64_t k : {(uint64_t)0, (uint64_t)1024}) {
        const ExactReportWs L = sd_exact_report_layout(BASE, n, m, k);
        snprintf(key, sizeof key, "exact_report(%llu,%llu,%llu)", (unsigned long long)n,
                 (unsigned long long)m, (unsigned long long)k);
        Line(key, L.bytes, sd_exact_report_layout(nullptr, n, m, k).bytes).M(ckeys, m * 8)
            .M(cdigests, m * 32).M(crows, m * 4).M(prior, m * 4).M(crep, m * 4).M(sizes, n * 8)
            .M(state, n).M(rep, n * 4).M(copies, n * 4).M(top_heads, k * 4).M(top_waste, k * 8);
      }
  }
  return 0;
}
