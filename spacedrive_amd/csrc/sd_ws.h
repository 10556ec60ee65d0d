// sd_ws.h — the one workspace carver (host only, no HIP include).  Every device chain here
// carves typed arrays out of one untyped buffer; a layout is ONE function that walks a
// WsCarve, and the same function both sizes the buffer (base == nullptr: measure only) and
// hands out the pointers, so the two cannot drift apart.
#pragma once
#include <stddef.h>
#include <stdint.h>

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
// packed whole-file contents start on 128-B lines: a K2 lane's line pair is one cache line
inline size_t up128(size_t x) { return (x + 127) & ~(size_t)127; }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct WsCarve {
  uintptr_t base, cur;  // integers: measuring from a null base does no arithmetic on null
  explicit WsCarve(void* b) : base((uintptr_t)b), cur((uintptr_t)b) {}
  // `count` elements of T at the cursor; the cursor advances by up256(count * sizeof(T)) (so a
  // few counters, take<uint64_t>(2) say, are a 256-B block of their own)
  template <class T>
  T* take(uint64_t count) {
    T* p = (T*)cur;
    cur += up256((size_t)count * sizeof(T));
    return p;
  }
  // a fixed reserve (a 256-B counter block, or bytes a total keeps that no launcher reads)
  void skip(size_t bytes) { cur += bytes; }
  void* rest() const { return (void*)cur; }  // where a nested workspace starts
  void* nest(size_t bytes) { void* p = rest(); skip(bytes); return p; }  // a nested workspace
  size_t bytes() const { return (size_t)(cur - base); }
};
