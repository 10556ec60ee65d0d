// sd_piece_queue.h — the validator file path's piece queue (validator_host.cpp): the cutter,
// the reader and the engine under both the windows of small files and the 64 MiB segments of
// big ones.  Host only: the engine reaches the device through the operations passed to it, so
// tests/native/piece_queue_test.cpp drives it on the CPU with a fake device.
//
// A job is a list of UNITS (a window or a segment), each a run of PIECES in the byte order of
// its data.  Unit u lives in slot u % slots of a pinned and a device buffer, its data at
// data_off inside the slot.  Readers (pool threads) take pieces from one cursor over the
// whole job; a piece of unit u waits only for unit u - slots to retire, so the readers never
// join.  One pump thread copies every landed prefix of the current unit to the device as it
// grows (by >= copy_unit bytes, or the rest at completion), alternating over two copy streams,
// issues the unit's work when all of it has landed, retires units in order as their `done`
// events complete, and reads a piece itself when idle.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <vector>

// A/B knobs, the plan's defaults (tools/build_variant.sh + tools/patch_define.py)
#ifndef SD_CK_PIECE_KB
#define SD_CK_PIECE_KB 1024
#endif
#ifndef SD_CK_COPY_MB
#define SD_CK_COPY_MB 8
#endif
#ifndef SD_CK_PUMP_READS
#define SD_CK_PUMP_READS 1
#endif
#ifndef SD_CK_PUMP_ON_POOL
#define SD_CK_PUMP_ON_POOL 1
#endif
#ifndef SD_CK_COPY_STREAMS
#define SD_CK_COPY_STREAMS 2
#endif

namespace sdq {

constexpr uint64_t PIECE = (uint64_t)SD_CK_PIECE_KB << 10;  // the product's read unit

// The cutter: a run of len bytes is max(1, len / piece) pieces, the last one taking the rest
// (so no piece is shorter than `piece` unless the run is).  emit(offset, length), in order.
template <class Emit>
inline uint64_t cut_pieces(uint64_t len, uint64_t piece, Emit&& emit) {
  const uint64_t np = std::max<uint64_t>(1, len / piece);
  for (uint64_t q = 0; q < np; q++) emit(q * piece, q + 1 < np ? piece : len - q * piece);
  return np;
}

// The reader: len bytes of path at file offset foff into dst, through a descriptor of its own
// (the pool's threads have private descriptor tables, HostPool::set_private_fds).  err = the
// errno of a failed open / pread.  irregular = a read that a local regular file never gives:
// data after a short read, or (before_end: the piece ends before the file's planned end) fewer
// bytes than planned.
struct ReadResult { uint64_t got = 0; int err = 0; bool irregular = false; };
inline ReadResult read_piece(const char* path, char* dst, uint64_t foff, uint64_t len, bool before_end) {
  ReadResult r;
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) { r.err = errno; return r; }
  bool was_short = false;
  while (r.got < len) {
    const ssize_t k = pread(fd, dst + r.got, len - r.got, (off_t)(foff + r.got));
    if (k < 0 && errno == EINTR) continue;
    if (k < 0) { r.err = errno; break; }
    if (k == 0) break;  // EOF
    if (was_short) r.irregular = true;
    if ((uint64_t)k < len - r.got) was_short = true;
    r.got += (uint64_t)k;
  }
  close(fd);
  if (r.got < len && before_end) r.irregular = true;
  return r;
}

struct Plan {
  int slots = 3;
  size_t slot_bytes = 0, data_off = 0;  // a slot's size; where a unit's data starts inside it
  uint64_t copy_unit = (uint64_t)SD_CK_COPY_MB << 20;  // a landed prefix is copied once it has grown by this
  int copy_streams = SD_CK_COPY_STREAMS;               // copies alternate over this many streams (1 or 2)
  bool pump_on_pool = SD_CK_PUMP_ON_POOL;  // the pump on a pool thread (1) or on the calling thread (0)
  bool pump_reads = SD_CK_PUMP_READS;      // the pump reads a piece too when it has nothing to issue
  unsigned threads = 2;  // pool threads with the pump on the pool (the readers + 1; one reader fewer otherwise)
  bool trace = false;    // time the pump's idle spins
  std::vector<uint32_t> punit;          // per piece: its unit,
  std::vector<uint64_t> poff, plen;     // its offset in the unit's data, its length
  std::vector<size_t> upiece{0};        // unit u's pieces are [upiece[u], upiece[u + 1])
  std::vector<uint64_t> usend;          // per unit: the bytes to copy to the device
  size_t units() const { return usend.size(); }
  size_t pieces() const { return punit.size(); }
  void add_piece(uint64_t off, uint64_t len) {  // to the unit being built
    punit.push_back((uint32_t)units());
    poff.push_back(off);
    plen.push_back(len);
  }
  void end_unit(uint64_t send) {
    upiece.push_back(pieces());
    usend.push_back(send);
  }
};

struct Result {
  int err = 0;            // the first device error (the Dev's / callbacks' own code), 0 = none
  const char* what = "";  // ... and where: "setup", "copy", "sync", "issue"
  size_t copies = 0;      // trace counters: copies issued, time the pump spent in idle spins
  double pump_idle_us = 0;
};

inline void spin_pause() {
#if defined(__x86_64__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}

// The engine.  Dev (every operation returns 0 or an error code, all called on the pump thread
// except drain):
//   begin()                    once, before anything else
//   copy(k, at, bytes)         pinned[at, at + bytes) -> device[at, ...) on copy stream k (0 / 1)
//   join_copies()              copy stream 0 waits for what copy stream 1 holds
//   join_compute()             the compute stream waits for what copy stream 0 holds
//   record_done(slot)          record the slot's `done` on the compute stream
//   query_done(slot, ready)    has it completed?
//   drain()                    the calling thread waits for all three streams
// Callbacks:
//   read(p, at)     read piece p to pinned + at (any thread; the engine publishes the piece)
//   landed(u)       pump: every piece of unit u is in the pinned slot; may put a header copy on
//                   copy stream 0
//   issue(u)        pump: enqueue unit u's work on the compute stream
//   retired(u)      pump: unit u's `done` has completed (in unit order; then the slot is reused)
// The ordering rule lives here and not in the callbacks: for EVERY unit, whatever landed() and
// issue() decide to enqueue, `done` is recorded only after the compute stream has been made to
// wait for all of the unit's copies on both copy streams — a slot is never handed to the
// readers (or its results read) while a copy of the old unit is still in flight.
// A device error stops the pump and the readers; the run still drains the streams.
template <class Pool, class Dev, class Read, class Landed, class Issue, class Retired>
Result run(const Plan& pl, Pool& pool, Dev& dev, Read&& read, Landed&& landed, Issue&& issue,
           Retired&& retired) {
  const size_t nu = pl.units(), np = pl.pieces(), slots = (size_t)pl.slots;
  Result res;
  std::vector<std::atomic<uint8_t>> fin(np);  // piece p is in its slot (zero-initialised)
  std::atomic<bool> abort{false};
  std::atomic<size_t> next{0};   // the piece cursor
  std::atomic<size_t> freed{0};  // units [0, freed) have retired: their slots are free
  auto slot_free = [&](uint32_t u) { return u < freed.load(std::memory_order_acquire) + slots; };
  auto read_publish = [&](size_t p) {
    read(p, (size_t)(pl.punit[p] % slots) * pl.slot_bytes + pl.data_off + pl.poff[p]);
    fin[p].store(1, std::memory_order_release);
  };
  auto worker = [&]() {
    for (size_t p; !abort.load(std::memory_order_relaxed) && (p = next.fetch_add(1)) < np;) {
      while (!slot_free(pl.punit[p]) && !abort.load(std::memory_order_relaxed)) std::this_thread::yield();
      if (abort.load(std::memory_order_relaxed)) break;
      read_publish(p);
    }
  };
  auto pump = [&]() {
    size_t uc = 0, issued = 0, retired_n = 0, ready = 0;  // uc: the unit being filled
    uint64_t sent = 0;                                    // ... and its bytes copied so far
    auto stop = [&](int e, const char* what) { res.err = e; res.what = what; abort.store(true); };
    if (int e = dev.begin()) return stop(e, "setup");
    while (retired_n < nu) {
      if (retired_n < issued) {  // the oldest unit in flight
        bool is_done = false;
        if (int e = dev.query_done((int)(retired_n % slots), is_done)) return stop(e, "sync");
        if (is_done) {
          retired(retired_n);
          freed.store(++retired_n, std::memory_order_release);
          continue;
        }
      }
      bool progress = false;
      if (uc < nu) {
        const size_t at = (uc % slots) * pl.slot_bytes + pl.data_off;
        while (ready < pl.upiece[uc + 1] && fin[ready].load(std::memory_order_acquire)) ++ready;
        const bool complete = ready == pl.upiece[uc + 1];
        const uint64_t hi = complete ? pl.usend[uc] : std::min(pl.usend[uc], pl.poff[ready]);
        if (hi > sent && (hi - sent >= pl.copy_unit || complete)) {
          // (the kernels read to the 16-B round-up of a unit's data; slots have the room)
          const uint64_t hi16 = complete ? (hi + 15) & ~(uint64_t)15 : hi;
          if (int e = dev.copy(pl.copy_streams > 1 && (res.copies & 1), at + sent, hi16 - sent)) return stop(e, "copy");
          sent = hi16;
          ++res.copies;
          progress = true;
        }
        if (complete && sent >= pl.usend[uc]) {
          int e = pl.copy_streams > 1 ? dev.join_copies() : 0;
          if (!e) e = landed(uc);
          if (!e) e = dev.join_compute();
          if (!e) e = issue(uc);
          if (!e) e = dev.record_done((int)(uc % slots));
          if (e) return stop(e, "issue");
          ++issued;
          ++uc;
          sent = 0;
          continue;
        }
      }
      if (progress) continue;
      // nothing to copy, issue or retire: read a piece too, but only one whose slot is free
      // now (this thread is the one that frees slots)
      size_t p = next.load(std::memory_order_relaxed);
      if (pl.pump_reads && p < np && slot_free(pl.punit[p]) && next.compare_exchange_strong(p, p + 1)) {
        read_publish(p);
      } else {
        using clk = std::chrono::steady_clock;
        const clk::time_point t0 = pl.trace ? clk::now() : clk::time_point();
        spin_pause();
        if (pl.trace) res.pump_idle_us += std::chrono::duration<double, std::micro>(clk::now() - t0).count();
      }
    }
  };
  if (pl.pump_on_pool) {  // the first pool thread to arrive pumps, the calling thread only waits
    std::atomic<bool> pump_taken{false};
    const std::function<void()> pool_fn = [&]() {
      if (!pump_taken.exchange(true)) pump(); else worker();
    };
    pool.run2(std::max(2u, pl.threads), pool_fn, []() {});
  } else {
    pool.run2(std::max(1u, pl.threads - 1), worker, pump);
  }
  dev.drain();  // nothing in flight may still read the pinned slots or write results
  return res;
}

}  // namespace sdq
