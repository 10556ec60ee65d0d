// sd_content_tasks.h — the index arithmetic of the whole-content compare (content_compare.hip).
// Plain arithmetic, host and device, so a host program checks it
// (tests/native/content_tasks_test.cpp).
//
// The entry list holds the rows still to be compared, ordered by their pivot, so one pivot's rows
// are consecutive.  A window is CT_RUN_K consecutive entries; a task is one PIECE of a window: the
// byte range [p PIECE, (p + 1) PIECE) of every entry of the window that is that long.  Inside a
// task the entries of one pivot form a run, and the pivot's bytes are read once per run.  A piece
// is CT_PIECE_SLICES slices of 8 KiB, K1V's slice (sd_dup_runs.h): a wave's 64 lanes hold
// DUP_SLICE_QUADS 16-B quads of one slice.
#pragma once
#include <stdint.h>

#include "sd_dup_runs.h"

namespace sdcas {

constexpr uint32_t CT_SLICE_BYTES = DUP_SLICE_BYTES;  // what a wave holds in registers
// One task's share of one content.  Small enough that a 1 GiB pair is 16,384 tasks for the whole
// chip to share, large enough that taking a task (one atomic, one binary search) is paid once per
// 128 KiB of loads.  A choice, not a measurement.
constexpr uint32_t CT_PIECE_SLICES = 8;
constexpr uint32_t CT_PIECE_BYTES = CT_PIECE_SLICES * CT_SLICE_BYTES;  // 64 KiB
constexpr uint32_t CT_RUN_K = DUP_RUN_K;  // entries per task: K1V's, swept there
static_assert(CT_RUN_K >= 1 && CT_RUN_K <= 32, "a task's entries are the bits of one u32");
static_assert(CT_PIECE_BYTES % CT_SLICE_BYTES == 0, "a piece is whole slices");
constexpr uint64_t CT_MAX_LEN = 64ull << 30;  // the arena layout's bound (sd_cas_checksums_dev)
constexpr uint32_t CT_MAX_ROWS = 1u << 24;

// pieces of a content of len bytes: 0 for an empty one, 2^20 at 64 GiB
SD_RUNS_HD inline uint32_t ct_pieces(uint64_t len) {
  return (uint32_t)(len / CT_PIECE_BYTES) + (len % CT_PIECE_BYTES ? 1u : 0u);
}
// bytes of piece p < ct_pieces(len): PIECE, or the rest
SD_RUNS_HD inline uint32_t ct_piece_bytes(uint64_t len, uint32_t p) {
  const uint64_t left = len - (uint64_t)p * CT_PIECE_BYTES;
  return left < CT_PIECE_BYTES ? (uint32_t)left : CT_PIECE_BYTES;
}
// slices that hold `bytes` bytes of a piece (bytes <= PIECE)
SD_RUNS_HD inline uint32_t ct_slices(uint32_t bytes) {
  return bytes / CT_SLICE_BYTES + (bytes % CT_SLICE_BYTES ? 1u : 0u);
}
// Bytes of a content readable from byte `from` on, by the layout's rule (the 16-B round-up of its
// end), at most one slice: what a slice's loads are bounded to.  from < len.
SD_RUNS_HD inline uint32_t ct_slice_limit(uint64_t len, uint64_t from) {
  const uint64_t left = ((len + 15) & ~15ull) - from;
  return left < CT_SLICE_BYTES ? (uint32_t)left : CT_SLICE_BYTES;
}

// windows over a list of n_ent entries, as K1V's tasks over list C
SD_RUNS_HD inline uint32_t ct_window_count(uint32_t n_ent) {
  return n_ent / CT_RUN_K + (n_ent % CT_RUN_K ? 1u : 0u);
}
SD_RUNS_HD inline uint32_t ct_window_first(uint32_t w) { return w * CT_RUN_K; }
SD_RUNS_HD inline uint32_t ct_window_entries(uint32_t w, uint32_t n_ent) {
  const uint32_t left = n_ent - ct_window_first(w);
  return left < CT_RUN_K ? left : CT_RUN_K;
}
// a window's pieces: those of its longest entry (lens[e]: the length of entry e's content)
SD_RUNS_HD inline uint32_t ct_window_pieces(const uint64_t* lens, uint32_t w, uint32_t n_ent) {
  const uint32_t first = ct_window_first(w), m = ct_window_entries(w, n_ent);
  uint32_t most = 0;
  for (uint32_t e = 0; e < m; ++e) {
    const uint32_t p = ct_pieces(lens[first + e]);
    most = p > most ? p : most;
  }
  return most;
}
// the tasks of a list (the device takes this sum from a scan of ct_window_pieces)
inline uint64_t ct_task_count(const uint64_t* lens, uint32_t n_ent) {
  uint64_t total = 0;
  for (uint32_t w = 0; w < ct_window_count(n_ent); ++w) total += ct_window_pieces(lens, w, n_ent);
  return total;
}
// Task t < total -> its window and piece.  wstart[w] = the tasks of the windows before w (the
// exclusive scan, n_win entries, total < 2^32): the last window with wstart[w] <= t, skipping
// windows without a task.
struct CtTask { uint32_t window, piece; };
SD_RUNS_HD inline CtTask ct_task_of(const uint32_t* wstart, uint32_t n_win, uint32_t t) {
  uint32_t lo = 0, hi = n_win;  // wstart[lo] <= t, and wstart[hi] > t where hi < n_win
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (wstart[mid] <= t) lo = mid; else hi = mid;
  }
  return {lo, t - wstart[lo]};
}
// does entry e of a window take part in piece p?
SD_RUNS_HD inline bool ct_entry_in_piece(uint64_t len, uint32_t p) { return p < ct_pieces(len); }

// Entry e of a window starts a run when it is the window's first or its pivot differs from the
// entry's before it; the bit mask over a window's entries, and the run of entry e = the heads up
// to e (1-based), are what the kernel derives from it.
SD_RUNS_HD inline bool ct_run_starts(uint32_t e, uint32_t pivot, uint32_t pivot_before) {
  return e == 0 || pivot != pivot_before;
}
SD_RUNS_HD inline uint32_t ct_run_of(uint32_t heads, uint32_t e) {
  return (uint32_t)__builtin_popcount(heads & ((2u << e) - 1u));
}

// The last quad of a content of len > 0 bytes holds len % 16 content bytes (16 when that is 0);
// the others are padding that differs between equal files.  Word k (0..3) of the quad's mask:
SD_RUNS_HD inline uint32_t ct_last_quad_mask(uint64_t len, uint32_t k) {
  const uint32_t r = (uint32_t)(len & 15u);
  if (r == 0 || r >= 4 * k + 4) return 0xFFFFFFFFu;
  if (r <= 4 * k) return 0u;
  return (1u << (8 * (r - 4 * k))) - 1u;
}
// index in its slice of the last quad of a content whose last slice starts at byte `from`
SD_RUNS_HD inline uint32_t ct_last_quad(uint64_t len, uint64_t from) {
  return (uint32_t)((len - 1 - from) / 16);
}

}  // namespace sdcas
