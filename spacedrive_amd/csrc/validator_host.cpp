// validator_host.cpp — the validator's entry points of the C ABI (include/sd_hip_cas.h):
// sd_cas_checksum_dev / sd_cas_file_checksum (file_checksum, core/src/object/validation/
// hash.rs:9-25: hash.rs's read loop exactly, K3 on the device) and sd_cas_checksums_dev /
// sd_cas_file_checksums (the validator job over many files, validator_job.rs:107-172: K3b).
// Split out of sd_hip_cas.cpp; every digest comes from the HIP kernels.
#include <errno.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "sd_checksum.h"
#include "sd_group.h"
#include "sd_kernels.h"
#include "sd_mix.h"

using namespace sdcas;

#include "sd_debug.h"
#include "ctx_internal.h"

// short local names for the shared helpers
#define fail sd_fail
#define pick sd_pick
#define ensure sd_ensure
#define ensure_pinned sd_ensure_pinned

// A/B knobs of the file paths below (tools/build_variant.sh + tools/patch_define.py)
#ifndef SD_CK_PIECE_KB
#define SD_CK_PIECE_KB 1024
#endif
#ifndef SD_CK_COPY_MB
#define SD_CK_COPY_MB 8
#endif
#ifndef SD_CK_PUMP_READS  // the pump thread also reads pieces when it has nothing to issue
#define SD_CK_PUMP_READS 1
#endif
#ifndef SD_CK_PUMP_ON_POOL  // the pump on a pool thread (1) or on the calling thread (0)
#define SD_CK_PUMP_ON_POOL 1
#endif
#ifndef SD_CK_COPY_STREAMS  // copies alternate over this many streams (1 or 2)
#define SD_CK_COPY_STREAMS 2
#endif


extern "C" {

// ---- file_checksum --------------------------------------------------------------------

int sd_cas_checksum_dev(sd_cas_ctx* c, const void* d_data, uint64_t len, uint8_t out[32],
                        void* stream) {
  if (!c || !out) return SD_CAS_EINVAL;
  if ((len && !d_data) || ((uintptr_t)d_data & 15))
    return fail(c, SD_CAS_EINVAL, "checksum: bad data pointer");
  hipStream_t s = pick(c, stream);
  // up to 64 GiB: the batch chain with one buffer (K3b: its wide static grid and spread
  // block level ran 2.99 vs K3's 2.88 TB/s on the same 16 GiB, profiles/r02b_validator_batch.log)
  constexpr uint64_t BATCH_MAX = 64ull << 30;
  const bool batch = len <= BATCH_MAX;
  int rc = ensure(c, c->ws, batch ? checksum_batch_workspace_bytes(1, len) : checksum_workspace_bytes(len));
  if (rc) return rc;
  uint32_t* d_out = (uint32_t*)c->d_scalar;  // d_scalar[0..3]: digest; [4], [5]: offs, lens
  HIP_TRY(c, sd_ws_acquire(c, s));
  if (batch) {
    uint64_t* d_ol = c->d_scalar + 4;
    HIP_TRY(c, checksum_single_setup(d_ol, len, (uint32_t*)(c->d_scalar + 6), s));
    HIP_TRY(c, checksum_batch_device((const uint8_t*)d_data, len, d_ol, d_ol + 1, 1, d_out,
                                     (uint32_t*)(c->d_scalar + 6), c->ws.p, s));
  } else {
    HIP_TRY(c, checksum_device((const uint8_t*)d_data, len, 0, true, d_out, c->ws.p, s));
  }
  HIP_TRY(c, hipMemcpyAsync(out, d_out, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, sd_ws_release(c, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

// file_checksum(path) (validation/hash.rs:11-25): the reference issues one read() of
// BLOCK_LEN = 1 MiB per iteration into one hasher and stops at the FIRST read that returns
// fewer bytes — the end of a regular file on a local filesystem, but after the first short
// read on anything that returns short reads before its end (procfs seq_files give about one
// page per read, FIFOs and FUSE/network mounts whatever is ready).
// Two read modes, one result:
//   * pieces (regular files; round 6, file_checksum_pieces): the file is planned from st_size
//     as 64 MiB segments (a segment = one complete 65,536-chunk subtree) rotating over three
//     pinned + device slots; 1 MiB pieces from one queue are read by the pool (bound to the
//     GPU's NUMA node) while a pump on a pool thread copies every landed prefix to HBM over
//     two copy streams and hashes each complete segment (K3) into its subtree CV — the
//     validator job's piece queue (sd_cas_file_checksums) for one file.  A regular file whose
//     reads show it is not read like a local file — a short pread before the planned end,
//     data in the probe byte past st_size (it grew), an end before st_size — is redone
//     sequentially;
//   * sequential (everything else, and those redos): hash.rs's loop literally, 1 MiB read()s
//     from the start, stopping after the first short one, through two pinned segment buffers.
// The segment CVs are merged on the GPU (pair-and-promote, ROOT on the last parent); a file
// of one segment is hashed with ROOT inside the segment.
static int cv_capacity(sd_cas_ctx* c, DevBuf& cvb, size_t need_cvs, hipStream_t s) {
  if (need_cvs * 32 <= cvb.bytes) return SD_CAS_OK;
  DevBuf nb;
  const size_t want = std::max<size_t>(need_cvs * 2 * 32, 1 << 16);
  HIP_TRY(c, hipStreamSynchronize(s));
  if (hipMalloc(&nb.p, want) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SD_CAS_ENOMEM, "hipMalloc(%zu) failed", want);
  }
  nb.bytes = want;
  if (cvb.p) {
    HIP_TRY(c, hipMemcpy(nb.p, cvb.p, cvb.bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(c, hipFree(cvb.p));
  }
  cvb = nb;
  return SD_CAS_OK;
}

// The pieces mode of file_checksum (see above), over one or many files in ONE queue: every
// file is planned from its st_size (+ one probe byte) as 64 MiB segments; the segments of all
// files, in file order, rotate over three pinned + device slots, and their 1 MiB pieces are
// read by the pool while the pump copies landed prefixes (two copy streams), hashes each
// complete segment (K3 at its chunk offset, ROOT inside for a one-segment file) and, after a
// file's last segment, reduces its CVs into its digest — so a validator job's large files
// stream back to back with no per-file fill and drain.  Each piece opens its file by path on
// the pool thread that reads it (the pool's threads have private descriptor tables,
// HostPool::set_private_fds: a descriptor opened on the calling thread is not theirs).  Per
// file: digests[32 j], errs[j] = the errno of a failed open/read (0 otherwise), go_seq[j] = 1
// when its reads were irregular (a short pread before its planned end, data in the probe byte,
// an end before st_size): redo with hash.rs's sequential reads.  Returns SD_CAS_OK or a HIP /
// allocation error.
static int file_checksums_pieces(sd_cas_ctx* c, const char* const* paths, const uint64_t* sizes,
                                 size_t nf, uint8_t* digests, int* errs, uint8_t* go_seq) {
  constexpr uint64_t SEG = 64ull << 20;  // 65,536 chunks: a complete left subtree
  constexpr uint64_t PIECE = (uint64_t)SD_CK_PIECE_KB << 10;
  constexpr uint64_t COPY = (uint64_t)SD_CK_COPY_MB << 20;
  constexpr int SLOTS = 3;
  if (nf == 0) return SD_CAS_OK;
  struct Seg { uint32_t file; uint64_t k, len, want; };  // len: planned bytes, want: bytes to hash
  struct Piece { uint32_t seg; uint64_t off, len; };     // off: from the segment's start
  std::vector<Seg> segs;
  std::vector<uint64_t> nreal(nf), cvbase(nf + 1, 0);
  uint64_t maxtotal = 0, maxreal = 1;
  for (size_t j = 0; j < nf; j++) {
    const uint64_t total = sizes[j] + 1;  // + the probe byte: data there means the file grew
    const uint64_t nplan = (total + SEG - 1) / SEG;
    nreal[j] = std::max<uint64_t>(1, (sizes[j] + SEG - 1) / SEG);  // segments holding data
    cvbase[j + 1] = cvbase[j] + nreal[j];
    maxtotal = std::max(maxtotal, total);
    maxreal = std::max(maxreal, nreal[j]);
    for (uint64_t k = 0; k < nplan; k++)
      segs.push_back({(uint32_t)j, k, std::min(SEG, total - k * SEG),
                      k < nreal[j] ? std::min(SEG, sizes[j] - std::min(sizes[j], k * SEG)) : 0});
    errs[j] = 0;
    go_seq[j] = 0;
  }
  std::vector<Piece> pieces;
  std::vector<size_t> spiece{0};
  for (size_t g = 0; g < segs.size(); g++) {
    const uint64_t np = std::max<uint64_t>(1, segs[g].len / PIECE);
    for (uint64_t q = 0; q < np; q++)
      pieces.push_back({(uint32_t)g, q * PIECE, q + 1 < np ? PIECE : segs[g].len - q * PIECE});
    spiece.push_back(pieces.size());
  }
  const size_t ns = segs.size(), np = pieces.size();
  const uint64_t cap = std::min<uint64_t>(SEG, ((maxtotal + 4095) / 4096) * 4096);
  const size_t sb = up256(cap + 16);
  const uint64_t ncv = cvbase[nf];
  hipStream_t s = c->stream, cs = c->copy;
  int rc = SD_CAS_OK;
  if ((rc = ensure_pinned(c, SLOTS * sb)) || (rc = ensure(c, c->staging, SLOTS * sb))) return rc;
  if ((rc = ensure(c, c->ws, std::max({checksum_workspace_bytes(cap), checksum_workspace_bytes(1 << 20),
                                        2 * up256((maxreal + 255) / 256 * 32) + 512}))))
    return rc;
  if ((rc = cv_capacity(c, c->cvbuf, ncv + nf, s))) return rc;  // CVs, then the digests
  uint32_t* d_cv = (uint32_t*)c->cvbuf.p;
  uint32_t* d_dig = d_cv + 8 * ncv;
  hipEvent_t done[SLOTS] = {}, landed = nullptr;
  auto destroy_events = [&]() {
    for (int b = 0; b < SLOTS; b++)
      if (done[b]) (void)hipEventDestroy(done[b]);
    if (landed) (void)hipEventDestroy(landed);
  };
  for (int b = 0; b < SLOTS; b++)
    if (hipEventCreateWithFlags(&done[b], hipEventDisableTiming) != hipSuccess) {
      destroy_events();
      return fail(c, SD_CAS_EHIP, "file_checksum: event create");
    }
  if (hipEventCreateWithFlags(&landed, hipEventDisableTiming) != hipSuccess) {
    destroy_events();
    return fail(c, SD_CAS_EHIP, "file_checksum: event create");
  }
  std::unique_ptr<std::atomic<uint8_t>[]> fin(new std::atomic<uint8_t>[np]);
  std::unique_ptr<std::atomic<uint64_t>[]> sgot(new std::atomic<uint64_t>[ns]);
  std::unique_ptr<std::atomic<int>[]> ferr(new std::atomic<int>[nf]);
  std::unique_ptr<std::atomic<uint8_t>[]> firr(new std::atomic<uint8_t>[nf]);
  for (size_t p = 0; p < np; p++) fin[p].store(0, std::memory_order_relaxed);
  for (size_t g = 0; g < ns; g++) sgot[g].store(0);
  for (size_t j = 0; j < nf; j++) { ferr[j].store(0); firr[j].store(0); }
  std::atomic<bool> abort{false};
  std::atomic<size_t> next{0}, freed{0};
  auto slot_free = [&](uint32_t g) { return g < freed.load(std::memory_order_acquire) + SLOTS; };
  auto read_piece = [&](size_t p) {
    const Piece& pc = pieces[p];
    const Seg& sg = segs[pc.seg];
    const uint32_t j = sg.file;
    if (ferr[j].load(std::memory_order_relaxed) || firr[j].load(std::memory_order_relaxed)) return;
    char* dst = (char*)c->pinned + (size_t)(pc.seg % SLOTS) * sb + pc.off;
    const uint64_t foff = sg.k * SEG + pc.off;
    const int fd = open(paths[j], O_RDONLY | O_CLOEXEC);
    if (fd < 0) { ferr[j].store(errno); return; }
    uint64_t got = 0;
    bool was_short = false;
    while (got < pc.len) {
      ssize_t r = pread(fd, dst + got, pc.len - got, (off_t)(foff + got));
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) { ferr[j].store(errno); break; }
      if (r == 0) break;  // EOF
      if (was_short) firr[j].store(1);  // data after a short read
      if ((uint64_t)r < pc.len - got) was_short = true;
      got += (uint64_t)r;
    }
    close(fd);
    if (got < pc.len && foff + pc.len < sizes[j] + 1) firr[j].store(1);  // ended before the planned end
    sgot[pc.seg].fetch_add(got);
  };
  auto worker = [&]() {
    for (size_t p; !abort.load(std::memory_order_relaxed) && (p = next.fetch_add(1)) < np;) {
      while (!slot_free(pieces[p].seg) && !abort.load(std::memory_order_relaxed)) std::this_thread::yield();
      if (abort.load(std::memory_order_relaxed)) break;
      read_piece(p);
      fin[p].store(1, std::memory_order_release);
    }
  };
  std::vector<uint8_t> fok(nf, 1);  // (pump only) every segment of the file so far as planned
  // the pump: copies landed prefixes, hashes complete segments and finished files, frees slots
  auto pump = [&]() {
    size_t kc = 0, issued = 0, retired = 0, ready = 0, ncopies = 0;
    uint64_t sent = 0;
    auto hipfail = [&](hipError_t e, const char* what) {
      rc = fail(c, SD_CAS_EHIP, "file_checksum %s: %s", what, hipGetErrorString(e));
      abort.store(true);
    };
    if (hipError_t e = hipSetDevice(c->device); e != hipSuccess) { hipfail(e, "setup"); return; }
    if (hipError_t e = sd_ws_acquire(c, s); e != hipSuccess) { hipfail(e, "setup"); return; }
    while (retired < ns && rc == SD_CAS_OK) {
      if (retired < issued) {
        const hipError_t q = hipEventQuery(done[retired % SLOTS]);
        if (q == hipSuccess) {
          freed.store(++retired, std::memory_order_release);
          continue;
        }
        if (q != hipErrorNotReady) { hipfail(q, "segment sync"); break; }
      }
      bool progress = false;
      if (kc < ns) {
        const Seg& sg = segs[kc];
        const size_t b = kc % SLOTS;
        char* pin = (char*)c->pinned + b * sb;
        char* dev = (char*)c->staging.p + b * sb;
        while (ready < spiece[kc + 1] && fin[ready].load(std::memory_order_acquire)) ++ready;
        const bool complete = ready == spiece[kc + 1];
        const uint64_t hi = complete ? sg.want : std::min(sg.want, pieces[ready].off);
        if (hi > sent && (hi - sent >= COPY || complete)) {
          hipStream_t xs = (SD_CK_COPY_STREAMS > 1 && (ncopies & 1)) ? c->copy2 : cs;
          const uint64_t hi16 = complete ? up16(hi) : hi;  // (K3 reads to the 16-B round-up)
          const hipError_t e = hipMemcpyAsync(dev + sent, pin + sent, hi16 - sent, hipMemcpyHostToDevice, xs);
          if (e != hipSuccess) { hipfail(e, "copy"); break; }
          sent = hi16;
          ++ncopies;
          progress = true;
        }
        if (complete && sent >= sg.want) {
          const uint32_t j = sg.file;
          const bool last = sg.k + 1 == (sizes[j] + SEG) / SEG;  // (sizes[j] + 1 + SEG - 1) / SEG segments
          // the segment must hold exactly its planned bytes (the probe byte none)
          if (ferr[j].load() || firr[j].load() || sgot[kc].load() != (last ? sg.len - 1 : sg.len)) fok[j] = 0;
          hipError_t e = hipSuccess;
          if (fok[j] && sg.k < nreal[j]) {
            if (SD_CK_COPY_STREAMS > 1) {
              e = hipEventRecord(landed, c->copy2);
              if (e == hipSuccess) e = hipStreamWaitEvent(s, landed, 0);
            }
            if (e == hipSuccess) e = hipEventRecord(landed, cs);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, landed, 0);
            if (e == hipSuccess)
              e = checksum_device((const uint8_t*)dev, sg.want, (sg.k * SEG) >> 10, nreal[j] == 1,
                                  d_cv + 8 * (cvbase[j] + sg.k), c->ws.p, s);
          }
          if (e == hipSuccess && fok[j] && last)  // the file's digest
            e = nreal[j] == 1 ? hipMemcpyAsync(d_dig + 8 * j, d_cv + 8 * cvbase[j], 32, hipMemcpyDeviceToDevice, s)
                              : reduce_cvs_device(d_cv + 8 * cvbase[j], nreal[j], d_dig + 8 * j, c->ws.p, s);
          if (e == hipSuccess) e = hipEventRecord(done[b], s);
          if (e != hipSuccess) { hipfail(e, "segment"); break; }
          ++issued;
          ++kc;
          sent = 0;
          continue;
        }
      }
      if (progress) continue;
      size_t p = next.load(std::memory_order_relaxed);
      if (SD_CK_PUMP_READS && p < np && slot_free(pieces[p].seg) && next.compare_exchange_strong(p, p + 1)) {
        read_piece(p);
        fin[p].store(1, std::memory_order_release);
      } else {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
      }
    }
  };
  std::atomic<bool> pump_taken{false};
  const std::function<void()> pool_fn = [&]() {
    if (!pump_taken.exchange(true)) pump(); else worker();
  };
  c->pool.run2(std::max(2u, std::min(16u, (unsigned)std::min<size_t>(np + 1, 16))), pool_fn, []() {});
  if (rc == SD_CAS_OK) {
    hipError_t e = hipMemcpyAsync(digests, d_dig, nf * 32, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(c, SD_CAS_EHIP, "checksum digests: %s", hipGetErrorString(e));
  }
  (void)sd_ws_release(c, s);
  // nothing in flight may still read the pinned slots or write the CVs
  (void)hipStreamSynchronize(cs);
  (void)hipStreamSynchronize(c->copy2);
  (void)hipStreamSynchronize(s);
  destroy_events();
  for (size_t j = 0; j < nf; j++) {
    errs[j] = ferr[j].load();
    go_seq[j] = !errs[j] && !fok[j];
  }
  return rc;
}

// One file (sd_cas_file_checksum): the queue above over its path (the readers open it
// themselves; a file replaced since the caller's open reads irregularly or not — the same
// race the batch path's per-piece opens have, and hash.rs's reads have no defined answer to).
static int file_checksum_pieces(sd_cas_ctx* c, uint64_t st_size, const char* path,
                                uint8_t digest[32], int* err_no, bool* go_seq) {
  int err = 0;
  uint8_t seq = 0;
  int rc = file_checksums_pieces(c, &path, &st_size, 1, digest, &err, &seq);
  *go_seq = rc == SD_CAS_OK && seq;
  if (rc == SD_CAS_OK && err) {
    if (err_no) *err_no = err;
    rc = fail(c, SD_CAS_EIO, "read(%s): %s", path, strerror(err));
  }
  return rc;
}

// The sequential mode of file_checksum: hash.rs:15-21 literally — 1 MiB read()s in order,
// stop after the first short one — through two pinned 64 MiB segment buffers (segment k is
// hashed on the GPU while the next one is read).
static int file_checksum_seq(sd_cas_ctx* c, int fd, const char* path, uint8_t digest[32], int* err_no) {
  constexpr uint64_t SEG = 64ull << 20;
  constexpr uint64_t BLOCK_LEN = 1ull << 20;  // hash.rs:9
  static_assert(SEG % BLOCK_LEN == 0, "a segment holds whole hash.rs reads");
  hipStream_t s = c->stream;
  const size_t sb = up256(SEG + 16);
  int rc = SD_CAS_OK;
  if ((rc = ensure_pinned(c, 2 * sb)) || (rc = ensure(c, c->staging, 2 * sb))) return rc;
  if ((rc = ensure(c, c->ws, checksum_workspace_bytes(SEG)))) return rc;
  hipEvent_t done[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; i++)
    if (hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess) {
      for (int k = 0; k < i; k++) (void)hipEventDestroy(done[k]);
      return fail(c, SD_CAS_EHIP, "file_checksum: event create");
    }
  char* pin[2] = {(char*)c->pinned, (char*)c->pinned + sb};
  char* dev[2] = {(char*)c->staging.p, (char*)c->staging.p + sb};
  bool stopped = false;  // the first short read has happened
  auto read_seg = [&](char* dst) -> int64_t {
    if (stopped) return 0;
    uint64_t got = 0;
    while (got < SEG) {
      ssize_t r = read(fd, dst + got, BLOCK_LEN);
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) return -(int64_t)errno;
      got += (uint64_t)r;
      if ((uint64_t)r != BLOCK_LEN) { stopped = true; break; }
    }
    return (int64_t)got;
  };
  // segment k is dispatched once it is known whether it is the only one (k == 0 waits for
  // segment 1's read); ROOT sits inside it only then
  auto dispatch = [&](uint64_t sgi, uint64_t len, bool only) -> int {
    const int b = (int)(sgi & 1);
    int r2 = cv_capacity(c, c->cvbuf, sgi + 1, s);
    if (r2) return r2;
    hipError_t e = hipMemcpyAsync(dev[b], pin[b], up16(len), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = checksum_device((const uint8_t*)dev[b], len, (sgi * SEG) >> 10, only,
                          (uint32_t*)c->cvbuf.p + 8 * sgi, c->ws.p, s);
    if (e == hipSuccess) e = hipEventRecord(done[b], s);
    if (e != hipSuccess) return fail(c, SD_CAS_EHIP, "checksum segment: %s", hipGetErrorString(e));
    return SD_CAS_OK;
  };
  auto io_fail = [&](int64_t neg) {
    if (err_no) *err_no = (int)-neg;
    return fail(c, SD_CAS_EIO, "read(%s): %s", path, strerror((int)-neg));
  };
  if (hipError_t e = sd_ws_acquire(c, s); e != hipSuccess) {
    (void)hipEventDestroy(done[0]);
    (void)hipEventDestroy(done[1]);
    return fail(c, SD_CAS_EHIP, "file_checksum: %s", hipGetErrorString(e));
  }
  uint64_t nseg = 1;
  const int64_t len0 = read_seg(pin[0]);
  if (len0 < 0) {
    rc = io_fail(len0);
  } else if ((uint64_t)len0 < SEG) {
    rc = dispatch(0, (uint64_t)len0, true);
  } else {  // a full first segment: more may follow
    for (uint64_t sgi = 1;; sgi++) {
      const int b = (int)(sgi & 1);
      if (sgi >= 2 && hipEventSynchronize(done[b]) != hipSuccess) { rc = fail(c, SD_CAS_EHIP, "checksum: segment sync"); break; }
      const int64_t ln = read_seg(pin[b]);
      if (ln < 0) { rc = io_fail(ln); break; }
      if (sgi == 1 && (rc = dispatch(0, (uint64_t)len0, ln == 0))) break;  // segment 0: the only one?
      if (ln == 0) { nseg = sgi; break; }
      if ((rc = dispatch(sgi, (uint64_t)ln, false))) break;
      if ((uint64_t)ln < SEG) { nseg = sgi + 1; break; }
    }
  }
  if (rc == SD_CAS_OK) {
    uint32_t* d_out = (uint32_t*)c->d_scalar;
    hipError_t e = hipSuccess;
    // reduce_cvs_device ping-pongs ceil(nseg / 256) CVs per level through ws
    if (nseg > 1) rc = ensure(c, c->ws, 2 * up256((nseg + 255) / 256 * 32) + 512);
    if (rc == SD_CAS_OK) {
      if (nseg == 1) e = hipMemcpyAsync(d_out, c->cvbuf.p, 32, hipMemcpyDeviceToDevice, s);
      else e = reduce_cvs_device((uint32_t*)c->cvbuf.p, nseg, d_out, c->ws.p, s);
      if (e == hipSuccess) e = hipMemcpyAsync(digest, d_out, 32, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = fail(c, SD_CAS_EHIP, "checksum reduce: %s", hipGetErrorString(e));
    }
  }
  (void)hipStreamSynchronize(s);  // no segment copy may still read the pinned buffers
  (void)sd_ws_release(c, s);
  (void)hipEventDestroy(done[0]);
  (void)hipEventDestroy(done[1]);
  return rc;
}

int sd_cas_file_checksum(sd_cas_ctx* c, const char* path, char out_hex[65], int* err_no) {
  if (!c || !path || !out_hex) return SD_CAS_EINVAL;
  if (err_no) *err_no = 0;
  HIP_TRY(c, hipSetDevice(c->device));
  int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    if (err_no) *err_no = errno;
    return fail(c, SD_CAS_EIO, "open(%s): %s", path, strerror(errno));
  }
  struct stat st;
  if (fstat(fd, &st) != 0) {
    if (err_no) *err_no = errno;
    close(fd);
    return fail(c, SD_CAS_EIO, "fstat(%s): %s", path, strerror(errno));
  }
  uint8_t digest[32];
  int rc = SD_CAS_OK;
  bool seq = !S_ISREG(st.st_mode);
  if (!seq) {  // a regular file: the pieces mode, redone sequentially if it reads irregularly
    rc = file_checksum_pieces(c, (uint64_t)st.st_size, path, digest, err_no, &seq);
    if (rc == SD_CAS_OK && seq && lseek(fd, 0, SEEK_SET) != 0) {
      if (err_no) *err_no = errno;
      rc = fail(c, SD_CAS_EIO, "lseek(%s): %s", path, strerror(errno));
    }
  }
  if (rc == SD_CAS_OK && seq) rc = file_checksum_seq(c, fd, path, digest, err_no);
  close(fd);
  if (rc) return rc;
  static const char* hx = "0123456789abcdef";
  for (int i = 0; i < 32; i++) { out_hex[2 * i] = hx[digest[i] >> 4]; out_hex[2 * i + 1] = hx[digest[i] & 15]; }
  out_hex[64] = 0;
  return SD_CAS_OK;
}

// ---- the validator job over many files -----------------------------------------------

int sd_cas_checksums_dev(sd_cas_ctx* c, const void* d_arena, uint64_t arena_bytes,
                         const uint64_t* d_offs, const uint64_t* d_lens, size_t n, uint8_t* d_out,
                         void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!d_arena || !d_offs || !d_lens || !d_out || ((uintptr_t)d_arena & 15) ||
      ((uintptr_t)d_out & 3) || n > (1u << 24))
    return fail(c, SD_CAS_EINVAL, "checksums: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick(c, stream);
  int rc = ensure(c, c->ws, checksum_batch_workspace_bytes(n, arena_bytes));
  if (rc) return rc;
  uint32_t* d_bad = (uint32_t*)(c->d_scalar + 6);
  uint32_t bad = 0;
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, s));
  HIP_TRY(c, checksum_batch_device((const uint8_t*)d_arena, arena_bytes, d_offs, d_lens, n,
                                   (uint32_t*)d_out, d_bad, c->ws.p, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, sd_ws_release(c, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad)
    return fail(c, SD_CAS_EINVAL, "checksums: %s",
                (bad & 1) ? "a buffer is longer than 64 GiB"
                          : (bad & 4) ? "a buffer is misaligned or extends past arena_bytes"
                                      : "the buffers' subtrees exceed arena_bytes' bound (overlapping buffers?)");
  return SD_CAS_OK;
}

// ---- cas_ids from whole contents in place (cas_inplace.hip) -----------------------------

// After inplace_classify on s: whole files through the packed dispatcher over classify's u32
// lengths (sampled files count as empty there; their keys are rewritten next), then K1P over
// the sampled list.  c->inplace and c->ws are sized and ws is acquired by the caller.
static hipError_t contents_hash_classified(sd_cas_ctx* c, const uint8_t* arena, const uint64_t* offs,
                                           const uint64_t* lens, size_t n, size_t n_sampled,
                                           uint64_t* keys, hipStream_t s) {
  void* iw = c->inplace.p;
  hipError_t e = hipSuccess;
  if (n_sampled < n) e = sd_dispatch_packed(c, arena, offs, inplace_lens32(iw), lens, n, keys, s);
  if (e == hipSuccess)
    e = hash_inplace_sampled(arena, offs, lens, inplace_sampled_idx(iw, n), n_sampled, keys, s);
  return e;
}

// Both device entry points: classify, the bounds verdict (one read-back; a batch that breaks
// the bounds is not read and writes nothing), then the cas hash and, with d_digests, the
// checksum batch chain over the same buffers.
static int contents_dev(sd_cas_ctx* c, const char* what, const void* d_arena, uint64_t arena_bytes,
                        const uint64_t* d_offs, const uint64_t* d_lens, size_t n, uint64_t* d_keys,
                        uint8_t* d_digests, bool digests, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!d_arena || !d_offs || !d_lens || !d_keys || (digests && !d_digests) ||
      ((uintptr_t)d_arena & 15) || ((uintptr_t)d_keys & 7) || ((uintptr_t)d_digests & 3) ||
      n > (1u << 24))
    return fail(c, SD_CAS_EINVAL, "%s: bad arguments", what);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick(c, stream);
  int rc = ensure(c, c->inplace, inplace_workspace_bytes(n));
  if (rc) return rc;
  rc = ensure(c, c->ws, std::max(sd_packed_workspace_bytes(c, n),
                                 digests ? checksum_batch_workspace_bytes(n, arena_bytes) : (size_t)0));
  if (rc) return rc;
  uint32_t verdict[2] = {0, 0};  // bad flags, sampled files
  HIP_TRY(c, sd_ws_acquire(c, s));
  HIP_TRY(c, inplace_classify(arena_bytes, d_offs, d_lens, n, c->inplace.p, s));
  HIP_TRY(c, hipMemcpyAsync(verdict, inplace_counters(c->inplace.p), 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (verdict[0]) {
    (void)sd_ws_release(c, s);
    return fail(c, SD_CAS_EINVAL, "%s: %s", what,
                (verdict[0] & 1) ? "a buffer is longer than 64 GiB"
                                 : "a buffer is misaligned or extends past arena_bytes");
  }
  HIP_TRY(c, contents_hash_classified(c, (const uint8_t*)d_arena, d_offs, d_lens, n, verdict[1],
                                      d_keys, s));
  if (!digests) {
    HIP_TRY(c, sd_ws_release(c, s));
    return SD_CAS_OK;
  }
  // the chain's own flag can only still report its CV list's bound (overlapping buffers)
  uint32_t* d_bad = (uint32_t*)(c->d_scalar + 6);
  uint32_t bad = 0;
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, s));
  HIP_TRY(c, checksum_batch_device((const uint8_t*)d_arena, arena_bytes, d_offs, d_lens, n,
                                   (uint32_t*)d_digests, d_bad, c->ws.p, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, sd_ws_release(c, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad)
    return fail(c, SD_CAS_EINVAL, "%s: the buffers' subtrees exceed arena_bytes' bound (overlapping buffers?)", what);
  return SD_CAS_OK;
}

int sd_cas_hash_contents_dev(sd_cas_ctx* c, const void* d_arena, uint64_t arena_bytes,
                             const uint64_t* d_offs, const uint64_t* d_lens, size_t n,
                             uint64_t* d_keys, void* stream) {
  return contents_dev(c, "hash_contents", d_arena, arena_bytes, d_offs, d_lens, n, d_keys, nullptr,
                      false, stream);
}

int sd_cas_identify_validate_dev(sd_cas_ctx* c, const void* d_arena, uint64_t arena_bytes,
                                 const uint64_t* d_offs, const uint64_t* d_lens, size_t n,
                                 uint64_t* d_keys, uint8_t* d_digests, void* stream) {
  return contents_dev(c, "identify_validate", d_arena, arena_bytes, d_offs, d_lens, n, d_keys,
                      d_digests, true, stream);
}

// file_checksum over many paths.  The batch files are laid out in windows of up to CK_WIN
// bytes / CK_WIN_FILES files in index order (one slot of up128(st_size + 1) per file: the
// spare byte shows EOF, so a file that grew since stat fills its slot and is redone by the
// streaming path), windows rotating over CK_SLOTS pinned + device slots.  Round 6 (VERDICT r5
// #1): the files are read as PIECES of <= CK_PIECE bytes (1 MiB reads into the pinned slot run
// faster host-side than one whole-file pread, profiles/r05/official_c/probe_pread.log) taken
// from ONE queue over the whole job by up to 15 pool threads, while a 16th pool thread pumps:
// every finished prefix of the current window (>= CK_COPY bytes) goes to HBM as it lands,
// alternating over two copy streams (one stream moves 8 MiB pieces at ~53 GB/s, two at ~57,
// profiles/r06/validator/h2d_sizes.log), a finished window gets its header, K3b and its
// digests back on the compute stream, and a window whose digests are back frees its slot for
// the readers (the pump reads pieces too when it has nothing to issue).  The pool's threads
// sit on the GPU's NUMA node (sd_cas_ctx_create).  Warm 2,000-file tmpfs set: 53.5-54.7 GB/s
// vs 51.6-52.4 with one copy stream and 49.9-53.0 with the pump on the calling thread
// (profiles/r06/validator/s7_*).  Pinned and device slot layout: offs | lens | digests | data.
//
// With out_keys (sd_cas_identify_validate_paths) the same read also gives each row's cas part
// of FileMetadata::new, exactly as sd_cas_file_metadata_from_paths decides it: the stat pass
// fills out_sizes and cas_status (-errno, -EISDIR, NO_CAS for length 0), and where a window
// launches K3b it launches the contents hash (cas_inplace.hip) on the same offs / lens, thread
// and stream; the slot header then holds 8 more bytes per file, the keys, which come back with
// the digests.  A window member decided as hashed takes both results from the window; every
// other row that still wants a key gets it from the path gather at the end, with the stat
// pass's sizes (one stat per path decides the row).  out_keys == NULL: nothing of this runs.
static int file_checksums_impl(sd_cas_ctx* c, const char* const* paths, size_t n, char* out_hex,
                               int32_t* status, uint64_t* out_keys, int32_t* cas_status,
                               uint64_t* out_sizes) {
  HIP_TRY(c, hipSetDevice(c->device));
  constexpr uint64_t CK_WIN = 128ull << 20;  // data bytes per window
  constexpr uint64_t CK_BIG = CK_WIN / 2;    // larger files stream on their own (64 MiB segments)
  constexpr size_t CK_WIN_FILES = 32768;
  constexpr uint64_t CK_PIECE = (uint64_t)SD_CK_PIECE_KB << 10;  // read unit (a file's last piece takes the rest)
  constexpr uint64_t CK_COPY = (uint64_t)SD_CK_COPY_MB << 20;     // H2D unit of a window's landed prefix
  constexpr int CK_SLOTS = 3;
  const size_t HDR = CK_WIN_FILES * (8 + 8 + 32 + (out_keys ? 8 : 0));
  const size_t SLOT = HDR + CK_WIN + 256;
  enum : uint8_t { K_BATCH = 0, K_STREAM = 1, K_ERROR = 2 };
  SdTrace tr(c->trace, "file_checksums", n);
  std::vector<uint64_t> fsize(n, 0);
  std::vector<uint8_t> kind(n, K_BATCH), big(n, 0);  // big: a regular file over CK_BIG
  for (size_t i = 0; i < n; i++) { status[i] = 0; out_hex[65 * i] = 0; }
  std::vector<uint8_t> khave(out_keys ? n : 0, 0);  // the row's key comes from its window
  if (out_keys)
    for (size_t i = 0; i < n; i++) { out_keys[i] = 0; cas_status[i] = 0; out_sizes[i] = 0; }
  {  // stat pass
    std::atomic<size_t> next{0};
    c->pool.run(std::max(1u, std::min(16u, (unsigned)((n + 63) / 64))), [&]() {
      for (size_t i; (i = next.fetch_add(1)) < n;) {
        struct stat st;
        if (stat(paths[i], &st) != 0) {
          status[i] = -errno;
          kind[i] = K_ERROR;
          if (out_keys) cas_status[i] = -errno;
          continue;
        }
        fsize[i] = (uint64_t)st.st_size;
        if (out_keys) {  // FileMetadata::new's decision (file_identifier/mod.rs:63-86)
          if (S_ISDIR(st.st_mode)) cas_status[i] = -EISDIR;
          else if ((out_sizes[i] = fsize[i]) == 0) cas_status[i] = SD_CAS_STATUS_NO_CAS;
        }
        // not a regular file (FIFO, device, ...): hash.rs's sequential reads, streamed
        if (fsize[i] > CK_BIG || !S_ISREG(st.st_mode)) kind[i] = K_STREAM;
        big[i] = fsize[i] > CK_BIG && S_ISREG(st.st_mode);
      }
    });
  }
  tr.mark("stat");
  // members (batch files) in index order, grouped into windows; each member's slot offset
  // and capacity; its pieces in slot byte order (so a prefix of pieces is a prefix of bytes)
  std::vector<size_t> mfile, wmem{0}, wpiece{0};
  std::vector<uint64_t> moff, mcap, wbytes;
  struct Piece { uint32_t mem; uint32_t win; uint64_t off, len; };
  std::vector<Piece> pieces;
  {
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; i++) {
      if (kind[i] != K_BATCH) continue;
      const uint64_t need = up128(fsize[i] + 1);
      const size_t files = mfile.size() - wmem.back();
      if (files && (bytes + need > CK_WIN || files == CK_WIN_FILES)) {
        wbytes.push_back(bytes);
        wmem.push_back(mfile.size());
        wpiece.push_back(pieces.size());
        bytes = 0;
      }
      const uint32_t k = (uint32_t)mfile.size();
      mfile.push_back(i);
      moff.push_back(bytes);
      mcap.push_back(need);
      const uint64_t np = std::max<uint64_t>(1, need / CK_PIECE);
      for (uint64_t j = 0; j < np; j++)
        pieces.push_back({k, (uint32_t)(wmem.size() - 1), j * CK_PIECE,
                          j + 1 < np ? CK_PIECE : need - j * CK_PIECE});
      bytes += need;
    }
    if (mfile.size() > wmem.back()) {
      wbytes.push_back(bytes);
      wmem.push_back(mfile.size());
      wpiece.push_back(pieces.size());
    }
  }
  const size_t nw = wbytes.size(), nm = mfile.size(), np = pieces.size();
  int rc = SD_CAS_OK;
  if (nw) {
    if ((rc = ensure_pinned(c, CK_SLOTS * SLOT))) return rc;
    if ((rc = ensure(c, c->staging, CK_SLOTS * SLOT))) return rc;
    size_t wsb = checksum_batch_workspace_bytes(CK_WIN_FILES, CK_WIN);
    if (out_keys) {
      for (size_t w = 0; w < nw; w++) wsb = std::max(wsb, sd_packed_workspace_bytes(c, wmem[w + 1] - wmem[w]));
      if ((rc = ensure(c, c->inplace, inplace_workspace_bytes(CK_WIN_FILES)))) return rc;
    }
    if ((rc = ensure(c, c->ws, wsb))) return rc;
  }
  hipStream_t s = c->stream, cs = c->copy;
  hipEvent_t done[CK_SLOTS] = {}, landed = nullptr;
  auto destroy_events = [&]() {
    for (int b = 0; b < CK_SLOTS; b++)
      if (done[b]) (void)hipEventDestroy(done[b]);
    if (landed) (void)hipEventDestroy(landed);
  };
  for (int b = 0; b < CK_SLOTS && nw; b++)
    if (hipEventCreateWithFlags(&done[b], hipEventDisableTiming) != hipSuccess) {
      destroy_events();
      return fail(c, SD_CAS_EHIP, "file_checksums: event create");
    }
  if (nw && hipEventCreateWithFlags(&landed, hipEventDisableTiming) != hipSuccess) {
    destroy_events();
    return fail(c, SD_CAS_EHIP, "file_checksums: event create");
  }
  // per member: bytes read, read error, and a read that a local regular file never gives (a
  // short piece before the file's last, or data after a short read)
  std::unique_ptr<std::atomic<uint64_t>[]> mgot(new std::atomic<uint64_t>[nm]);
  std::unique_ptr<std::atomic<int>[]> merr(new std::atomic<int>[nm]);
  std::unique_ptr<std::atomic<uint8_t>[]> mirr(new std::atomic<uint8_t>[nm]);
  std::unique_ptr<std::atomic<uint8_t>[]> fin(new std::atomic<uint8_t>[np]);
  for (size_t k = 0; k < nm; k++) { mgot[k].store(0); merr[k].store(0); mirr[k].store(0); }
  for (size_t p = 0; p < np; p++) fin[p].store(0, std::memory_order_relaxed);
  std::atomic<size_t> next{0};
  std::atomic<size_t> freed{0};  // windows [0, freed) have their digests back: their slots are free
  std::atomic<bool> abort{false};
  auto slot_free = [&](uint32_t w) { return w < freed.load(std::memory_order_acquire) + CK_SLOTS; };
  auto read_piece = [&](size_t p) {
    const Piece& pc = pieces[p];
    const size_t i = mfile[pc.mem];
    char* dst = (char*)c->pinned + (size_t)(pc.win % CK_SLOTS) * SLOT + HDR + moff[pc.mem] + pc.off;
    int fd = open(paths[i], O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
      merr[pc.mem].store(errno);
      return;
    }
    uint64_t got = 0;
    bool was_short = false;
    while (got < pc.len) {
      ssize_t r = pread(fd, dst + got, pc.len - got, (off_t)(pc.off + got));
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) { merr[pc.mem].store(errno); break; }
      if (r == 0) break;  // EOF
      if (was_short) mirr[pc.mem].store(1);  // data after a short read: not a local file
      if ((uint64_t)r < pc.len - got) was_short = true;
      got += (uint64_t)r;
    }
    close(fd);
    if (got < pc.len && pc.off + pc.len < mcap[pc.mem]) mirr[pc.mem].store(1);  // ended before its last piece
    mgot[pc.mem].fetch_add(got);
  };
  auto spin = []() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  };
  auto worker = [&]() {
    for (size_t p; !abort.load(std::memory_order_relaxed) && (p = next.fetch_add(1)) < np;) {
      // a piece of window w waits for window w - CK_SLOTS to free the slot
      while (!slot_free(pieces[p].win) && !abort.load(std::memory_order_relaxed)) std::this_thread::yield();
      if (abort.load(std::memory_order_relaxed)) break;
      read_piece(p);
      fin[p].store(1, std::memory_order_release);
    }
  };
  static const char* hx = "0123456789abcdef";
  auto emit = [&](size_t w) {  // window w's digests are back in its pinned slot: -> hex
    const uint8_t* dg = (const uint8_t*)c->pinned + (size_t)(w % CK_SLOTS) * SLOT + CK_WIN_FILES * 16;
    for (size_t k = wmem[w]; k < wmem[w + 1]; k++) {
      const uint8_t* d = dg + 32 * (k - wmem[w]);
      char* o = out_hex + 65 * mfile[k];
      for (int j = 0; j < 32; j++) { o[2 * j] = hx[d[j] >> 4]; o[2 * j + 1] = hx[d[j] & 15]; }
      o[64] = 0;
    }
    if (!out_keys) return;
    // the window's keys follow its digests; a member whose key is not the window's (khave),
    // or that has no cas_id, keeps key 0
    const size_t m = wmem[w + 1] - wmem[w];
    const uint8_t* kp = dg + 32 * m;
    for (size_t k = wmem[w]; k < wmem[w + 1]; k++) {
      const size_t i = mfile[k];
      if (khave[i] && cas_status[i] == 0) memcpy(&out_keys[i], kp + 8 * (k - wmem[w]), 8);
    }
  };
  uint32_t* d_bad = (uint32_t*)(c->d_scalar + 6);
  size_t ncopies = 0;
  double stall_us = 0;
  // the pump (this thread): copies, window launches, retirement; reads a piece when idle
  auto pump = [&]() {
    size_t wc = 0, issued = 0, retired = 0, ready = 0;
    uint64_t sent = 0;
    auto hipfail = [&](hipError_t e, const char* what) {
      rc = fail(c, SD_CAS_EHIP, "file_checksums %s: %s", what, hipGetErrorString(e));
      abort.store(true);
    };
    {
      hipError_t e = hipSetDevice(c->device);  // (HIP's current device is per thread)
      if (e == hipSuccess) e = sd_ws_acquire(c, s);
      if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 4, s);
      if (e != hipSuccess) { hipfail(e, "setup"); return; }
    }
    while (retired < nw && rc == SD_CAS_OK) {
      bool progress = false;
      if (retired < issued) {  // the oldest window in flight: digests back?
        const hipError_t q = hipEventQuery(done[retired % CK_SLOTS]);
        if (q == hipSuccess) {
          emit(retired);
          freed.store(++retired, std::memory_order_release);
          continue;
        }
        if (q != hipErrorNotReady) { hipfail(q, "window sync"); break; }
      }
      if (wc < nw) {
        const size_t b = wc % CK_SLOTS;
        char* pin = (char*)c->pinned + b * SLOT;
        char* dev = (char*)c->staging.p + b * SLOT;
        while (ready < wpiece[wc + 1] && fin[ready].load(std::memory_order_acquire)) ++ready;
        const bool complete = ready == wpiece[wc + 1];
        const uint64_t hi = complete ? wbytes[wc] : moff[pieces[ready].mem] + pieces[ready].off;
        if (hi > sent && (hi - sent >= CK_COPY || complete)) {
          hipStream_t xs = (SD_CK_COPY_STREAMS > 1 && (ncopies & 1)) ? c->copy2 : cs;
          const hipError_t e = hipMemcpyAsync(dev + HDR + sent, pin + HDR + sent, hi - sent, hipMemcpyHostToDevice, xs);
          if (e != hipSuccess) { hipfail(e, "copy"); break; }
          sent = hi;
          ++ncopies;
          progress = true;
        }
        if (complete && sent == wbytes[wc]) {
          // every piece of the window has landed: decide each member, header, K3b, digests back
          uint64_t* h_offs = (uint64_t*)pin;
          uint64_t* h_lens = h_offs + CK_WIN_FILES;
          const size_t m = wmem[wc + 1] - wmem[wc];
          size_t sampled = 0;  // members the contents hash will route to K1P
          for (size_t k = wmem[wc]; k < wmem[wc + 1]; k++) {
            const size_t i = mfile[k], j = k - wmem[wc];
            h_offs[j] = moff[k];
            h_lens[j] = 0;  // failed or redone entries are hashed as empty buffers and ignored
            if (int er = merr[k].load()) { status[i] = -er; kind[i] = K_ERROR; continue; }
            const uint64_t got = mgot[k].load();
            // grew past its slot, or read unlike a local regular file (a short read before
            // the end, or an end before st_size): sd_cas_file_checksum afterwards, which reads
            // such a file exactly as hash.rs:15-21 does (1 MiB reads, stop at the first short one)
            if (got == mcap[k] || mirr[k].load() || got < fsize[i]) { kind[i] = K_STREAM; continue; }
            h_lens[j] = got;
            sampled += got > MINIMUM_FILE_SIZE;
            // the window's key is le64(got) || what was read: the row's key only when that is
            // the metadata length too (a procfs file reads past its st_size of 0)
            if (out_keys && got == fsize[i]) khave[i] = 1;
          }
          hipError_t e = hipSuccess;
          if (SD_CK_COPY_STREAMS > 1) {  // the header copy (on cs) after copy2's pieces too
            e = hipEventRecord(landed, c->copy2);
            if (e == hipSuccess) e = hipStreamWaitEvent(cs, landed, 0);
          }
          if (e == hipSuccess) e = hipMemcpyAsync(dev, pin, CK_WIN_FILES * 16, hipMemcpyHostToDevice, cs);
          if (e == hipSuccess) e = hipEventRecord(landed, cs);
          if (e == hipSuccess) e = hipStreamWaitEvent(s, landed, 0);
          if (e == hipSuccess)
            e = checksum_batch_device((const uint8_t*)(dev + HDR), wbytes[wc], (const uint64_t*)dev,
                                      (const uint64_t*)dev + CK_WIN_FILES, m,
                                      (uint32_t*)(dev + CK_WIN_FILES * 16), d_bad, c->ws.p, s);
          if (e == hipSuccess && out_keys) {  // the same buffers' cas keys, after the digests
            e = inplace_classify(wbytes[wc], (const uint64_t*)dev, (const uint64_t*)dev + CK_WIN_FILES, m,
                                 c->inplace.p, s);
            if (e == hipSuccess)
              e = contents_hash_classified(c, (const uint8_t*)(dev + HDR), (const uint64_t*)dev,
                                           (const uint64_t*)dev + CK_WIN_FILES, m, sampled,
                                           (uint64_t*)(dev + CK_WIN_FILES * 16 + m * 32), s);
          }
          if (e == hipSuccess)
            e = hipMemcpyAsync(pin + CK_WIN_FILES * 16, dev + CK_WIN_FILES * 16, m * (out_keys ? 40 : 32),
                               hipMemcpyDeviceToHost, s);
          if (e == hipSuccess) e = hipEventRecord(done[b], s);
          if (e != hipSuccess) { hipfail(e, "window"); break; }
          ++issued;
          ++wc;
          sent = 0;
          continue;
        }
      }
      if (progress) continue;
      // nothing to copy or retire: read a piece too (a 16th reader) if its slot is free
      // (only a piece whose slot is free now: this thread is the one that frees slots)
      size_t p = next.load(std::memory_order_relaxed);
      if (SD_CK_PUMP_READS && p < np && slot_free(pieces[p].win) && next.compare_exchange_strong(p, p + 1)) {
        read_piece(p);
        fin[p].store(1, std::memory_order_release);
      } else {
        const auto t0 = std::chrono::steady_clock::now();
        spin();
        if (tr.on) stall_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      }
    }
  };
  if (nw) {
#if SD_CK_PUMP_ON_POOL
    // the pump runs on a pool thread too (bound to the GPU's NUMA node like the readers, see
    // sd_cas_ctx_create), the calling thread only waits
    std::atomic<bool> pump_taken{false};
    const std::function<void()> pool_fn = [&]() {
      if (!pump_taken.exchange(true)) pump(); else worker();
    };
    c->pool.run2(std::max(2u, std::min(16u, (unsigned)((np + 1) / 2) + 1)), pool_fn, []() {});
#else
    c->pool.run2(std::max(1u, std::min(15u, (unsigned)((np + 1) / 2))), worker, pump);
#endif
    tr.mark("windows");
    tr.note("windows", (double)nw);
    tr.note("pieces", (double)np);
    tr.note("copies", (double)ncopies);
    tr.note("pump_idle_us", stall_us);
    if (tr.on) tr.note("pinned_node", (double)sd_page_node(c->pinned));
    uint32_t bad = 0;
    if (rc == SD_CAS_OK) {
      hipError_t e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = fail(c, SD_CAS_EHIP, "file_checksums: %s", hipGetErrorString(e));
      else if (bad) rc = fail(c, SD_CAS_EHIP, "file_checksums: batch work list overflow");
    }
    (void)sd_ws_release(c, s);
    // a failed call leaves nothing in flight that reads the pinned slots
    (void)hipStreamSynchronize(cs);
    (void)hipStreamSynchronize(c->copy2);
    (void)hipStreamSynchronize(s);
  }
  destroy_events();
  if (rc) return rc;
  // big regular files: 64 MiB segments of all of them in one piece queue, back to back (after
  // the windows: it reuses the pinned and device staging)
  {
    std::vector<size_t> bi;
    std::vector<const char*> bp;
    std::vector<uint64_t> bs;
    for (size_t i = 0; i < n; i++)
      if (kind[i] == K_STREAM && big[i]) { bi.push_back(i); bp.push_back(paths[i]); bs.push_back(fsize[i]); }
    if (!bi.empty()) {
      std::vector<uint8_t> dg(32 * bi.size()), gs(bi.size());
      std::vector<int> er(bi.size());
      if ((rc = file_checksums_pieces(c, bp.data(), bs.data(), bi.size(), dg.data(), er.data(),
                                      gs.data())))
        return rc;
      for (size_t k = 0; k < bi.size(); k++) {
        const size_t i = bi[k];
        if (er[k]) { status[i] = -er[k]; kind[i] = K_ERROR; continue; }
        if (gs[k]) continue;  // read irregularly (or changed since stat): the path below
        char* o = out_hex + 65 * i;
        for (int j = 0; j < 32; j++) { o[2 * j] = hx[dg[32 * k + j] >> 4]; o[2 * j + 1] = hx[dg[32 * k + j] & 15]; }
        o[64] = 0;
        kind[i] = K_BATCH;
      }
    }
  }
  tr.mark("big");
  // everything else off the windows — files that grew or read irregularly there, files that
  // changed since stat, non-regular files: sd_cas_file_checksum, one at a time
  for (size_t i = 0; i < n; i++) {
    if (kind[i] != K_STREAM) continue;
    char* o = out_hex + 65 * i;
    int err_no = 0;
    const int r = sd_cas_file_checksum(c, paths[i], o, &err_no);
    if (r == SD_CAS_EIO) { status[i] = -(err_no ? err_no : EIO); o[0] = 0; continue; }
    if (r) return r;
  }
  tr.mark("streamed");
  for (size_t i = 0; i < n; i++)
    if (status[i]) out_hex[65 * i] = 0;
  if (out_keys) {
    // rows that want a key and did not get it from a window (big, irregular or changed
    // files): the path gather, decided by the sizes of the stat pass above
    std::vector<size_t> ri;
    std::vector<const char*> rp;
    std::vector<uint64_t> rs;
    for (size_t i = 0; i < n; i++)
      if (cas_status[i] == 0 && !khave[i]) { ri.push_back(i); rp.push_back(paths[i]); rs.push_back(out_sizes[i]); }
    if (!ri.empty()) {
      std::vector<uint64_t> rk(ri.size());
      std::vector<int32_t> rst(ri.size());
      if ((rc = sd_cas_generate_cas_ids_from_paths(c, rp.data(), rs.data(), ri.size(), rk.data(), rst.data())))
        return rc;
      for (size_t k = 0; k < ri.size(); k++) { out_keys[ri[k]] = rk[k]; cas_status[ri[k]] = rst[k]; }
    }
    tr.mark("gathered");
  }
  return SD_CAS_OK;
}

int sd_cas_file_checksums(sd_cas_ctx* c, const char* const* paths, size_t n, char* out_hex,
                          int32_t* status) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!paths || !out_hex || !status) return fail(c, SD_CAS_EINVAL, "file_checksums: null argument");
  return file_checksums_impl(c, paths, n, out_hex, status, nullptr, nullptr, nullptr);
}

int sd_cas_identify_validate_paths(sd_cas_ctx* c, const char* const* paths, size_t n,
                                   uint64_t* out_keys, int32_t* cas_status, uint64_t* out_sizes,
                                   char* out_hex, int32_t* ck_status) {
  if (!c) return SD_CAS_EINVAL;
  if (n == 0) return SD_CAS_OK;
  if (!paths || !out_keys || !cas_status || !out_sizes || !out_hex || !ck_status || n >= (1ull << 32))
    return fail(c, SD_CAS_EINVAL, "identify_validate_paths: null argument");
  return file_checksums_impl(c, paths, n, out_hex, ck_status, out_keys, cas_status, out_sizes);
}

}  // extern "C"
