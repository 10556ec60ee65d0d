// validator_host.cpp — the validator's entry points of the C ABI (include/sd_hip_cas.h):
// sd_cas_checksum_dev / sd_cas_file_checksum (file_checksum, core/src/object/validation/
// hash.rs:9-25: hash.rs's read loop exactly, K3 on the device) and sd_cas_checksums_dev /
// sd_cas_file_checksums (the validator job over many files, validator_job.rs:107-172: K3b).
// Every digest comes from the HIP kernels.
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
#include "sd_piece_queue.h"

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
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  if (batch) {
    uint64_t* d_ol = c->d_scalar + 4;
    HIP_TRY(c, checksum_single_setup(d_ol, len, (uint32_t*)(c->d_scalar + 6), s));
    HIP_TRY(c, checksum_batch_device((const uint8_t*)d_data, len, d_ol, d_ol + 1, 1, d_out,
                                     (uint32_t*)(c->d_scalar + 6), c->ws.p, s));
  } else {
    HIP_TRY(c, checksum_device((const uint8_t*)d_data, len, 0, true, d_out, c->ws.p, s));
  }
  HIP_TRY(c, hipMemcpyAsync(out, d_out, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, ws.release());
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

// file_checksum(path) (validation/hash.rs:11-25): the reference issues one read() of
// BLOCK_LEN = 1 MiB per iteration into one hasher and stops at the FIRST read that returns
// fewer bytes — the end of a regular file on a local filesystem, but after the first short
// read on anything that returns short reads before its end (procfs seq_files give about one
// page per read, FIFOs and FUSE/network mounts whatever is ready).
// Two read modes, one result:
//   * pieces (regular files, file_checksums_pieces): the file is planned from st_size and read
//     through the piece queue; a file whose reads show it is not read like a local file is
//     redone sequentially;
//   * sequential (everything else, and those redos, file_checksum_seq): hash.rs's loop literally.
// The segment CVs are merged on the GPU (pair-and-promote, ROOT on the last parent); a file
// of one segment is hashed with ROOT inside the segment.

// The three slot events and the copies' event of the file paths, created and destroyed here only.
struct SlotEvents {
  hipEvent_t done[3] = {}, landed = nullptr;
  bool ok = true;
  SlotEvents() {
    for (hipEvent_t* e : {&done[0], &done[1], &done[2], &landed})
      ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  }
  ~SlotEvents() {
    for (hipEvent_t e : {done[0], done[1], done[2], landed})
      if (e) (void)hipEventDestroy(e);
  }
  SlotEvents(const SlotEvents&) = delete;
};

// The piece queue's device (sd_piece_queue.h): pinned slot -> staging slot over c->copy /
// c->copy2, the work on c->stream.  begin() runs on the pump thread (HIP's current device is
// per thread) and takes the workspace, which the queue's caller releases after the run; zero: a
// flag word the unit kernels report into.
struct QueueDev {
  sd_cas_ctx* c;
  uint32_t* zero;
  SlotEvents ev;
  WsLease ws;
  int begin() {
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = (ws = WsLease(c, c->stream)).error();
    if (e == hipSuccess && zero) e = hipMemsetAsync(zero, 0, 4, c->stream);
    return e;
  }
  int copy(int k, size_t at, size_t bytes) {
    return hipMemcpyAsync((char*)c->staging.p + at, (char*)c->pinned + at, bytes, hipMemcpyHostToDevice,
                          k ? c->copy2 : c->copy);
  }
  int join(hipStream_t from, hipStream_t to) {
    const hipError_t e = hipEventRecord(ev.landed, from);
    return e == hipSuccess ? hipStreamWaitEvent(to, ev.landed, 0) : e;
  }
  int join_copies() { return join(c->copy2, c->copy); }
  int join_compute() { return join(c->copy, c->stream); }
  int record_done(int b) { return hipEventRecord(ev.done[b], c->stream); }
  int query_done(int b, bool& ready) {
    const hipError_t q = hipEventQuery(ev.done[b]);
    ready = q == hipSuccess;
    return q == hipErrorNotReady ? 0 : q;
  }
  void drain() {
    for (hipStream_t x : {c->copy, c->copy2, c->stream}) (void)hipStreamSynchronize(x);
  }
};
static int queue_failed(sd_cas_ctx* c, const char* call, const sdq::Result& r) {
  return fail(c, SD_CAS_EHIP, "%s %s: %s", call, r.what, hipGetErrorString((hipError_t)r.err));
}

static int cv_capacity(sd_cas_ctx* c, DevBuf& cvb, size_t need_cvs, hipStream_t s) {
  if (need_cvs * 32 <= cvb.bytes) return SD_CAS_OK;
  DevBuf nb;
  const size_t want = std::max<size_t>(need_cvs * 2 * 32, 1 << 16);
  HIP_TRY(c, hipStreamSynchronize(s));
  if (sd_dev_malloc(&nb.p, want, "cvbuf") != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SD_CAS_ENOMEM, "hipMalloc(%zu) failed", want);
  }
  nb.bytes = want;
  if (cvb.p) {
    HIP_TRY(c, hipMemcpy(nb.p, cvb.p, cvb.bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(c, sd_dev_free(cvb.p));
  }
  cvb = nb;
  return SD_CAS_OK;
}

// The pieces mode of file_checksum, over one or many files in ONE queue: every file is planned
// from its st_size (+ one probe byte: data there means the file grew) as 64 MiB segments (a
// segment = one complete 65,536-chunk subtree); the segments of all files, in file order, are
// the queue's units, so a validator job's large files stream back to back with no per-file
// fill and drain.  A complete segment is hashed (K3 at its chunk offset, ROOT inside for a
// one-segment file) and, after a file's last segment, the file's CVs are reduced into its
// digest.  Per file: digests[32 j], errs[j] = the errno of a failed open/read (0 otherwise),
// go_seq[j] = 1 when its reads were irregular (sdq::read_piece, or a segment that did not hold
// exactly its planned bytes): redo with hash.rs's sequential reads.  Returns SD_CAS_OK or a
// HIP / allocation error.
static int file_checksums_pieces(sd_cas_ctx* c, const char* const* paths, const uint64_t* sizes,
                                 size_t nf, uint8_t* digests, int* errs, uint8_t* go_seq) {
  constexpr uint64_t SEG = 64ull << 20;  // 65,536 chunks: a complete left subtree
  if (nf == 0) return SD_CAS_OK;
  struct Seg { uint32_t file; uint64_t k, len, want; };  // len: planned bytes, want: bytes to hash
  std::vector<Seg> segs;
  std::vector<uint64_t> nreal(nf), cvbase(nf + 1, 0);
  uint64_t maxtotal = 0, maxreal = 1;
  for (size_t j = 0; j < nf; j++) {
    const uint64_t total = sizes[j] + 1;  // + the probe byte
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
  const uint64_t cap = std::min<uint64_t>(SEG, ((maxtotal + 4095) / 4096) * 4096);
  sdq::Plan pl;
  pl.slot_bytes = up256(cap + 16);
  for (const Seg& sg : segs) {
    sdq::cut_pieces(sg.len, sdq::PIECE, [&](uint64_t off, uint64_t len) { pl.add_piece(off, len); });
    pl.end_unit(sg.want);
  }
  const uint64_t ncv = cvbase[nf];
  hipStream_t s = c->stream;
  int rc = SD_CAS_OK;
  if ((rc = ensure_pinned(c, pl.slots * pl.slot_bytes)) || (rc = ensure(c, c->staging, pl.slots * pl.slot_bytes)))
    return rc;
  if ((rc = ensure(c, c->ws, std::max({checksum_workspace_bytes(cap), checksum_workspace_bytes(1 << 20),
                                        reduce_cvs_workspace_bytes(maxreal)}))))
    return rc;
  if ((rc = cv_capacity(c, c->cvbuf, ncv + nf, s))) return rc;  // CVs, then the digests
  uint32_t* d_cv = (uint32_t*)c->cvbuf.p;
  uint32_t* d_dig = d_cv + 8 * ncv;
  QueueDev dev{c, nullptr};
  if (!dev.ev.ok) return fail(c, SD_CAS_EHIP, "file_checksum: event create");
  // per segment: bytes read; per file: read error, irregular read (all zero-initialised)
  std::vector<std::atomic<uint64_t>> sgot(segs.size());
  std::vector<std::atomic<int>> ferr(nf);
  std::vector<std::atomic<uint8_t>> firr(nf);
  std::vector<uint8_t> fok(nf, 1);  // (pump only) every segment of the file so far as planned
  auto read = [&](size_t p, size_t at) {
    const uint32_t g = pl.punit[p], j = segs[g].file;
    if (ferr[j].load(std::memory_order_relaxed) || firr[j].load(std::memory_order_relaxed)) return;
    const uint64_t foff = segs[g].k * SEG + pl.poff[p];
    const sdq::ReadResult r =
        sdq::read_piece(paths[j], (char*)c->pinned + at, foff, pl.plen[p], foff + pl.plen[p] < sizes[j] + 1);
    if (r.err) ferr[j].store(r.err);
    if (r.irregular) firr[j].store(1);
    sgot[g].fetch_add(r.got);
  };
  auto last_of_file = [&](const Seg& sg) { return sg.k + 1 == (sizes[sg.file] + SEG) / SEG; };
  auto landed = [&](size_t g) {  // the segment must hold exactly its planned bytes (the probe byte none)
    const Seg& sg = segs[g];
    const uint32_t j = sg.file;
    if (ferr[j].load() || firr[j].load() || sgot[g].load() != (last_of_file(sg) ? sg.len - 1 : sg.len)) fok[j] = 0;
    return 0;
  };
  auto issue = [&](size_t g) {
    const Seg& sg = segs[g];
    const uint32_t j = sg.file;
    hipError_t e = hipSuccess;
    if (!fok[j]) return e;
    if (sg.k < nreal[j])
      e = checksum_device((const uint8_t*)c->staging.p + (g % pl.slots) * pl.slot_bytes, sg.want,
                          (sg.k * SEG) >> 10, nreal[j] == 1, d_cv + 8 * (cvbase[j] + sg.k), c->ws.p, s);
    if (e == hipSuccess && last_of_file(sg))  // the file's digest
      e = nreal[j] == 1 ? hipMemcpyAsync(d_dig + 8 * j, d_cv + 8 * cvbase[j], 32, hipMemcpyDeviceToDevice, s)
                        : reduce_cvs_device(d_cv + 8 * cvbase[j], nreal[j], d_dig + 8 * j, c->ws.p, s);
    return e;
  };
  pl.threads = std::max(2u, std::min(16u, (unsigned)std::min<size_t>(pl.pieces() + 1, 16)));
  const sdq::Result res = sdq::run(pl, c->pool, dev, read, landed, issue, [](size_t) {});
  if (res.err) rc = queue_failed(c, "file_checksum segment", res);
  if (rc == SD_CAS_OK) {
    hipError_t e = hipMemcpyAsync(digests, d_dig, nf * 32, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(c, SD_CAS_EHIP, "checksum digests: %s", hipGetErrorString(e));
  }
  (void)dev.ws.release();
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
  SlotEvents ev;  // (two of its slots)
  if (!ev.ok) return fail(c, SD_CAS_EHIP, "file_checksum: event create");
  hipEvent_t* done = ev.done;
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
  WsLease ws(c, s);
  if (ws.error() != hipSuccess) return fail(c, SD_CAS_EHIP, "file_checksum: %s", hipGetErrorString(ws.error()));
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
    if (nseg > 1) rc = ensure(c, c->ws, reduce_cvs_workspace_bytes(nseg));
    if (rc == SD_CAS_OK) {
      if (nseg == 1) e = hipMemcpyAsync(d_out, c->cvbuf.p, 32, hipMemcpyDeviceToDevice, s);
      else e = reduce_cvs_device((uint32_t*)c->cvbuf.p, nseg, d_out, c->ws.p, s);
      if (e == hipSuccess) e = hipMemcpyAsync(digest, d_out, 32, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = fail(c, SD_CAS_EHIP, "checksum reduce: %s", hipGetErrorString(e));
    }
  }
  (void)hipStreamSynchronize(s);  // no segment copy may still read the pinned buffers
  (void)ws.release();
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
  sd_hex32(digest, out_hex);
  return SD_CAS_OK;
}

// ---- the validator job over many files -----------------------------------------------

// what the bad flags of classify (bits 1, 4) and of the batch chain (those and its CV list's
// bound) say
static const char* batch_bad_message(uint32_t bad) {
  return (bad & 1) ? "a buffer is longer than 64 GiB"
                   : (bad & 4) ? "a buffer is misaligned or extends past arena_bytes"
                               : "the buffers' subtrees exceed arena_bytes' bound (overlapping buffers?)";
}

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
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, s));
  HIP_TRY(c, checksum_batch_device((const uint8_t*)d_arena, arena_bytes, d_offs, d_lens, n,
                                   (uint32_t*)d_out, d_bad, c->ws.p, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, ws.release());
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad) return fail(c, SD_CAS_EINVAL, "checksums: %s", batch_bad_message(bad));
  return SD_CAS_OK;
}

// ---- cas_ids from whole contents in place (cas_inplace.hip) -----------------------------

// After inplace_classify on s: whole files through the packed dispatcher over classify's u32
// lengths (sampled files count as empty there; their keys are rewritten next), then K1P over
// the sampled list.  c->inplace and c->ws are sized and ws is acquired by the caller.
static hipError_t contents_hash_classified(sd_cas_ctx* c, const uint8_t* arena, const uint64_t* offs,
                                           const uint64_t* lens, size_t n, size_t n_sampled,
                                           uint64_t* keys, hipStream_t s) {
  const InplaceWs iw = inplace_layout(c->inplace.p, n);
  hipError_t e = hipSuccess;
  if (n_sampled < n) e = sd_dispatch_packed(c, arena, offs, iw.lens32, lens, n, keys, s);
  if (e == hipSuccess) e = hash_inplace_sampled(arena, offs, lens, iw.sampled_idx, n_sampled, keys, s);
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
  WsLease ws(c, s);  HIP_TRY(c, ws.error());
  HIP_TRY(c, inplace_classify(arena_bytes, d_offs, d_lens, n, c->inplace.p, s));
  HIP_TRY(c, hipMemcpyAsync(verdict, inplace_layout(c->inplace.p, n).counters, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (verdict[0]) return fail(c, SD_CAS_EINVAL, "%s: %s", what, batch_bad_message(verdict[0]));
  HIP_TRY(c, contents_hash_classified(c, (const uint8_t*)d_arena, d_offs, d_lens, n, verdict[1],
                                      d_keys, s));
  if (!digests) {
    HIP_TRY(c, ws.release());
    return SD_CAS_OK;
  }
  // the chain's own flag can only still report its CV list's bound (overlapping buffers)
  uint32_t* d_bad = (uint32_t*)(c->d_scalar + 6);
  uint32_t bad = 0;
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, s));
  HIP_TRY(c, checksum_batch_device((const uint8_t*)d_arena, arena_bytes, d_offs, d_lens, n,
                                   (uint32_t*)d_digests, d_bad, c->ws.p, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, ws.release());
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad) return fail(c, SD_CAS_EINVAL, "%s: %s", what, batch_bad_message(bad & ~5u));
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
// bytes / CK_WIN_FILES files in index order (one room of up128(st_size + 1) bytes per file:
// the spare byte shows EOF, so a file that grew since stat fills its room and is redone by the
// streaming path).  The windows are the units of one piece queue over the whole job
// (sd_piece_queue.h; round 6): 1 MiB reads into the pinned slot run faster
// host-side than one whole-file pread (profiles/r05/official_c/probe_pread.log), and one copy
// stream moves 8 MiB prefixes at ~53 GB/s, two at ~57 (profiles/r06/validator/h2d_sizes.log).
// A landed window gets its header, K3b and its digests back on the compute stream.  Up to 15
// readers and the pump run on the pool, which sits on the GPU's NUMA node (sd_cas_ctx_create).
// Warm 2,000-file tmpfs set: 53.5-54.7 GB/s vs 51.6-52.4 with one copy stream and 49.9-53.0
// with the pump on the calling thread (profiles/r06/validator/s7_*).  Pinned and device slot
// layout: offs | lens | digests (| keys) | data.
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
  // members (batch files) in index order, grouped into windows; each member's offset in the
  // window's data and its capacity; its pieces in data byte order (so a prefix of pieces is a
  // prefix of bytes)
  std::vector<size_t> mfile, wmem{0};
  std::vector<uint64_t> moff, mcap;
  std::vector<uint32_t> pmem;  // per piece: its member
  sdq::Plan pl;
  pl.slot_bytes = SLOT;
  pl.data_off = HDR;
  pl.trace = tr.on;
  {
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; i++) {
      if (kind[i] != K_BATCH) continue;
      const uint64_t need = up128(fsize[i] + 1);
      const size_t files = mfile.size() - wmem.back();
      if (files && (bytes + need > CK_WIN || files == CK_WIN_FILES)) {
        pl.end_unit(bytes);
        wmem.push_back(mfile.size());
        bytes = 0;
      }
      const uint32_t k = (uint32_t)mfile.size();
      mfile.push_back(i);
      moff.push_back(bytes);
      mcap.push_back(need);
      sdq::cut_pieces(need, sdq::PIECE, [&](uint64_t off, uint64_t len) {
        pl.add_piece(bytes + off, len);
        pmem.push_back(k);
      });
      bytes += need;
    }
    if (mfile.size() > wmem.back()) {
      pl.end_unit(bytes);
      wmem.push_back(mfile.size());
    }
  }
  const size_t nw = pl.units(), nm = mfile.size(), np = pl.pieces();
  int rc = SD_CAS_OK;
  if (nw) {
    if ((rc = ensure_pinned(c, pl.slots * SLOT))) return rc;
    if ((rc = ensure(c, c->staging, pl.slots * SLOT))) return rc;
    size_t wsb = checksum_batch_workspace_bytes(CK_WIN_FILES, CK_WIN);
    if (out_keys) {
      for (size_t w = 0; w < nw; w++) wsb = std::max(wsb, sd_packed_workspace_bytes(c, wmem[w + 1] - wmem[w]));
      if ((rc = ensure(c, c->inplace, inplace_workspace_bytes(CK_WIN_FILES)))) return rc;
    }
    if ((rc = ensure(c, c->ws, wsb))) return rc;
    hipStream_t s = c->stream;
    uint32_t* d_bad = (uint32_t*)(c->d_scalar + 6);
    QueueDev dev{c, d_bad};
    if (!dev.ev.ok) return fail(c, SD_CAS_EHIP, "file_checksums: event create");
    // per member: bytes read, read error, irregular read (all zero-initialised)
    std::vector<std::atomic<uint64_t>> mgot(nm);
    std::vector<std::atomic<int>> merr(nm);
    std::vector<std::atomic<uint8_t>> mirr(nm);
    auto read = [&](size_t p, size_t at) {
      const uint32_t k = pmem[p];
      const uint64_t foff = pl.poff[p] - moff[k];
      const sdq::ReadResult r =
          sdq::read_piece(paths[mfile[k]], (char*)c->pinned + at, foff, pl.plen[p], foff + pl.plen[p] < mcap[k]);
      if (r.err) merr[k].store(r.err);
      if (r.irregular) mirr[k].store(1);
      mgot[k].fetch_add(r.got);
    };
    size_t sampled = 0;  // (pump only) members of the landed window that the contents hash routes to K1P
    // every piece of window w has landed: decide each member, build and send the header
    auto landed = [&](size_t w) {
      char* pin = (char*)c->pinned + (w % pl.slots) * SLOT;
      uint64_t* h_offs = (uint64_t*)pin;
      uint64_t* h_lens = h_offs + CK_WIN_FILES;
      sampled = 0;
      for (size_t k = wmem[w]; k < wmem[w + 1]; k++) {
        const size_t i = mfile[k], j = k - wmem[w];
        h_offs[j] = moff[k];
        h_lens[j] = 0;  // failed or redone entries are hashed as empty buffers and ignored
        if (int er = merr[k].load()) { status[i] = -er; kind[i] = K_ERROR; continue; }
        const uint64_t got = mgot[k].load();
        // grew past its room, or read unlike a local regular file (a short read before the
        // end, or an end before st_size): sd_cas_file_checksum afterwards, which reads such a
        // file exactly as hash.rs:15-21 does (1 MiB reads, stop at the first short one)
        if (got == mcap[k] || mirr[k].load() || got < fsize[i]) { kind[i] = K_STREAM; continue; }
        h_lens[j] = got;
        sampled += got > MINIMUM_FILE_SIZE;
        // the window's key is le64(got) || what was read: the row's key only when that is
        // the metadata length too (a procfs file reads past its st_size of 0)
        if (out_keys && got == fsize[i]) khave[i] = 1;
      }
      return hipMemcpyAsync((char*)c->staging.p + (w % pl.slots) * SLOT, pin, CK_WIN_FILES * 16,
                            hipMemcpyHostToDevice, c->copy);
    };
    auto issue = [&](size_t w) {  // K3b, the keys, digests and keys back
      char* pin = (char*)c->pinned + (w % pl.slots) * SLOT;
      char* dev_slot = (char*)c->staging.p + (w % pl.slots) * SLOT;
      const uint64_t* d_offs = (const uint64_t*)dev_slot;
      const uint64_t* d_lens = d_offs + CK_WIN_FILES;
      const size_t m = wmem[w + 1] - wmem[w];
      hipError_t e = checksum_batch_device((const uint8_t*)(dev_slot + HDR), pl.usend[w], d_offs, d_lens, m,
                                           (uint32_t*)(dev_slot + CK_WIN_FILES * 16), d_bad, c->ws.p, s);
      if (e == hipSuccess && out_keys) {  // the same buffers' cas keys, after the digests
        e = inplace_classify(pl.usend[w], d_offs, d_lens, m, c->inplace.p, s);
        if (e == hipSuccess)
          e = contents_hash_classified(c, (const uint8_t*)(dev_slot + HDR), d_offs, d_lens, m, sampled,
                                       (uint64_t*)(dev_slot + CK_WIN_FILES * 16 + m * 32), s);
      }
      if (e == hipSuccess)
        e = hipMemcpyAsync(pin + CK_WIN_FILES * 16, dev_slot + CK_WIN_FILES * 16, m * (out_keys ? 40 : 32),
                           hipMemcpyDeviceToHost, s);
      return e;
    };
    auto emit = [&](size_t w) {  // window w's digests are back in its pinned slot: -> hex
      const uint8_t* dg = (const uint8_t*)c->pinned + (w % pl.slots) * SLOT + CK_WIN_FILES * 16;
      const size_t m = wmem[w + 1] - wmem[w];
      for (size_t j = 0; j < m; j++) sd_hex32(dg + 32 * j, out_hex + 65 * mfile[wmem[w] + j]);
      if (!out_keys) return;
      // the window's keys follow its digests; a member whose key is not the window's (khave),
      // or that has no cas_id, keeps key 0
      for (size_t j = 0; j < m; j++) {
        const size_t i = mfile[wmem[w] + j];
        if (khave[i] && cas_status[i] == 0) memcpy(&out_keys[i], dg + 32 * m + 8 * j, 8);
      }
    };
    pl.threads = std::max(2u, std::min(16u, (unsigned)((np + 1) / 2) + 1));
    const sdq::Result res = sdq::run(pl, c->pool, dev, read, landed, issue, emit);
    if (res.err) rc = queue_failed(c, "file_checksums window", res);
    tr.mark("windows");
    tr.note("windows", (double)nw);
    tr.note("pieces", (double)np);
    tr.note("copies", (double)res.copies);
    tr.note("pump_idle_us", res.pump_idle_us);
    if (tr.on) tr.note("pinned_node", (double)sd_page_node(c->pinned));
    uint32_t bad = 0;
    if (rc == SD_CAS_OK) {
      hipError_t e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = fail(c, SD_CAS_EHIP, "file_checksums: %s", hipGetErrorString(e));
      else if (bad) rc = fail(c, SD_CAS_EHIP, "file_checksums: batch work list overflow");
    }
    (void)dev.ws.release();
  }
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
        sd_hex32(&dg[32 * k], out_hex + 65 * i);
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
