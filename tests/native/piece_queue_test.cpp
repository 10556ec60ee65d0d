// CPU test of the validator's piece queue (spacedrive_amd/csrc/sd_piece_queue.h): the cutter
// at its boundaries, the reader on real files (argv[1] = a scratch directory), and the engine
// itself — the real sdq::run on a real HostPool over a fake device whose "copy" is a memcpy
// into an ordinary buffer, whose `done` needs a few polls, and which logs every operation.
// Jobs of a few thousand pieces of 1-63 bytes in many more units than slots, with one-piece
// units, units that send nothing (a probe-only last segment), failed units, 1-15 readers, the
// pump on the pool and on the caller.  Checked per job:
//   (a) every piece is read exactly once;
//   (b) at a unit's issue() the device memory holds exactly the unit's bytes;
//   (c) no piece of unit u is read before unit u - slots has retired;
//   (d) the log shows, for every unit (failed ones too): its copies (contiguous, alternating
//       streams), the copy-stream join, landed(), the join into compute, issue(), done — and
//       nothing of another unit in between;
//   (e) retired() comes once per unit, in order;
//   (f) an error injected at a random operation ends the run with that error, every thread
//       back, and the pool runs the next job.
// Exit 0 and "piece queue ok" = ok.  Built by tests/test_piece_queue_cpu.py, once plain and
// once with the thread sanitizer.
#include <sys/stat.h>

#include <random>
#include <string>

#include "ctx_internal.h"
#include "sd_piece_queue.h"

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("%s:%d: %s: ", __FILE__, __LINE__, #cond);    \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
      return 1;                                            \
    }                                                      \
  } while (0)

static int test_cutter() {
  const uint64_t P = 1024;
  for (uint64_t len : {(uint64_t)0, (uint64_t)1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 3 * P + 129}) {
    uint64_t at = 0, count = 0;
    bool tiled = true;
    const uint64_t np = sdq::cut_pieces(len, P, [&](uint64_t off, uint64_t n) {
      tiled = tiled && off == at && (n > 0 || len == 0);
      at += n;
      ++count;
    });
    CHECK(tiled && at == len, "len %llu: pieces do not tile [0, len) in order", (unsigned long long)len);
    CHECK(np == count && count == std::max<uint64_t>(1, len / P), "len %llu: %llu pieces",
          (unsigned long long)len, (unsigned long long)count);
  }
  return 0;
}

static char file_byte(uint64_t i) { return (char)(i * 37 + 11); }
static bool write_file(const std::string& path, uint64_t n) {
  std::string s(n, 0);
  for (uint64_t i = 0; i < n; i++) s[i] = file_byte(i);
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(s.data(), 1, n, f) == n;
  return fclose(f) == 0 && ok;
}
static bool holds(const char* buf, uint64_t foff, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (buf[i] != file_byte(foff + i)) return false;
  return true;
}

static int test_reader(const std::string& dir) {
  char buf[256];
  const std::string exact = dir + "/exact", grown = dir + "/grown", cut = dir + "/cut";
  CHECK(write_file(exact, 100) && write_file(grown, 101) && write_file(cut, 60), "cannot write under %s", dir.c_str());
  // planned 100 bytes + the probe byte: the file as planned gives 100 and is regular
  sdq::ReadResult r = sdq::read_piece(exact.c_str(), buf, 0, 101, false);
  CHECK(r.got == 100 && !r.err && !r.irregular && holds(buf, 0, 100), "exact: got %llu err %d irr %d",
        (unsigned long long)r.got, r.err, r.irregular);
  r = sdq::read_piece(exact.c_str(), buf, 10, 50, true);  // an inner piece
  CHECK(r.got == 50 && !r.err && !r.irregular && holds(buf, 10, 50), "inner: got %llu", (unsigned long long)r.got);
  // one byte longer than planned: the probe byte comes back
  r = sdq::read_piece(grown.c_str(), buf, 0, 101, false);
  CHECK(r.got == 101 && !r.err && !r.irregular && holds(buf, 0, 101), "grown: got %llu", (unsigned long long)r.got);
  // truncated to 60 of the planned 100: irregular on a piece that is not the file's last ...
  r = sdq::read_piece(cut.c_str(), buf, 32, 32, true);
  CHECK(r.got == 28 && !r.err && r.irregular && holds(buf, 32, 28), "cut inner: got %llu irr %d",
        (unsigned long long)r.got, r.irregular);
  // ... and not on its last (the caller sees the shortfall in the byte count)
  r = sdq::read_piece(cut.c_str(), buf, 50, 51, false);
  CHECK(r.got == 10 && !r.err && !r.irregular && holds(buf, 50, 10), "cut last: got %llu irr %d",
        (unsigned long long)r.got, r.irregular);
  r = sdq::read_piece((dir + "/missing").c_str(), buf, 0, 16, false);
  CHECK(r.got == 0 && r.err == ENOENT, "missing: err %d", r.err);
  r = sdq::read_piece(dir.c_str(), buf, 0, 16, false);
  CHECK(r.got == 0 && r.err == EISDIR, "directory: err %d", r.err);
  return 0;
}

// ---- the engine over a fake device ------------------------------------------------------

struct Op { char kind; size_t a, b, c; };  // b begin, c copy(k, at, bytes), j, k joins, d done(slot), q query(slot)
                                           // l landed(u), i issue(u), r retired(u)
constexpr int INJECTED = 77;

struct FakeDev {
  const std::vector<char>& pinned;
  std::vector<char> mem;
  std::vector<Op> log;
  long fail_at = -1, nops = 0;  // the operation (counted from 0) that fails; operations so far
  int polls[8] = {};
  bool drained = false;
  FakeDev(const std::vector<char>& host) : pinned(host), mem(host.size(), 0) {}
  int op(char kind, size_t a = 0, size_t b = 0, size_t c = 0) {  // pump thread only
    const bool bad = nops++ == fail_at;
    log.push_back({bad ? 'X' : kind, a, b, c});
    return bad ? INJECTED : 0;
  }
  int begin() { return op('b'); }
  int copy(int k, size_t at, size_t bytes) {
    if (int e = op('c', (size_t)k, at, bytes)) return e;
    if (at + bytes > mem.size()) return 1000;  // (reported by the log check as an unknown error)
    memcpy(mem.data() + at, pinned.data() + at, bytes);
    return 0;
  }
  int join_copies() { return op('j'); }
  int join_compute() { return op('k'); }
  int record_done(int b) { polls[b] = 3; return op('d', (size_t)b); }
  int query_done(int b, bool& ready) {
    ready = polls[b] == 0;
    if (!ready) --polls[b];
    return op('q', (size_t)b);
  }
  void drain() { drained = true; }
};

static char piece_byte(size_t p, uint64_t i) { return (char)(p * 131 + i * 7 + 1); }

struct Job {
  sdq::Plan pl;
  std::vector<uint8_t> ufail;  // the reader fails this unit: its pieces are not read into the slot
};

static Job make_job(std::mt19937& rng, uint64_t piece, size_t units) {
  Job j;
  uint64_t maxbytes = 0;
  for (size_t u = 0; u < units; u++) {
    uint64_t bytes = 0, send;
    const unsigned shape = rng() % 8;
    if (shape == 0) {  // probe only: one piece of one byte, nothing to send
      j.pl.add_piece(0, 1);
      bytes = 1;
      send = 0;
    } else if (shape == 1) {  // one piece
      bytes = 1 + rng() % (2 * piece - 1);
      sdq::cut_pieces(bytes, piece, [&](uint64_t off, uint64_t n) { j.pl.add_piece(off, n); });
      send = bytes;
    } else {  // a window of members / a segment with a probe byte
      const unsigned members = 1 + rng() % 6;
      for (unsigned m = 0; m < members; m++) {
        const uint64_t need = 1 + rng() % (5 * piece);
        sdq::cut_pieces(need, piece, [&](uint64_t off, uint64_t n) { j.pl.add_piece(bytes + off, n); });
        bytes += need;
      }
      send = bytes - rng() % 2;
    }
    j.pl.end_unit(send);
    j.ufail.push_back(rng() % 9 == 0);
    maxbytes = std::max(maxbytes, bytes);
  }
  j.pl.data_off = 24;
  j.pl.slot_bytes = j.pl.data_off + ((maxbytes + 15) & ~(uint64_t)15) + 8;
  j.pl.copy_unit = 3 * piece;
  return j;
}

// the operations every run of the job makes at least (a unit's prefix copies depend on timing)
static long min_ops(const Job& job) {
  long n = 1;  // begin
  for (size_t u = 0; u < job.pl.units(); u++)
    n += (job.pl.usend[u] > 0) + (job.pl.copy_streams > 1) + 4 /* l k i d */ + 4 /* queries: 3 not ready, 1 ready */;
  return n;
}

// one run of the engine; fail_at < 0: a clean run, all of (a)-(e); else (f)
static int run_job(HostPool& pool, Job& job, std::mt19937& rng, long fail_at) {
  sdq::Plan& pl = job.pl;
  const size_t nu = pl.units(), np = pl.pieces(), slots = (size_t)pl.slots;
  std::vector<char> pinned(slots * pl.slot_bytes, 0);
  FakeDev dev(pinned);
  dev.fail_at = fail_at;
  std::vector<std::atomic<int>> reads(np);
  std::atomic<size_t> retired_n{0};
  std::atomic<int> active{0}, early{0}, order{0}, content{0};
  const unsigned jitter = rng();
  auto read = [&](size_t p, size_t at) {
    active.fetch_add(1);
    const size_t u = pl.punit[p];
    if (u >= slots && retired_n.load(std::memory_order_acquire) + slots <= u) early.fetch_add(1);  // (c)
    if (at != (u % slots) * pl.slot_bytes + pl.data_off + pl.poff[p]) order.fetch_add(1);
    if (!job.ufail[u])
      for (uint64_t i = 0; i < pl.plen[p]; i++) pinned[at + i] = piece_byte(p, i);
    if ((p * 2654435761u + jitter) % 7 == 0) std::this_thread::yield();
    reads[p].fetch_add(1);
    active.fetch_sub(1);
  };
  auto landed = [&](size_t u) {
    for (size_t p = pl.upiece[u]; p < pl.upiece[u + 1]; p++)
      if (reads[p].load() != 1) order.fetch_add(1);
    return dev.op('l', u);
  };
  auto issue = [&](size_t u) {  // (b)
    const size_t base = (u % slots) * pl.slot_bytes + pl.data_off;
    for (size_t p = pl.upiece[u]; p < pl.upiece[u + 1] && !job.ufail[u]; p++)
      for (uint64_t i = 0; i < pl.plen[p] && pl.poff[p] + i < pl.usend[u]; i++)
        if (dev.mem[base + pl.poff[p] + i] != piece_byte(p, i)) content.fetch_add(1);
    return dev.op('i', u);
  };
  auto retired = [&](size_t u) {  // (e)
    if (u != retired_n.load()) order.fetch_add(1);
    dev.log.push_back({'r', u, 0, 0});
    retired_n.fetch_add(1, std::memory_order_release);
  };
  const sdq::Result res = sdq::run(pl, pool, dev, read, landed, issue, retired);
  CHECK(dev.drained && active.load() == 0, "the run returned with %d reads active", active.load());
  CHECK(early.load() == 0, "(c) %d pieces read before their slot was free", early.load());
  CHECK(order.load() == 0 && content.load() == 0, "(b)/(e) %d order and %d content violations", order.load(), content.load());
  if (fail_at >= 0) {  // (f): that error, nothing issued after it, no piece read twice
    CHECK(res.err == INJECTED && dev.log.back().kind == 'X' && dev.nops == fail_at + 1,
          "(f) err %d, %ld operations for a failure at %ld", res.err, dev.nops, fail_at);
    for (size_t p = 0; p < np; p++) CHECK(reads[p].load() <= 1, "(f) piece %zu read %d times", p, reads[p].load());
    return 0;
  }
  CHECK(res.err == 0, "clean run: err %d at %s", res.err, res.what);
  for (size_t p = 0; p < np; p++) CHECK(reads[p].load() == 1, "(a) piece %zu read %d times", p, reads[p].load());
  CHECK(retired_n.load() == nu, "(e) %zu of %zu units retired", retired_n.load(), nu);
  // (d): the log, queries and retirements aside, is begin, then per unit c* [j] l k i d
  size_t u = 0, ncopies = 0, nret = 0;
  uint64_t sent = 0;
  const char* want = "c";  // what may come next within the unit
  CHECK(dev.log[0].kind == 'b', "the log starts with '%c'", dev.log[0].kind);
  for (size_t x = 1; x < dev.log.size(); x++) {
    const Op& o = dev.log[x];
    if (o.kind == 'q') { CHECK(nret < u && o.a == nret % slots, "op %zu: a query of slot %zu", x, o.a); continue; }
    if (o.kind == 'r') { CHECK(o.a == nret && nret < u, "op %zu: unit %zu retired", x, o.a); ++nret; continue; }
    CHECK(u < nu, "op %zu '%c' after the last unit", x, o.kind);
    const size_t base = (u % slots) * pl.slot_bytes + pl.data_off;
    if (o.kind == 'c') {
      CHECK(*want == 'c', "op %zu: a copy of unit %zu after its join", x, u);
      CHECK(o.a == (pl.copy_streams > 1 ? ncopies & 1 : 0) && o.b == base + sent && o.c > 0, "op %zu: copy k %zu at %zu", x, o.a, o.b);
      sent += o.c;
      ++ncopies;
      continue;
    }
    if (*want == 'c') {  // the unit's copies are over: all of its bytes sent, to the 16-byte round-up at most
      CHECK(sent >= pl.usend[u] && sent <= ((pl.usend[u] + 15) & ~(uint64_t)15), "unit %zu: %llu of %llu bytes sent",
            u, (unsigned long long)sent, (unsigned long long)pl.usend[u]);
      want = pl.copy_streams > 1 ? "jlkid" : "lkid";
    }
    CHECK(o.kind == *want, "op %zu: '%c' where unit %zu wants '%c'", x, o.kind, u, *want);
    if ((o.kind == 'l' || o.kind == 'i') && o.a != u) CHECK(false, "op %zu: callback of unit %zu in unit %zu", x, o.a, u);
    if (o.kind == 'd') {
      CHECK(o.a == u % slots && u < nret + slots, "op %zu: done of slot %zu for unit %zu", x, o.a, u);
      ++u;
      sent = 0;
      want = "c";
    } else {
      ++want;
    }
  }
  CHECK(u == nu && nret == nu, "(d) the log ends after %zu units, %zu retired", u, nret);
  return 0;
}

static int test_engine() {
  std::mt19937 rng(11);
  HostPool pool;
  size_t pieces = 0;
  for (int round = 0; round < 45; round++) {
    const uint64_t piece = round % 3 == 0 ? 8 : round % 3 == 1 ? 16 : 32;
    Job job = make_job(rng, piece, 40 + rng() % 160);
    job.pl.threads = 2 + round % 15;  // 1 to 15 readers
    job.pl.pump_on_pool = (round / 15) % 2 == 0;
    job.pl.pump_reads = round % 4 != 3;
    job.pl.copy_streams = round % 5 == 4 ? 1 : 2;
    job.pl.slots = round % 7 == 6 ? 2 : 3;
    pieces += job.pl.pieces();
    if (run_job(pool, job, rng, -1)) { printf("round %d (clean)\n", round); return 1; }
    // (f): fail one operation of those a clean run makes (setup, a copy, a join, a callback, a
    // done, a query), then show the pool still runs a whole job
    const long fail_at = round == 0 ? 0 : (long)(rng() % min_ops(job));
    if (run_job(pool, job, rng, fail_at)) { printf("round %d (failure at %ld)\n", round, fail_at); return 1; }
    if (run_job(pool, job, rng, -1)) { printf("round %d (after the failure)\n", round); return 1; }
  }
  CHECK(pieces > 3000, "only %zu pieces", pieces);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: piece_queue_test <scratch directory>\n"); return 2; }
  if (test_cutter() || test_reader(argv[1]) || test_engine()) return 1;
  printf("piece queue ok\n");
  return 0;
}
