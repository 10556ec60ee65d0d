// links_host.cpp — the Object-link emission of the C ABI (include/sd_hip_cas.h) over links.hip:
// which rows of an identifier job create an Object, which link to one, and each job step's
// counts (file_identifier_job.rs:180-236, mod.rs:98-350).
#include "ctx_internal.h"
#include "sd_group.h"
#include "sd_links.h"

using namespace sdcas;

static_assert(SD_CAS_ROW_HASHED == SD_LINKS_HASHED && SD_CAS_ROW_NO_CAS == SD_LINKS_NO_CAS &&
                  SD_CAS_ROW_ERROR == SD_LINKS_ERROR && SD_CAS_LINK_CREATED == SD_LINKS_CREATED &&
                  SD_CAS_LINK_LINKED == SD_LINKS_LINKED && SD_CAS_LINK_DROPPED == SD_LINKS_DROPPED &&
                  SD_CAS_LINK_NOT_REACHED == SD_LINKS_NOT_REACHED &&
                  SD_CAS_LINK_EXISTING == SD_LINKS_EXISTING &&
                  SD_CAS_NO_STEP == SD_LINKS_NO_STEP && SD_CAS_NO_OBJECT == SD_LINKS_NO_OBJECT,
              "link constants");

extern "C" {

size_t sd_cas_identifier_max_steps(size_t n, uint32_t chunk) {
  return chunk ? (n + chunk - 1) / chunk : 0;
}

// the link emission's staging: rep | hkeys | hrows | minrow | orphans | starts | counts |
// [event block offsets | scan tiles | key filter] | 4 counters (hashed rows, orphan rows, waves
// with a bad Object id, events); the seeded grouping runs over the n hashed rows + the n_seed
// existing Objects' keys.  The bracketed sections serve rows with pre-existing Objects (pre) and
// take no room without them; such rows reuse the grouping's buffers once it is done: events
// (hkeys / hrows), sorted events (orphans / minrow), scan elements (hkeys).
LinkStagingWs sd_link_staging_layout(void* base, size_t n, size_t n_seed, size_t steps_total, bool pre) {
  const size_t m = n + n_seed;
  WsCarve w(base);  LinkStagingWs L;
  L.rep = w.take<uint32_t>(n);  L.hkeys = w.take<uint64_t>(m);
  L.hrows = w.take<uint32_t>(m);  L.minrow = w.take<uint32_t>(m);
  L.orphans = w.take<uint64_t>(n);  L.starts = w.take<uint32_t>(steps_total + 1);
  L.counts = w.take<uint32_t>(2 * steps_total);  L.boff = w.take<uint32_t>(pre ? pre_blocks(n) : 0);
  L.tiles = w.take<uint64_t>(pre ? segmin_tiles_bytes(n) / 8 : 0);
  L.filter = w.take<uint32_t>(pre ? pre_filter_bytes() / 4 : 0);  L.counters = w.take<uint64_t>(4);
  L.bytes = w.bytes();  return L;
}
// the host forms' device copies of their arrays (c->io)
LinkIoWs sd_link_io_layout(void* base, size_t n, size_t n_seed, bool pre) {
  WsCarve w(base);  LinkIoWs L;
  L.keys = w.take<uint64_t>(n);  L.state = w.take<uint8_t>(n);
  L.step = w.take<uint32_t>(n);  L.object = w.take<uint32_t>(n);
  L.action = w.take<uint8_t>(n);  L.seed_keys = w.take<uint64_t>(n_seed);
  L.seed_objects = w.take<uint32_t>(n_seed);  L.pre = pre ? w.take<uint32_t>(n) : nullptr;
  L.bytes = w.bytes();  return L;
}

}  // extern "C"

// The emission behind every device form.  The Objects that exist before the job come either as
// seed arrays, grouped together with the rows, or (index != NULL, no seeds) from a
// library-resident Object index: then the rows are grouped alone and every hashed row's minimum is
// lowered to its key's id in the index, which gives the seeded grouping's result for seeds = the
// index's pairs (an id is below every ROW_FLAG | row, SD_CAS_NO_OBJECT above).
static int links_emit(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state, size_t n,
                      uint32_t chunk, const uint64_t* d_seed_keys, const uint32_t* d_seed_objects,
                      size_t n_seed, const uint32_t* index, const uint32_t* d_pre_objects,
                      uint32_t* d_step, uint32_t* d_object, uint8_t* d_action, uint64_t* h_step_counts,
                      size_t max_steps, uint64_t* out_steps, void* stream) {
  if (!c) return SD_CAS_EINVAL;
  const size_t steps_total = sd_cas_identifier_max_steps(n, chunk);
  if (chunk == 0 || n >= (1ull << 32) || !out_steps || max_steps < steps_total ||
      (n && (!d_keys || !d_step || !d_object || !d_action || !h_step_counts)) ||
      (n_seed && (!d_seed_keys || !d_seed_objects)))
    return fail(c, SD_CAS_EINVAL, "identifier_links: bad arguments");
  if (index && !sd_index_alive(c, *index)) return fail(c, SD_CAS_EINVAL, "identifier_links: no index %u", *index);
  // a seeded grouping tags rows with LINKS_ROW_FLAG: rows and Object ids below 2^31 (rows
  // that already own an Object run the seeded grouping too, and so do rows read against an index)
  const bool seeded = n_seed > 0 || d_pre_objects || index;
  if (seeded && (n >= LINKS_ROW_FLAG || n_seed >= LINKS_ROW_FLAG || n + n_seed >= (1ull << 32)))
    return fail(c, SD_CAS_EINVAL, "identifier_links: %zu rows + %zu existing Objects exceed 2^31",
                n, n_seed);
  *out_steps = 0;
  for (size_t k = 0; k < 2 * steps_total; k++) h_step_counts[k] = 0;
  if (n == 0) return SD_CAS_OK;
  hipStream_t s = pick(c, stream);
  // (this call is blocking)
  int rc = ensure(c, c->staging,
                  sd_link_staging_layout(nullptr, n, n_seed, steps_total, d_pre_objects != nullptr).bytes);
  if (rc) return rc;
  const LinkStagingWs L = sd_link_staging_layout(c->staging.p, n, n_seed, steps_total, d_pre_objects != nullptr);
  // 1. grouping over the hashed rows (rep = the key's first row; seeded: the lowest existing
  //    Object id when the key has one — mod.rs:180-198 finds Objects by cas over the whole
  //    library), and the rows that stay orphan after being processed (they steer the cursor)
  std::vector<uint64_t> stay;  // row << 8 | state, ascending
  if (d_state || seeded) {
    uint64_t cnt[3] = {0, 0, 0};
    HIP_TRY(c, hipMemsetAsync(L.counters, 0, 32, s));
    HIP_TRY(c, links_check_ids(d_seed_objects, n_seed, false, L.counters + 2, s));
    if (d_pre_objects) HIP_TRY(c, links_check_ids(d_pre_objects, n, true, L.counters + 2, s));
    HIP_TRY(c, links_split(d_keys, d_state, n, L.hkeys, L.hrows, L.counters, L.orphans, L.counters + 1,
                           seeded ? LINKS_ROW_FLAG : 0u, s));
    HIP_TRY(c, hipMemcpyAsync(cnt, L.counters, 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (cnt[2])
      return fail(c, SD_CAS_EINVAL, "identifier_links: an existing Object id is >= 2^31");
    stay.resize(cnt[1]);
    if (cnt[1]) {
      HIP_TRY(c, hipMemcpyAsync(stay.data(), L.orphans, cnt[1] * 8, hipMemcpyDeviceToHost, s));
    }
    if (n_seed) {  // the existing Objects' (cas key, id) pairs after the hashed rows
      HIP_TRY(c, hipMemcpyAsync(L.hkeys + cnt[0], d_seed_keys, n_seed * 8, hipMemcpyDeviceToDevice, s));
      HIP_TRY(c, hipMemcpyAsync(L.hrows + cnt[0], d_seed_objects, n_seed * 4, hipMemcpyDeviceToDevice, s));
    }
    if (cnt[0]) {
      if ((rc = sd_cas_group_min_dev(c, L.hkeys, L.hrows, cnt[0] + n_seed, L.minrow, nullptr, s))) return rc;
      if (index && (rc = sd_index_lookup_min(c, *index, L.hkeys, cnt[0], L.minrow, s))) return rc;
      HIP_TRY(c, links_scatter(L.minrow, L.hrows, cnt[0], L.rep, seeded ? LINKS_ROW_FLAG : 0u, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    std::sort(stay.begin(), stay.end());
  } else {
    if ((rc = sd_cas_group_dev(c, d_keys, n, L.rep, nullptr, s))) return rc;
  }
  // 2. the cursor walk (host; O(steps + orphans)): step k covers [start, start + chunk);
  //    the next cursor is its last row, which the next query returns again iff it is
  //    still orphan; an empty query ends the job
  // the rows asked about only increase (each step's last row), so one forward pointer into
  // the sorted orphan list answers them all: O(steps + orphans) (a binary search per step
  // cost ~2 ms of a 10 M-row job)
  size_t sp = 0;
  auto stays = [&](uint64_t row, uint8_t* st) {
    while (sp < stay.size() && (stay[sp] >> 8) < row) ++sp;
    if (sp == stay.size() || (stay[sp] >> 8) != row) return false;
    *st = (uint8_t)(stay[sp] & 0xFF);
    return true;
  };
  std::vector<uint32_t> h_starts;
  h_starts.reserve(steps_total + 1);
  std::vector<uint64_t> extra(steps_total, 0);  // re-queried empty rows: one creation per step
  uint64_t start = 0, reached = 0;
  for (size_t k = 0; k < steps_total && start < n; k++) {
    h_starts.push_back((uint32_t)start);
    const uint64_t end = std::min<uint64_t>(start + chunk, n), last = end - 1;
    reached = end;
    uint8_t st = 0;
    if (stays(last, &st)) {
      if (st == SD_CAS_ROW_NO_CAS && k + 1 < steps_total) extra[k] += 1;
      start = last;
    } else {
      start = end;
    }
  }
  const size_t nsteps = h_starts.size();
  h_starts.push_back(0xFFFFFFFFu);  // sentinel
  HIP_TRY(c, hipMemcpyAsync(L.starts, h_starts.data(), h_starts.size() * 4, hipMemcpyHostToDevice, s));
  // 3. rows that already own an Object (links.hip, sd_links_pre_*): the events — hashed rows
  //    of the reached steps that hold an Object — compacted in row order, sorted stably by key,
  //    and scanned; each hashed row then looks its key up in the decision kernel
  uint64_t n_ev = 0;
  if (d_pre_objects) {
    HIP_TRY(c, links_pre_count(d_state, d_pre_objects, reached, L.boff, L.counters + 3, s));
    HIP_TRY(c, hipMemcpyAsync(&n_ev, L.counters + 3, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  if (n_ev) {
    HIP_TRY(c, hipMemsetAsync(L.filter, 0, pre_filter_bytes(), s));
    HIP_TRY(c, links_pre_emit(d_keys, d_state, d_pre_objects, reached, L.boff, L.hkeys, L.hrows, L.filter, s));
    uint64_t* skeys = L.orphans;
    uint32_t* srows = L.minrow;
    if ((rc = sd_cas_sort_pairs_dev(c, L.hkeys, L.hrows, n_ev, skeys, srows, 0, 64, s))) return rc;
    HIP_TRY(c, links_pre_scan(skeys, srows, d_pre_objects, n_ev, L.starts, (uint32_t)nsteps, L.hkeys,
                              L.tiles, s));
  }
  // 4. per-row decisions + per-step counts (device)
  HIP_TRY(c, hipMemsetAsync(L.counts, 0, std::max<size_t>(nsteps, 1) * 8, s));
  HIP_TRY(c, links_decide(d_state, L.rep, n, L.starts, (uint32_t)nsteps, reached, d_step, d_object,
                          d_action, L.counts, seeded, d_keys, L.orphans, L.minrow, L.hkeys, L.filter, n_ev,
                          (uint32_t)chunk, s));
  std::vector<uint32_t> hc(2 * std::max<size_t>(nsteps, 1));
  HIP_TRY(c, hipMemcpyAsync(hc.data(), L.counts, hc.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  for (size_t k = 0; k < nsteps; k++) {
    h_step_counts[2 * k] = hc[2 * k] + extra[k];
    h_step_counts[2 * k + 1] = hc[2 * k + 1];
  }
  *out_steps = nsteps;
  return SD_CAS_OK;
}

extern "C" {

int sd_cas_identifier_links_ex_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                   size_t n, uint32_t chunk, const uint64_t* d_seed_keys,
                                   const uint32_t* d_seed_objects, size_t n_seed,
                                   const uint32_t* d_pre_objects, uint32_t* d_step,
                                   uint32_t* d_object, uint8_t* d_action, uint64_t* h_step_counts,
                                   size_t max_steps, uint64_t* out_steps, void* stream) {
  return links_emit(c, d_keys, d_state, n, chunk, d_seed_keys, d_seed_objects, n_seed, nullptr,
                    d_pre_objects, d_step, d_object, d_action, h_step_counts, max_steps, out_steps, stream);
}

int sd_cas_identifier_links_indexed_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                        size_t n, uint32_t chunk, uint32_t index,
                                        const uint32_t* d_pre_objects, uint32_t* d_step,
                                        uint32_t* d_object, uint8_t* d_action, uint64_t* h_step_counts,
                                        size_t max_steps, uint64_t* out_steps, void* stream) {
  return links_emit(c, d_keys, d_state, n, chunk, nullptr, nullptr, 0, &index, d_pre_objects, d_step,
                    d_object, d_action, h_step_counts, max_steps, out_steps, stream);
}

int sd_cas_identifier_links_seeded_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                       size_t n, uint32_t chunk, const uint64_t* d_seed_keys,
                                       const uint32_t* d_seed_objects, size_t n_seed, uint32_t* d_step,
                                       uint32_t* d_object, uint8_t* d_action, uint64_t* h_step_counts,
                                       size_t max_steps, uint64_t* out_steps, void* stream) {
  return sd_cas_identifier_links_ex_dev(c, d_keys, d_state, n, chunk, d_seed_keys, d_seed_objects,
                                        n_seed, nullptr, d_step, d_object, d_action, h_step_counts,
                                        max_steps, out_steps, stream);
}

int sd_cas_identifier_links_dev(sd_cas_ctx* c, const uint64_t* d_keys, const uint8_t* d_state,
                                size_t n, uint32_t chunk, uint32_t* d_step, uint32_t* d_object,
                                uint8_t* d_action, uint64_t* h_step_counts, size_t max_steps,
                                uint64_t* out_steps, void* stream) {
  return sd_cas_identifier_links_seeded_dev(c, d_keys, d_state, n, chunk, nullptr, nullptr, 0, d_step,
                                            d_object, d_action, h_step_counts, max_steps, out_steps,
                                            stream);
}

}  // extern "C"

// the host forms: the rows (and seeds) staged in c->io, links_emit, the decisions copied back
static int links_emit_host(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state, size_t n,
                           uint32_t chunk, const uint64_t* h_seed_keys, const uint32_t* h_seed_objects,
                           size_t n_seed, const uint32_t* index, const uint32_t* h_pre_objects,
                           uint32_t* h_step, uint32_t* h_object, uint8_t* h_action,
                           uint64_t* h_step_counts, size_t max_steps, uint64_t* out_steps) {
  if (!c) return SD_CAS_EINVAL;
  if ((n && (!h_keys || !h_step || !h_object || !h_action)) ||
      (n_seed && (!h_seed_keys || !h_seed_objects)))
    return fail(c, SD_CAS_EINVAL, "identifier_links: bad arguments");
  for (size_t j = 0; j < n_seed; j++)
    if (h_seed_objects[j] >= LINKS_ROW_FLAG)
      return fail(c, SD_CAS_EINVAL, "identifier_links: existing Object id %u >= 2^31", h_seed_objects[j]);
  if (h_pre_objects)
    for (size_t i = 0; i < n; i++)
      if (h_pre_objects[i] >= LINKS_ROW_FLAG && h_pre_objects[i] != SD_CAS_NO_OBJECT)
        return fail(c, SD_CAS_EINVAL, "identifier_links: row %zu's Object id %u >= 2^31", i,
                    h_pre_objects[i]);
  if (n == 0 || n >= (1ull << 32))
    return links_emit(c, nullptr, nullptr, n, chunk, nullptr, nullptr, 0, index, nullptr, nullptr, nullptr,
                      nullptr, h_step_counts, max_steps, out_steps, c->stream);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure(c, c->io, sd_link_io_layout(nullptr, n, n_seed, h_pre_objects != nullptr).bytes);
  if (rc) return rc;
  const LinkIoWs L = sd_link_io_layout(c->io.p, n, n_seed, h_pre_objects != nullptr);
  uint8_t* d_state = h_state ? L.state : nullptr;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(L.keys, h_keys, n * 8, hipMemcpyHostToDevice, s));
  if (h_state) HIP_TRY(c, hipMemcpyAsync(d_state, h_state, n, hipMemcpyHostToDevice, s));
  if (n_seed) {
    HIP_TRY(c, hipMemcpyAsync(L.seed_keys, h_seed_keys, n_seed * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(L.seed_objects, h_seed_objects, n_seed * 4, hipMemcpyHostToDevice, s));
  }
  if (L.pre) HIP_TRY(c, hipMemcpyAsync(L.pre, h_pre_objects, n * 4, hipMemcpyHostToDevice, s));
  rc = links_emit(c, L.keys, d_state, n, chunk, L.seed_keys, L.seed_objects, n_seed, index, L.pre, L.step,
                  L.object, L.action, h_step_counts, max_steps, out_steps, s);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(h_step, L.step, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(h_object, L.object, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(h_action, L.action, n, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SD_CAS_OK;
}

extern "C" {

int sd_cas_identifier_links_ex(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                               size_t n, uint32_t chunk, const uint64_t* h_seed_keys,
                               const uint32_t* h_seed_objects, size_t n_seed,
                               const uint32_t* h_pre_objects, uint32_t* h_step, uint32_t* h_object,
                               uint8_t* h_action, uint64_t* h_step_counts, size_t max_steps,
                               uint64_t* out_steps) {
  return links_emit_host(c, h_keys, h_state, n, chunk, h_seed_keys, h_seed_objects, n_seed, nullptr,
                         h_pre_objects, h_step, h_object, h_action, h_step_counts, max_steps, out_steps);
}

int sd_cas_identifier_links_indexed(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                                    size_t n, uint32_t chunk, uint32_t index,
                                    const uint32_t* h_pre_objects, uint32_t* h_step, uint32_t* h_object,
                                    uint8_t* h_action, uint64_t* h_step_counts, size_t max_steps,
                                    uint64_t* out_steps) {
  return links_emit_host(c, h_keys, h_state, n, chunk, nullptr, nullptr, 0, &index, h_pre_objects, h_step,
                         h_object, h_action, h_step_counts, max_steps, out_steps);
}

int sd_cas_identifier_links_seeded(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                                   size_t n, uint32_t chunk, const uint64_t* h_seed_keys,
                                   const uint32_t* h_seed_objects, size_t n_seed, uint32_t* h_step,
                                   uint32_t* h_object, uint8_t* h_action, uint64_t* h_step_counts,
                                   size_t max_steps, uint64_t* out_steps) {
  return sd_cas_identifier_links_ex(c, h_keys, h_state, n, chunk, h_seed_keys, h_seed_objects, n_seed,
                                    nullptr, h_step, h_object, h_action, h_step_counts, max_steps,
                                    out_steps);
}

int sd_cas_identifier_links(sd_cas_ctx* c, const uint64_t* h_keys, const uint8_t* h_state,
                            size_t n, uint32_t chunk, uint32_t* h_step, uint32_t* h_object,
                            uint8_t* h_action, uint64_t* h_step_counts, size_t max_steps,
                            uint64_t* out_steps) {
  return sd_cas_identifier_links_seeded(c, h_keys, h_state, n, chunk, nullptr, nullptr, 0, h_step,
                                        h_object, h_action, h_step_counts, max_steps, out_steps);
}

}  // extern "C"
