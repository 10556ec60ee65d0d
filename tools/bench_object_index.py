#!/usr/bin/env python3
"""Measurements of the library-resident Object index (sd_cas_index_*) on one
MI355X.  Three parts, each a text table on stdout and a JSON record in --out:

  sweep   10 M uniform keys at maximum load 30 / 50 / 70 % (SD_CAS_INDEX_LOAD_PERCENT, which a
          context reads when it is created: one engine per setting): insert, lookup of hits,
          lookup of misses, the table's bytes and its real load.
  rates   insert and lookup at 10^4, 1.31 M and 10 M keys, in keys/s and bytes per key.
  links   the point of the index: a 100-row step and a 1.31 M-row job against libraries of 10^4,
          10^6 and 10^7 (cas key, Object) pairs — the indexed call, the seeded call (device form,
          seeds already resident) and the fresh-library call on the same rows, alternated in one
          session, medians of --reps repetitions.

What a figure includes.  Every time is a host clock from a synchronised device to the next
synchronisation, after one untimed call of the same shape.  The index calls go through the Python
methods of ObjectIndex (tens of microseconds of argument checks: visible at 10^4 keys, where the
figure is launches and synchronisations, not the table).  insert includes its id check and the
wait for that verdict.  The link calls go through the C ABI directly with every buffer, the count
array included, allocated before the loop: what a C or Rust caller pays, that is the launches,
the kernels, the read-back of the per-step counts and the call's own final synchronisation.

The tables go to stdout and to bench_object_index.txt, the records to bench_object_index.json.
Usage: tools/bench_object_index.py [--out profiles/object_index] [--reps 20]
[--parts sweep,rates,links] [--keys 10000000]
"""
import ctypes
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacedrive_amd import CasEngine  # noqa: E402


def keys_dev(rng, n):
    return torch.from_numpy(rng.integers(0, 1 << 63, n, dtype=np.int64)).cuda()


LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn, reps, setup=None):
    """Median and all wall-clock times (ms) of fn(), each after setup() and a device sync and
    ending in one; one untimed call first."""
    out = []
    for k in range(reps + 1):
        if setup:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def index_times(eng, keys, ids, misses, reps, expected):
    """insert (into a cleared table sized for `expected`), lookup hits, lookup misses."""
    out = torch.empty(keys.numel(), dtype=torch.int32, device="cuda")
    with eng.object_index(expected) as ix:
        ins, _ = timed(lambda: ix.insert(keys, ids), reps, setup=ix.clear)
        st = ix.stats()
        ix.lookup(keys, out=out)
        assert bool((out == ids).all()), "lookup after insert disagrees"
        hit, _ = timed(lambda: ix.lookup(keys, out=out), reps)
        probe_hit = ix.stats()["last_max_probe"]
        miss, _ = timed(lambda: ix.lookup(misses, out=out), reps)
        probe_miss = ix.stats()["last_max_probe"]
        assert bool((out == -1).all()), "a miss was found"
    return dict(insert_ms=ins, hit_ms=hit, miss_ms=miss, slots=st["slots"], entries=st["entries"],
                table_mib=st["slots"] * 16 / 2 ** 20, load=st["entries"] / st["slots"],
                rehashes=st["rehashes"], max_probe_hit=probe_hit, max_probe_miss=probe_miss)


def part_sweep(_eng, args, rng):
    n = args.keys
    keys, misses = keys_dev(rng, n), keys_dev(rng, n) | (1 << 62) | 1
    keys &= ~(1 << 62)                      # hits and misses are disjoint by bit 62
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    rows = []
    say(f"# sweep: {n} uniform keys, medians of {args.reps}")
    say("max_load  slots      table_MiB  real_load  insert_ms  hit_ms   miss_ms  probe_hit  probe_miss")
    for pct in (30, 50, 70):
        os.environ["SD_CAS_INDEX_LOAD_PERCENT"] = str(pct)
        eng = CasEngine(0)                  # the knob is read here
        os.environ.pop("SD_CAS_INDEX_LOAD_PERCENT")
        r = dict(max_load_percent=pct, keys=n, **index_times(eng, keys, ids, misses, args.reps, n))
        eng.close()
        rows.append(r)
        say(f"{pct:7d}%  {r['slots']:9d}  {r['table_mib']:9.0f}  {r['load']:9.3f}  {r['insert_ms']:9.3f}  "
            f"{r['hit_ms']:7.3f}  {r['miss_ms']:7.3f}  {r['max_probe_hit']:9d}  {r['max_probe_miss']:10d}")
    return rows


def part_rates(eng, args, rng):
    rows = []
    say(f"# rates at the default load, medians of {args.reps}; bytes/key = the caller's arrays (12 B insert, "
        "12 B lookup) + one 16-B slot per probe, which is one 64-B sector of random HBM traffic")
    say("keys       insert_ms  insert_Mkeys/s  hit_ms   hit_Mkeys/s  miss_ms  miss_Mkeys/s  load")
    for n in (10_000, 1_310_720, args.keys):
        keys, misses = keys_dev(rng, n) & ~(1 << 62), keys_dev(rng, n) | (1 << 62)
        ids = torch.arange(n, dtype=torch.int32, device="cuda")
        r = dict(keys=n, **index_times(eng, keys, ids, misses, args.reps, n))
        rows.append(r)
        say(f"{n:9d}  {r['insert_ms']:9.4f}  {n / r['insert_ms'] / 1e3:14.1f}  {r['hit_ms']:7.4f}  "
            f"{n / r['hit_ms'] / 1e3:11.1f}  {r['miss_ms']:7.4f}  {n / r['miss_ms'] / 1e3:12.1f}  {r['load']:.3f}")
    return rows


def link_calls(eng, ix, empty, keys, sk, so, chunk=100):
    """The three calls on `keys` as closures over the C ABI, buffers allocated here: indexed,
    seeded (device form, seeds resident), fresh library; and indexed over an EMPTY index, which
    has to equal the fresh call (the check that all of them saw the same rows).  Each returns its
    (step, object, action) tensors and the per-step counts."""
    from spacedrive_amd.cas import _np_ptr, _ptr, _stream
    n = keys.numel()
    L, h = eng.L, eng.h
    ms = int(L.sd_cas_identifier_max_steps(n, chunk))

    def make(call):
        out = tuple(torch.empty(n, dtype=d, device="cuda") for d in (torch.int32, torch.int32, torch.uint8))
        counts, steps = np.zeros(2 * max(ms, 1), dtype=np.uint64), ctypes.c_uint64(0)
        tail = (None, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _np_ptr(counts), ms, ctypes.byref(steps),
                _stream(None))

        def run():
            rc = call(tail)
            assert rc == 0, L.sd_cas_last_error(h)
            return out, counts[:2 * int(steps.value)]
        return run

    def indexed(index):
        return lambda tail: L.sd_cas_identifier_links_indexed_dev(h, _ptr(keys), None, n, chunk,
                                                                  index._handle(eng), *tail)
    return {
        "indexed": make(indexed(ix)),
        "seeded": make(lambda tail: L.sd_cas_identifier_links_ex_dev(h, _ptr(keys), None, n, chunk, _ptr(sk),
                                                                     _ptr(so), sk.numel(), *tail)),
        "fresh": make(lambda tail: L.sd_cas_identifier_links_ex_dev(h, _ptr(keys), None, n, chunk, None, None,
                                                                    0, *tail)),
    }, make(indexed(empty))


def equal(a, b):
    return all(bool((x == y).all()) for x, y in zip(a[0], b[0])) and (a[1] == b[1]).all()


def part_links(eng, args, rng):
    rows = []
    say(f"# links: indexed vs seeded (device form, seeds resident) vs fresh library, alternated, medians of "
        f"{args.reps} (min-max of the indexed call); a third of the rows carry a key the library holds")
    say("rows      library   indexed_ms (min-max)         seeded_ms  fresh_ms  seeded/indexed  indexed-fresh_ms")
    for lib in (10_000, 1_000_000, 10_000_000):
        sk = keys_dev(rng, lib)
        so = torch.arange(lib, dtype=torch.int32, device="cuda")
        with eng.object_index(lib) as ix, eng.object_index() as empty:
            ix.insert(sk, so)
            for n in (100, 1_310_720):
                keys = keys_dev(rng, n)
                take = torch.from_numpy(rng.integers(0, lib, n)).cuda()
                held = torch.from_numpy(rng.random(n) < 1 / 3).cuda()
                keys = torch.where(held, sk[take], keys).contiguous()
                calls, on_empty = link_calls(eng, ix, empty, keys, sk, so)
                # same outputs on the same rows, which also warms every shape up
                assert equal(calls["indexed"](), calls["seeded"]()), "indexed != seeded"
                assert equal(on_empty(), calls["fresh"]()), "indexed over an empty index != fresh"
                times = {k: [] for k in calls}
                for _ in range(args.reps):
                    for k, fn in calls.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[k].append((time.perf_counter() - t0) * 1e3)
                med = {k: statistics.median(v) for k, v in times.items()}
                rows.append(dict(rows=n, library=lib, reps=args.reps, median_ms=med, all_ms=times))
                say(f"{n:8d}  {lib:8d}  {med['indexed']:10.4f} ({min(times['indexed']):.4f}-"
                    f"{max(times['indexed']):.4f})  {med['seeded']:9.4f}  {med['fresh']:8.4f}  "
                    f"{med['seeded'] / med['indexed']:14.2f}  {med['indexed'] - med['fresh']:16.4f}")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/object_index")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--parts", default="sweep,rates,links")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    eng = CasEngine(0)
    rng = np.random.default_rng(5)
    record = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    parts = {"sweep": part_sweep, "rates": part_rates, "links": part_links}
    for name in args.parts.split(","):
        record[name] = parts[name](eng, args, rng)
        sys.stdout.flush()
    with open(os.path.join(args.out, "bench_object_index.json"), "w") as fh:
        json.dump(record, fh, indent=1)
    with open(os.path.join(args.out, "bench_object_index.txt"), "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
