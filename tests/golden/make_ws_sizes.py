"""Generates tests/golden/ws_sizes.json: the workspace totals of commit PARENT, the last one
whose layouts were spelled out by hand (a `*_bytes()` sum next to a chain of pointer bumps).
tests/test_ws_layout_cpu.py holds every later library to these totals.  The file is a record:
it is not re-made from a newer library.

Two sources, kept apart in the file:
  * "exported":   the `S` lines of tests/native/ws_layout_test.cpp built with -DWS_SIZES_ONLY
                  and linked against PARENT's libsd_hip_cas.so (functions that commit exports).
                  Run:  python tests/golden/make_ws_sizes.py <that program's output file>
  * "by_formula": totals PARENT computed in static functions or inline, which no program can
                  call: its formulas, restated below from its source (file:line of PARENT;
                  group_hash.hip by the name of the function or constant), and
                  evaluated over the exported inputs (region_capacity, sort_workspace_bytes, ...).
"""
from __future__ import annotations

import json
import os
import sys

PARENT = "7f8fb288376fb527e794d113ce166be80f829cc9"
HERE = os.path.dirname(os.path.abspath(__file__))

NS = [1, 255, 256, 257, 4095, 4096, 4097, 65536, 1441792, 1441793, 12500000, 40000001, 2 ** 32 - 1]
TARGETS = [0, 1, 16]
REGIONS = 256                                      # sd_mix.h
TARGET_PER_BUCKET, MAX_BITS, MAX_B2 = 1536, 19, 9  # group_hash.hip, constants of the same names
BIG_MAX_KEYS, COARSE10_KEYS = 256 * 5632, 40_000_000  # (the same)
OBJ_SHARDS, OBJ_STRIDE, TOTALS_REPL, STAGED_MAX_NB = 64, 16, 16, 1024  # (the same)
TOP_BINS, TOP_SEL_WORDS = 65, 4                    # sd_object_stats.h:27,28


def al(x):
    return (x + 255) // 256 * 256


def group_plan(n, target):  # group_hash.hip group_plan() -> (l1.nb, nb())
    target = target or TARGET_PER_BUCKET
    bits = 1
    while bits < MAX_BITS and (1 << bits) * target < n:
        bits += 1
    cb = 8 if n <= COARSE10_KEYS else 10
    b1 = bits if bits < cb else (bits - MAX_B2 if bits - cb > MAX_B2 else cb)
    b2 = bits - b1
    if b2 > 0 and n <= BIG_MAX_KEYS:
        b2 = 0
    return 1 << b1, 1 << (b1 + b2)


def region_capacity_nb(n, nb):  # group_hash.hip region_capacity_nb() (doubles, as there)
    mean = n / nb
    var = mean * (1.0 - 1.0 / nb)
    sd = 1
    while float(sd * sd) < var:
        sd += 1
    return int(mean) + 1 + 8 * sd + 64


def by_formula(ex):
    out = {}
    sort = lambda n: ex[f"sort_workspace_bytes({n})"]  # noqa: E731
    for n in NS:
        rows = REGIONS * ex[f"region_capacity({n})"]
        # group_hash.hip small_regions_bytes() (since then: small_regions_layout)
        out[f"small_regions({n})"] = (al(rows * 8) + al(rows * 4) + al(2 * n * 8) + al(2 * n * 4) + 256 +
                                      al(n * 8) + al(n * 4))
        # group_hash.hip big_regions_bytes() (since then: big_regions_layout)
        nb1, nb = group_plan(n, 0)
        rows = nb1 * region_capacity_nb(n, nb1)
        out[f"big_regions({n})"] = (al(rows * 8) + al(rows * 4) + 2 * (al(n * 8) + al(n * 4)) + al(nb * 4) +
                                    al(OBJ_SHARDS * OBJ_STRIDE * 8) + al(2 * n * 8) + al(2 * n * 4))
        for t in TARGETS:  # the `chain` term of group_hash.hip hash_group_workspace_bytes()
            nb1, nb = group_plan(n, t)
            repl = TOTALS_REPL if nb1 <= STAGED_MAX_NB else 1
            out[f"hash_chain({n},{t})"] = (2 * (al(n * 8) + al(n * 4)) + al(repl * nb1 * 4) + al(nb1 * 4) +
                                           al(nb * 4) + al(OBJ_SHARDS * OBJ_STRIDE * 8) + al(2 * n * 8) +
                                           al(2 * n * 4))
        # validator_host.cpp:200,346
        out[f"reduce_cvs({n})"] = 2 * al((n + 255) // 256 * 32) + 512
        for G in (1, 8):  # bufs_bytes, sd_multi.cpp:67-70
            m = n // 2 + 3
            out[f"multi_bufs({n},{m},{G})"] = (al(n * 8) + al(n * 4) + al(n * 8) + al((G + 1) * 8) + al(n * 8) +
                                               al(m * 8) * 2 + al(m * 8) + al(m * 4) * 2 + al(m * 8) + 256)
        # top duplicates, sd_cas_top_duplicates_dev (now sd_top_layout, reports_host.cpp)
        small = al(TOP_BINS * 8) + al(TOP_SEL_WORDS * 8) + al(ex[f"top_scan_bytes({n})"])
        out[f"top({n},0)"] = small
        out[f"top({n},{n})"] = small + 2 * (al(n * 8) + al(n * 4)) + sort(n)
        # the duplicate report, sd_cas_duplicate_report (now sd_dup_report_layout, reports_host.cpp)
        b8, b4, b1 = al(n * 8), al(n * 4), al(n)
        for state, k in ((0, 0), (1, 1024)):
            bst = b1 + b8 + 2 * b4 + b8 if state else 0
            out[f"dup_report({n},{state},{k})"] = 2 * b8 + 2 * b4 + bst + al(k * 4) + al(k * 8) + 256
        for pre in (0, 1):
            for n_seed in (0, 5):
                m, steps = n + n_seed, (n + 99) // 100
                # the link emission's staging, sd_cas_identifier_links_ex_dev (now sd_link_staging_layout, links_host.cpp)
                b = (al(n * 4) + al(m * 8) + al(m * 4) + al(m * 4) + al(n * 8) + al((steps + 1) * 4) +
                     al(steps * 8) + 256)
                if pre:
                    b += (al(ex[f"pre_blocks({n})"] * 4) + al(ex[f"segmin_tiles_bytes({n})"]) +
                          al(ex["pre_filter_bytes(0)"]))
                out[f"link_staging({n},{n_seed},{steps},{pre})"] = b
                # its host arrays' device copies, sd_cas_identifier_links_ex (now sd_link_io_layout, links_host.cpp)
                out[f"link_io({n},{n_seed},{pre})"] = (al(n * 8) + 2 * al(n) + 2 * al(n * 4) + al(n_seed * 8) +
                                                       al(n_seed * 4) + (al(n * 4) if pre else 0))
    # object statistics, object_stats_impl (now sd_stats_layout, reports_host.cpp)
    out["stats()"] = al(ex["stats_shard_bytes(0)"]) + 256
    # the staged host batch, host_paths.cpp:191-195 (plan_batch :70,:73-74 for the two content sizes)
    for ns, np_ in ((0, 1), (1, 0), (100, 0), (37, 63)):
        for plen in (0, 1, 127, 128, 102400):
            n = ns + np_
            sampled, packed = ns * 57344, np_ * ((plen + 127) // 128 * 128) + 16
            out[f"staged({ns},{np_},{plen})"] = (sampled + al(packed) + al((ns + np_) * 8) + al(np_ * 8) +
                                                 al(np_ * 4) + al(n * 8))
    return out


def main():
    ex = {}
    with open(sys.argv[1]) as f:
        for ln in f:
            kind, key, val = ln.split()
            assert kind == "S"
            ex[key] = int(val)
    doc = {"parent_commit": PARENT, "exported": ex, "by_formula": by_formula(ex)}
    with open(os.path.join(HERE, "ws_sizes.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(ex), "exported,", len(doc["by_formula"]), "by formula")


if __name__ == "__main__":
    main()
