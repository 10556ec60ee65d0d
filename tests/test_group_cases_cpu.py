"""CPU tests of the hash grouping's edge cases (tests/group_cases.py): the restated constants
match the sources, np_unmix64 inverts the mix, the capacity matches the golden workspace record,
and — by the model, from the keys alone — every case takes the chain and reaches the exits it is
named for, every reachable exit of every chain is reached, every x / x + 1 pair lands on opposite
sides, and the numpy reference is self-consistent.  These are conditions on the inputs: the GPU
tests (tests/test_group_edges_gpu.py) run the same cases and rely on them.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

from tests import group_cases as gc
from tests.golden import make_ws_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_mirror_sources():
    s = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "group_hash.hip")).read()
    mix = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "sd_mix.h")).read()

    def const(name, text=s):
        return int(re.search(rf"constexpr \w+ {name} = (\d+)[u;]", text).group(1))
    assert f"#define SD_REGION_BITS {gc.REGION_BITS}" in mix and "REGIONS = 1u << REGION_BITS" in mix
    assert "0xBF58476D1CE4E5B9ull" in mix and "0x94D049BB133111EBull" in mix
    assert "(z ^ (z >> 30))" in mix and "(z ^ (z >> 27))" in mix and "z ^ (z >> 31)" in mix
    assert const("RPART_THREADS") * const("RPART_ITEMS") == gc.RPART_TILE
    assert const("RBIG_THREADS") * const("RBIG_ITEMS") == gc.RBIG_TILE
    assert const("TABLE") == gc.TABLE and const("MIN_THREADS") * const("MIN_ITEMS") == gc.TRIP
    assert const("BIG_TABLE") == gc.BIG_TABLE and const("BIG_THREADS") * const("ITEMS") == gc.BIG_TRIP
    assert "REG_TABLE = REGION_BITS >= 9 ? 6144 : BIG_TABLE" in s
    assert "REG_THREADS = REGION_BITS >= 9 ? 512 : BIG_THREADS" in s and "REG_ITEMS = REGION_BITS >= 9 ? 7 : ITEMS" in s
    assert "fill_limit < TBL / 8 * 7 ? fill_limit : TBL / 8 * 7" in s
    assert (gc.FILL, gc.BIG_FILL) == (3584, 10752)
    assert "BIG_MAX_KEYS = 256ull * 5632" in s and gc.BIG_MAX_KEYS == 1_441_792
    assert const("TARGET_PER_BUCKET") == gc.TARGET_PER_BUCKET and const("MAX_BITS") == gc.MAX_BITS
    assert const("MAX_B2") == gc.MAX_B2 and const("COARSE10_KEYS") == gc.COARSE10_KEYS
    assert const("RBIG_MAX_NB") == gc.RBIG_MAX_NB
    assert "return (uint32_t)(((k & 0xFFFFFFFFull) * TBL) >> 32);" in s     # home_slot, 12,288 slots
    assert "(kk & 0xFFFFFFFFull) % cap" in s and "cap = 2 * m" in s          # global home, cap = 2m
    assert ((gc.HOME_LAST_LOW32 * gc.BIG_TABLE) >> 32) == gc.BIG_TABLE - 1
    assert (((gc.HOME_LAST_LOW32 - 1) * gc.BIG_TABLE) >> 32) == gc.BIG_TABLE - 2
    assert "if (target == 0 && n > 0 && n <= BIG_MAX_KEYS) return Chain::SmallRegions;" in s
    assert "if (target == 0 && !g.big && g.b2 > 0 && g.l1.nb <= RBIG_MAX_NB) return Chain::BigRegions;" in s


def test_unmix_round_trips():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 63, 1_000_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 1_000_000, dtype=np.uint64)
    x[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    assert (gc.np_mix64(gc.np_unmix64(x)) == x).all() and (gc.np_unmix64(gc.np_mix64(x)) == x).all()
    from oracle.pyoracle import np_mix64                     # the oracle's own statement of the mix
    assert (np_mix64(x[:1000]) == gc.np_mix64(x[:1000])).all()
    # the scalar inverse the older grouping tests use
    from tests.test_gpu_parity import unmix64
    assert [unmix64(int(v)) for v in x[:50]] == gc.np_unmix64(x[:50]).tolist()


def test_capacity_matches_the_golden_record():
    """region_capacity(n) of tests/golden/ws_sizes.json — exported by the library the record was
    made from and held to every later one by tests/native/ws_layout_test.cpp."""
    with open(os.path.join(ROOT, "tests", "golden", "ws_sizes.json")) as f:
        ex = json.load(f)["exported"]
    seen = 0
    for k, v in ex.items():
        mo = re.fullmatch(r"region_capacity\((\d+)\)", k)
        if mo:
            assert gc.region_capacity(int(mo.group(1))) == v, k
            seen += 1
    assert seen >= 10
    assert gc.region_capacity(20_000) == 215 and gc.region_capacity(gc.BIG_MAX_KEYS) == 6297
    for n in make_ws_sizes.NS:
        for t in make_ws_sizes.TARGETS:
            b1, b2, _ = gc.group_plan(n, t)
            assert make_ws_sizes.group_plan(n, t) == (1 << b1, 1 << (b1 + b2)), (n, t)


def test_dispatch():
    assert gc.pick_chain(20_000, 0) == ("S", 8) and gc.pick_chain(gc.BIG_MAX_KEYS, 0) == ("S", 8)
    assert gc.pick_chain(gc.BIG_MAX_KEYS + 1, 0) == ("B", 10)
    assert gc.pick_chain(20_000, 1300) == ("T-fine", 4) and gc.pick_chain(30_000, 16) == ("T-big", 8)


@pytest.mark.parametrize("case_id", list(gc.CASES))
def test_case_reaches_what_it_claims(case_id):
    c = gc.build(case_id)
    m = gc.model(c["keys"], c["target"])
    want_chain = case_id.split("-")[0] + ("-" + case_id.split("-")[1] if case_id.startswith("T-") else "")
    assert m["chain"] == want_chain
    for b, e in c["claims"].items():
        assert m["exit"][b] == e, (case_id, b, m["exit"][b], e, int(m["rows"][b]), int(m["distinct"][b]))
    f = c["facts"]
    if "spill" in f:
        assert m["total_spill"] == f["spill"]
    if "full" in f:
        assert int(m["full"].sum()) == f["full"]
    for b, t in f.get("trips", {}).items():
        assert m["trips"][b] == t
    for b, r in f.get("span", {}).items():
        assert m["span"][b] == r
    for b, r in f.get("region_rows", {}).items():
        assert m["region_rows"][b] == r
    if "carved" in f:
        assert m["carved"] == f["carved"] <= 2 * m["n"]
    if m["chain"] == "S":      # every full region is claimed; the overflow tables fit their 2n slots
        assert {b for b in range(gc.REGIONS) if m["full"][b]} == {b for b, e in c["claims"].items()
                                                                  if e not in ("one_trip", "empty")}
        assert m["carved"] <= 2 * m["n"]
    # the reference is self-consistent
    keys, rep, mins, vals = c["keys"], c["rep"], c["mins"], c["vals"]
    assert (keys[rep] == keys).all() and (rep <= np.arange(len(keys))).all()
    assert (rep[rep] == rep).all() and c["objects"] == int((rep == np.arange(len(keys))).sum()) == m["objects"]
    assert (mins <= vals).all() and (mins[rep] == mins).all()
    order = np.lexsort((vals, keys))
    firsts = np.r_[True, keys[order][1:] != keys[order][:-1]]
    assert (mins[order][firsts] == vals[order][firsts]).all()      # the minimum is a value of the key


def test_every_reachable_exit_is_reached():
    reached = {ch: set() for ch in gc.REACHABLE}
    for case_id in gc.CASES:
        c = gc.build(case_id)
        m = gc.model(c["keys"], c["target"])
        reached[m["chain"]] |= set(m["exit"])
        assert set(c["claims"].values()) <= set(m["exit"])
    assert reached == gc.REACHABLE
    # claim_fail cannot be forced on the 4,096-slot table: two trips fill it exactly
    assert gc.exit_of_segment(10 ** 6, 10 ** 6, gc.TABLE, gc.FILL, gc.TRIP) == "own_table"


def test_edge_pairs_split():
    for lo, hi, b in gc.EDGE_PAIRS:
        ml, mh = (gc.model(gc.build(c)["keys"], gc.build(c)["target"]) for c in (lo, hi))
        assert (ml["exit"][b], int(ml["trips"][b])) != (mh["exit"][b], int(mh["trips"][b])), (lo, hi)
        dr, dd = int(mh["rows"][b] - ml["rows"][b]), int(mh["distinct"][b] - ml["distinct"][b])
        assert (dr, dd) in ((1, 0), (0, 1)), (lo, hi, dr, dd)       # exactly one more row or key
    m0, m1 = (gc.model(gc.build(c)["keys"]) for c in ("S-region_at_cap-1", "S-region_at_cap+0"))
    assert m0["rows"][7] == m0["cap"] - 1 and m1["rows"][7] == m1["cap"] and not m1["full"].any()
    ms, mb = (gc.model(gc.build(c)["keys"]) for c in ("S-dispatch_edge", "B-dispatch_edge"))
    assert (ms["n"], mb["n"]) == (gc.BIG_MAX_KEYS, gc.BIG_MAX_KEYS + 1) and (ms["chain"], mb["chain"]) == ("S", "B")
    assert (gc.build("B-dispatch_edge")["keys"][:-1] == gc.build("S-dispatch_edge")["keys"]).all()


def test_placements_hold_for_every_reservation_order():
    """The order-dependent edges: what a case needs is true of the ROWS, whichever tile goes first."""
    T = gc.RPART_TILE
    for tiles in (2, 3):
        c = gc.build(f"S-fill_from_g_eq_cap-{tiles}tiles")
        cap = gc.region_capacity(len(c["keys"]))
        per_tile = np.bincount(np.flatnonzero(gc.np_mix64(c["keys"]) >> np.uint64(56) == 9) // T, minlength=5)
        assert per_tile.tolist() == [cap] * tiles + [0] * (5 - tiles)
    c = gc.build("S-fill_in_one_tile")
    rows = np.flatnonzero(gc.np_mix64(c["keys"]) >> np.uint64(56) == 11)
    assert (rows // T == 2).all() and len(rows) > gc.region_capacity(len(c["keys"]))
    # home slots
    c = gc.build("S-probe_wrap")
    mk = np.unique(gc.np_mix64(c["keys"]))
    mk = mk[mk >> np.uint64(56) == 33]
    assert len(mk) == 150 and ((((mk & np.uint64(0xFFFFFFFF)) * np.uint64(gc.BIG_TABLE)) >> np.uint64(32)) == 12287).all()
    c = gc.build("S-global_home_wrap")
    b, cap_g, cnt = c["facts"]["global_home_last"]
    mixed = gc.np_mix64(c["keys"])
    assert 2 * int((mixed >> np.uint64(56) == b).sum()) == cap_g
    mk = np.unique(mixed[mixed >> np.uint64(56) == b])
    assert int(((mk & np.uint64(0xFFFFFFFF)) % np.uint64(cap_g) == cap_g - 1).sum()) >= cnt
    for cid in ("S-trips-8192", "S-trips-8193", "T-big-rows8193"):
        mk = np.unique(gc.np_mix64(gc.build(cid)["keys"]))
        mk = mk[mk >> np.uint64(56) == (21 if cid[0] == "S" else 17)]
        assert int((mk & np.uint64(0xFFFFFFFF) >= gc.HOME_LAST_LOW32).sum()) >= 40
    # the sequences: H's rows rise from call to call, and region 60 holds nothing else
    H = None
    for w, (lo, hi) in {"A": (0, 10_000), "B": (10_000, 20_000), "D": (20_000, 30_000)}.items():
        c = gc.build(f"S-seq-{w}")
        rows = np.flatnonzero(gc.np_mix64(c["keys"]) >> np.uint64(56) == 60)
        assert lo <= rows.min() and rows.max() < hi and len(np.unique(c["keys"][rows])) == 1
        assert H is None or H == c["keys"][rows[0]]
        H = c["keys"][rows[0]]
    rows = np.flatnonzero(gc.build("S-seq-A2")["keys"] == H)
    assert np.bincount(rows // T, minlength=8).tolist()[:3] == [270, 270, 0] and gc.region_capacity(30_000) == 270
    for seq in gc.SEQUENCES.values():
        assert set(seq) <= set(gc.CASES)


def test_vals_edges_are_present():
    c = gc.build("S-vals_edges")
    keys, vals, mins = c["keys"], c["vals"], c["mins"]
    assert (vals == 0).any() and (vals == 0xFFFFFFFF).any()
    uniq, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    hot = np.flatnonzero(inv == np.argmax(cnt))
    assert len(hot) >= 2500 and vals[hot[-1]] == mins[hot[0]] == 7 and (vals[hot[:-1]] > 7).all()
    allmax = (mins == 0xFFFFFFFF)
    assert allmax.any() and np.bincount(inv[allmax]).max() > 1      # a repeated key whose minimum is 0xFFFFFFFF
