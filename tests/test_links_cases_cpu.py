"""CPU tests of the link emission's size-edge cases (tests/links_cases.py): for every generator
the vectorised closed form (cursor_walk + closed_form + closed_counts) equals the literal job
replay, and the edges the case claims — event count, `reached`, a value carried over each tile
and round edge of the sorted event list, a carry stopped at a key that starts on one, compaction
block edges, filter collisions, actions — hold, computed from the reference's answer alone.
These are conditions on the inputs: the GPU tests (tests/test_links_edges_gpu.py) run the same
cases and rely on them.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import links_cases as lc
from tests.golden.make_golden import closed_form, cursor_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lc.SEG_TILE


def test_constants_mirror_links_hip():
    s = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "links.hip")).read()
    a, b = map(int, re.search(r"SCAN_THREADS = (\d+), SCAN_ITEMS = (\d+);", s).groups())
    assert a * b == lc.SEG_TILE and a == lc.ROUND      # tile_prefix: SCAN_THREADS tiles a round
    assert "uint64_t SCAN_TILE = (uint64_t)SCAN_THREADS * SCAN_ITEMS;" in s
    a, b = map(int, re.search(r"EV_THREADS = (\d+), EV_ITEMS = (\d+);", s).groups())
    assert a * b == lc.EV_ROWS and "uint64_t EV_ROWS = (uint64_t)EV_THREADS * EV_ITEMS;" in s
    assert f"for (uint64_t base = 0; base < nb; base += {lc.ROUND})" in s    # sd_links_pre_bscan
    assert int(re.search(r"uint32_t FILTER_BITS = (\d+);", s).group(1)) == lc.FILTER_BITS
    assert f"key * 0x{lc.FILTER_MUL:016X}ull" in s
    assert (lc.FILTER_MUL * pow(lc.FILTER_MUL, -1, 1 << 64)) % (1 << 64) == 1


def solved(case_id):
    """(case, reference, step, starts, reached, geometry) with the closed form held to the
    reference (the literal replay for every case but many_blocks)."""
    case, (rstep, robj, ract, rcounts) = lc.build(case_id)
    keys, states, pre, seeds, chunk, _ = case
    step, starts, reached = cursor_walk(states, len(keys), chunk)
    obj, act = closed_form(keys, states, pre, seeds, step, starts)
    assert (step == rstep).all() and (obj == robj).all() and (act == ract).all()
    assert lc.closed_counts(states, step, starts, act, chunk) == rcounts
    return case, step, starts, reached, obj, act, lc.scan_geometry(case, step, starts, reached, obj, act)


def check_scan_edges(claims, g):
    """A value is carried over every claimed carry edge and a leak over every claimed stop edge
    would show; the edges are what they are called."""
    for e in claims["carry_edges"]:
        assert not g["head"][e] and lc.carry_count(g, e) > 0, e
    for e in claims["stop_edges"]:
        assert g["head"][e] and lc.stop_count(g, e) > 0, e


def check_actions(case, step, reached, act, nsteps):
    keys, states = case[0], case[1]
    want = {0, 4} | ({1} if nsteps > 1 else set())      # LINKED needs a second step
    want |= {2} if (states == lc.ERROR).any() else set()
    want |= {3} if reached < len(keys) else set()
    assert want <= set(np.unique(act).tolist())


@pytest.mark.parametrize("case_id", [c for c in lc.CASES if c.startswith("dense_tiles")])
def test_dense_tiles(case_id):
    case, step, starts, reached, obj, act, g = solved(case_id)
    claims = case[5]
    n = 259 * T + 5
    assert g["m"] == claims["events"] == n == reached and (act == 4).all()
    check_scan_edges(claims, g)
    # the round edge of sd_segmin_tile_prefix: one key from before tile 255 to after tile 256
    e = claims["round_edge"]
    assert e == lc.ROUND * T and len(set(g["ekeys"][[e - T - 3, e - 1, e, e + T + 5]].tolist())) == 1
    assert lc.carry_count(g, e) > 0
    assert sorted(claims["carry_edges"] + claims["stop_edges"])[:13] == [k * T for k in range(1, 14)]


@pytest.mark.parametrize("case_id", [c for c in lc.CASES if c.startswith("sparse_events")])
def test_sparse_events(case_id):
    case, step, starts, reached, obj, act, g = solved(case_id)
    keys, states, pre, seeds, chunk, claims = case
    assert g["m"] == claims["events"]
    assert sorted(claims["carry_edges"] + claims["stop_edges"]) == list(range(T, g["m"], T))
    check_scan_edges(claims, g)
    check_actions(case, step, reached, act, len(starts))
    late = np.flatnonzero((states == 0) & (np.arange(len(keys)) >= reached))
    if len(late):                                   # unreached Objects, the smallest ids: never seen
        assert (pre[late] < 1024).all() and not np.isin(obj[act == 4], pre[late]).any()
    # rows find an event of their key that comes later in their own step, and one of an earlier step
    rows, er = g["rows"], g["erows"][np.maximum(g["p"], 0)]
    assert (g["found"] & (er > rows)).any()
    assert len(starts) == 1 or (g["found"] & (step[er] < step[rows])).any()
    assert (states != 0)[pre != lc.NONE].any()      # an Object on a NO_CAS / ERROR row: no event


@pytest.mark.parametrize("case_id", [c for c in lc.CASES if c.startswith("block_edges")])
def test_block_edges(case_id):
    case, step, starts, reached, obj, act, g = solved(case_id)
    keys, states, pre, seeds, chunk, claims = case
    n = len(keys)
    assert reached == claims["reached"] < n
    # compaction blocks: one short of full, exactly full, one row into the next
    assert -(-reached // lc.EV_ROWS) == {16_383: 1, 16_384: 1, 16_385: 2, 32_768: 2, 32_769: 3}[reached]
    ev = set(g["erows"].tolist())
    assert reached - 1 in ev and reached not in ev and states[reached] == 0 and pre[reached] != lc.NONE
    assert keys[reached] == keys[reached - 1] and pre[reached] < pre[reached - 1]
    # the last reached row sees its own Object, not the smaller one of the first unreached row
    assert act[reached - 1] == 4 and obj[reached - 1] == pre[reached - 1] and act[reached] == 3
    unseen = pre[reached:][pre[reached:] != lc.NONE]
    assert not np.isin(obj[act == 4], unseen[unseen < 16]).any()
    for a, b in claims["pairs"]:                    # one key's events on both sides of a block edge
        assert b % lc.EV_ROWS == 0 and a == b - 1 and {a, b} <= ev and keys[a] == keys[b]
        assert obj[b] == pre[b] < pre[a] and act[a] == act[b] == 4
    assert len(claims["pairs"]) == (reached - 1) // lc.EV_ROWS
    check_actions(case, step, reached, act, len(starts))


def test_filter_collisions():
    case, step, starts, reached, obj, act, g = solved("filter_collisions")
    keys, states, pre, seeds, chunk, claims = case
    bits = {lc.filter_bit(k) for k in claims["event_keys"].tolist()}
    evk = set(g["ekeys"].tolist())
    assert evk == set(claims["event_keys"].tolist())
    crafted = claims["crafted"]
    assert len(crafted["below"]) >= 1 and len(crafted["above"]) >= 1 and len(crafted["between"]) >= 3
    for where, ks in crafted.items():
        for k in ks:
            assert lc.filter_bit(k) in bits and k not in evk
            assert (k < min(evk)) if where == "below" else (k > max(evk)) if where == "above" \
                else (min(evk) < k < max(evk))
            rows = np.flatnonzero(keys == np.uint64(k))
            assert len(rows) and (states[rows] == 0).all() and (pre[rows] == lc.NONE).all()
    # every "not found" answer of the binary search: lo == 0, lo == m, a neighbour with another key
    assert g["miss_lo0"] > 0 and g["miss_lom"] > 0 and g["miss_between"] > 0
    ck = np.array(sum(crafted.values(), []), np.uint64)
    a = act[np.isin(keys, ck) & (step != lc.NONE)]
    assert set(a.tolist()) == {0, 1}                # created and linked, never an Object's
    check_scan_edges(claims, g)
    check_actions(case, step, reached, act, len(starts))


def test_many_blocks():
    case, step, starts, reached, obj, act, g = solved("many_blocks")
    keys, states, pre, seeds, chunk, claims = case
    blocks = -(-reached // lc.EV_ROWS)
    assert blocks == claims["blocks"] > lc.ROUND + 1          # sd_links_pre_bscan's second round
    assert g["m"] > 16 * T                                     # several scan tiles as well
    hot = np.array(claims["hot_rows"])
    assert (hot // lc.EV_ROWS).tolist() == [0, lc.ROUND - 1, lc.ROUND, lc.ROUND + 1]
    assert set(hot.tolist()) <= set(g["erows"].tolist()) and (np.diff(pre[hot].astype(np.int64)) < 0).all()
    assert (obj[hot] == pre[hot]).all() and (act[hot] == 4).all()
    # rows of the hot key in the steps between its events take the latest (smallest) Object so far
    rows = np.flatnonzero((keys == np.uint64(claims["hot"])) & (states == 0) & (step != lc.NONE))
    assert set(obj[rows].tolist()) == set(pre[hot].tolist()) and len(rows) > 2000
    assert (states != 0).mean() > 0.015


def test_the_backward_scan_is_read_at_run_ends_only():
    """What the issue behind these tests asked to count — rows whose answer the BACKWARD scan
    brings from another tile — is zero for every input: a row's lookup bound is its next step's
    first row, so the lookup lands on the last event of a (key, step) run, where the backward
    scan's element is a segment start and T = F.  The backward pass (sd_links_pre_runs and the
    reverse sd_segmin_*) cannot change an answer, so no test through the entry point can see a
    defect in it; the forward counts above are the ones that bind."""
    for case_id in lc.CASES:
        if case_id == "many_blocks":
            continue
        case, ref = lc.build(case_id)
        keys, states, pre, seeds, chunk, _ = case
        step, starts, reached = cursor_walk(states, len(keys), chunk)
        g = lc.scan_geometry(case, step, starts, reached, ref[1], ref[2])
        assert g["reads_inside_run"] == 0 and g["found"].any()
