"""Inputs and CPU-side edge accounting of the link emission's size-edge tests
(tests/test_links_cases_cpu.py, tests/test_links_edges_gpu.py).

The path for rows that already own an Object (spacedrive_amd/csrc/links.hip, sd_links_pre_* and
sd_segmin_*) works on the EVENT list — hashed, reached rows owning an Object — sorted by
(key, row).  A case therefore sets the scan geometry exactly by choosing how many events each
key has: a key whose events lie on both sides of a multiple of SEG_TILE makes the scan carry a
value over that tile edge, a key that starts on the multiple makes the carry stop there.

Every generator returns (keys u64, states u8, pre u32, seeds [(key, id)], chunk, claims), claims
being a dict of the edges the case says it hits; `scan_geometry` recomputes all of them from the
reference's answer alone (cursor_walk + closed_form of tests/golden/make_golden.py).  Numpy
only: no torch, no library.
"""
import numpy as np

# mirrored from spacedrive_amd/csrc/links.hip:
SEG_TILE = 2048                    # SCAN_TILE = SCAN_THREADS * SCAN_ITEMS (sd_segmin_*)
EV_ROWS = 16384                    # EV_ROWS = EV_THREADS * EV_ITEMS (ordered compaction)
ROUND = 256                        # blocks per sd_links_pre_bscan round, tiles per sd_segmin_tile_prefix round
FILTER_BITS = 23                   # FILTER_BITS
FILTER_MUL = 0x9E3779B97F4A7C15    # filter_bit(): key * this, top FILTER_BITS bits

NONE = 0xFFFFFFFF
HASHED, NO_CAS, ERROR = 0, 1, 2
_M64 = (1 << 64) - 1


def filter_bit(key: int) -> int:
    """links.hip filter_bit."""
    return ((int(key) * FILTER_MUL) & _M64) >> (64 - FILTER_BITS)


def pattern(T=SEG_TILE):
    """Events per key, in key order: ends on, one before and one after a tile edge, single
    events on both sides of one, keys over three and five tiles."""
    return [T, T - 1, 1, T + 1, T - 1, 3 * T, 1, 1, T - 2, 5 * T + 7, 2]


def _truncate(mult, m):
    out, left = [], m
    for c in mult:
        if left <= 0:
            break
        out.append(min(c, left))
        left -= out[-1]
    assert left == 0, "pattern shorter than the events asked for"
    return out


def _event_keys(rng, count):
    """Distinct ascending keys with room below and above for keys that have no event."""
    k = np.unique(rng.integers(1 << 60, (1 << 64) - (1 << 60), 2 * count + 8, dtype=np.uint64))
    return np.sort(rng.permutation(k)[:count])


def _walk(states, n, chunk):
    from tests.golden.make_golden import cursor_walk
    return cursor_walk(states, n, chunk)


def _states(rng, n, chunk, share):
    """`share` of the rows NO_CAS / ERROR, more of them on the chunks' last rows (the cursor
    queries those again)."""
    states = np.zeros(n, np.uint8)
    bad = rng.random(n) < share
    states[bad] = rng.choice(np.array([NO_CAS, ERROR], np.uint8), int(bad.sum()))
    last = np.arange(chunk - 1, n, chunk)
    if len(last):
        states[last[rng.random(len(last)) < 0.10]] = ERROR
        states[last[rng.random(len(last)) < 0.10]] = NO_CAS
    return states


def _plant_stops(pre, order, stops):
    """The key that ENDS on stop edge e (event e - 1, `order` = event index -> row) gets an id
    below every other: a carry that leaked over e would change every answer of the next key."""
    for j, e in enumerate(stops):
        pre[order[e - 1]] = 1 + j


def dense_tiles(chunk, seed=7100):
    """Every row hashed and owning a distinct Object: the events are all the rows.  259 tiles
    + 5 events; the pattern, keys of 1-39 events up to three events before tile 255's start, one
    key of 2T + 9 events across the 256-tile round edge, keys of 1-39 events to the end."""
    rng = np.random.default_rng(seed + chunk)
    T = SEG_TILE
    n = 259 * T + 5
    mult = pattern(T)
    at = sum(mult)
    stop = ROUND * T - T - 3
    while at < stop:
        mult.append(min(int(rng.integers(1, 40)), stop - at))
        at += mult[-1]
    long_at = at
    mult.append(2 * T + 9)
    at += mult[-1]
    while at < n:
        mult.append(min(int(rng.integers(1, 40)), n - at))
        at += mult[-1]
    K = _event_keys(rng, len(mult))
    seg = np.repeat(np.arange(len(mult)), mult)
    keys = np.empty(n, np.uint64)
    keys[rng.permutation(n)] = K[seg]         # each key's rows spread over the steps
    ids = rng.permutation(1 << 21).astype(np.int64) * 1021 + 7   # distinct, below 2^31
    pre = ids[:n].astype(np.uint32)
    sk = K[rng.random(len(K)) < 0.05]
    seeds = list(zip(sk.tolist(), ids[n:n + len(sk)].tolist()))
    T_ = [k * T for k in (3, 5, 6, 9, 10, 11, 12, 13)]
    order = np.lexsort((np.arange(n), keys))   # event index -> row
    stops = [k * T for k in (1, 2, 4, 7, 8)]
    _plant_stops(pre, order, stops)
    pre[order[long_at]] = len(stops) + 1       # the long key's first event holds its smallest id
    claims = {"events": n, "reached": n,
              "carry_edges": T_ + [(ROUND - 1) * T, ROUND * T, (ROUND + 1) * T],
              "stop_edges": stops,
              "round_edge": ROUND * T, "long_key_at": long_at}
    return keys, np.zeros(n, np.uint8), pre, seeds, chunk, claims


def sparse_events(m, n=40_000, chunk=100, lead=0, seed=7200):
    """Exactly lead + m events among n rows: `lead` keys of one event, then the pattern cut off
    at m.  With lead = 0 the pattern's first keys END on the tile edges 2048 and 4096 (the carry
    must stop); lead = 3 moves them so that a key lies across each edge."""
    rng = np.random.default_rng(seed + 13 * m + chunk + 1000 * lead)
    states = _states(rng, n, chunk, 0.05)
    step, starts, reached = _walk(states, n, chunk)
    idx = np.arange(n)
    hashed = states == HASHED
    cand = np.flatnonzero(hashed & (idx < reached))
    mult = [1] * lead + _truncate(pattern(), m)
    m_all = lead + m
    ev_rows = rng.permutation(cand)[:m_all]
    assert len(ev_rows) == m_all
    K = _event_keys(rng, len(mult))
    keys = rng.integers(1, 1 << 60, n, dtype=np.uint64)      # rows without a cas_id: ignored
    is_ev = np.zeros(n, bool)
    is_ev[ev_rows] = True
    keys[ev_rows] = K[np.repeat(np.arange(len(mult)), mult)]
    other = rng.permutation(np.flatnonzero(hashed & ~is_ev))
    cut = int(0.4 * len(other))
    keys[other[:cut]] = K[rng.integers(0, len(K), cut)]       # look events up, earlier and later steps
    fresh = rng.integers(1, 1 << 64, max(1, (len(other) - cut) // 2), dtype=np.uint64)
    fresh = fresh[~np.isin(fresh, K)]
    keys[other[cut:]] = fresh[rng.integers(0, len(fresh), len(other) - cut)]
    ids = (rng.permutation(4 * n) + 1024).astype(np.uint32)   # pre and seed ids interleaved
    pre = np.full(n, NONE, np.uint32)
    pre[ev_rows] = ids[:m_all]
    bounds = np.cumsum(mult)
    edges = list(range(SEG_TILE, m_all, SEG_TILE))
    _plant_stops(pre, ev_rows, [e for e in edges if e in bounds])   # ev_rows[e - 1]: a row of that key
    used = m_all
    owners = np.flatnonzero(~hashed)                          # NO_CAS / ERROR rows owning an Object:
    owners = owners[rng.random(len(owners)) < 0.3]            # no events
    pre[owners] = ids[used:used + len(owners)]
    used += len(owners)
    late = np.flatnonzero(hashed & (idx >= reached))          # unreached rows: an event key and the
    keys[late] = K[rng.integers(0, len(K), len(late))]        # smallest ids, never seen by the job
    pre[late] = 16 + np.arange(len(late), dtype=np.uint32)
    assert len(late) < 1000
    allk = np.unique(keys[hashed])
    sk = np.concatenate([allk[rng.random(len(allk)) < 0.1], [np.uint64(12345)]]).astype(np.uint64)
    seeds = list(zip(sk.tolist(), ids[used:used + len(sk)].tolist()))
    claims = {"events": m_all,
              "carry_edges": [e for e in edges if e not in bounds],
              "stop_edges": [e for e in edges if e in bounds],
              "event_keys": K}
    return keys, states, pre, seeds, chunk, claims


def block_edges(reached_target, chunk=100, seed=7300):
    """The job reaches exactly `reached_target` rows of n > reached_target (stay-orphan rows end
    as many steps as that takes).  One key owns Objects at rows reached - 1 (seen) and reached
    (smaller id, not seen); another at the last row of each compaction block and the first of the
    next."""
    rng = np.random.default_rng(seed + reached_target)
    n = -(-(reached_target + 1) // chunk) * chunk
    steps_total = n // chunk
    stays = n - reached_target                # each re-queried row costs the job one row
    assert 1 <= stays < steps_total
    states = np.zeros(n, np.uint8)
    bad = rng.random(n) < 0.05
    states[bad] = rng.choice(np.array([NO_CAS, ERROR], np.uint8), int(bad.sum()))
    pairs = [(b - 1, b) for b in range(EV_ROWS, n, EV_ROWS)]
    guard = {r for p in pairs for r in p} | {reached_target - 1, reached_target}
    states[sorted(guard)] = HASHED
    start = 0
    for k in range(steps_total):              # the cursor walk, fixing each step's last row
        last = min(start + chunk, n) - 1
        if stays and k + 1 < steps_total and last not in guard:
            if states[last] == HASHED:
                states[last] = NO_CAS if k % 2 else ERROR
            stays -= 1
            start = last
        else:
            states[last] = HASHED
            start = last + 1
    pool = rng.integers(1, 1 << 64, n // 3, dtype=np.uint64)
    keys = pool[rng.integers(0, len(pool), n)]
    ids = (rng.permutation(4 * n) + 16).astype(np.uint32)
    pre = np.where((rng.random(n) < 0.1), ids[:n], NONE).astype(np.uint32)
    k_edge = np.uint64(0x0B10C4ED6E5)
    marked = sorted(guard)
    keys[marked] = k_edge
    pre[marked] = 15 - np.arange(len(marked))             # the later row holds the smaller id
    keys[7], states[7], pre[7] = k_edge, HASHED, NONE     # step 0: before any of these Objects
    sk = pool[rng.random(len(pool)) < 0.1]
    seeds = list(zip(sk.tolist(), ids[n:n + len(sk)].tolist()))
    claims = {"reached": reached_target, "pairs": [p for p in pairs if p[1] < reached_target],
              "k_edge": int(k_edge), "marked": marked}
    return keys, states, pre, seeds, chunk, claims


def many_blocks(seed=7400):
    """258 compaction blocks + 5 rows (259 blocks): the block-offset scan's second round.  One row in 64 owns
    an Object (about 33 scan tiles); one key has events in blocks 0, 255, 256 and 257 with ids
    descending and rows in many steps."""
    rng = np.random.default_rng(seed)
    n, chunk = 258 * EV_ROWS + 5, 4096
    states = _states(rng, n, chunk, 0.02)
    uniq = rng.integers(1, 1 << 64, int(n * 0.7), dtype=np.uint64)
    keys = np.concatenate([uniq, uniq[rng.integers(0, len(uniq), n - len(uniq))]])
    rng.shuffle(keys)
    own = rng.random(n) < 1 / 64
    ids = rng.permutation(1 << 24).astype(np.uint32) + 100
    pre = np.full(n, NONE, np.uint32)
    pre[own] = ids[:int(own.sum())]
    hot = np.uint64(0xABCDEF)
    hot_rows = np.array([5, 255 * EV_ROWS + 7, 256 * EV_ROWS, 257 * EV_ROWS + 3])
    keys[np.arange(11, n, 1999)] = hot
    keys[hot_rows] = hot
    states[hot_rows] = HASHED
    pre[keys == hot] = NONE
    pre[hot_rows] = [40, 30, 20, 10]
    sk = uniq[:len(uniq) // 100]
    seeds = list(zip(sk.tolist(), ids[int(own.sum()):int(own.sum()) + len(sk)].tolist()))
    claims = {"hot": int(hot), "hot_rows": hot_rows.tolist(), "blocks": 259}
    return keys, states, pre, seeds, chunk, claims


def filter_collisions(seed=7500):
    """A sparse_events batch (3 tiles + 1 events) in which hashed rows without an Object take keys
    that NO event has but that set an event key's bit in the key filter, so the lookup passes the
    filter and its binary search has to answer "not found": below every event key (lo == 0),
    above every one (lo == m), and between two (a neighbour with another key)."""
    rng = np.random.default_rng(seed)
    keys, states, pre, seeds, chunk, claims = sparse_events(3 * SEG_TILE + 1, lead=3, seed=seed)
    K = claims["event_keys"]
    ginv = pow(FILTER_MUL, -1, 1 << 64)
    shift = 64 - FILTER_BITS
    crafted = {"below": [], "between": [], "above": []}
    want = {"below": 3, "between": 12, "above": 3}
    lo_k, hi_k = int(K.min()), int(K.max())
    evset = set(K.tolist())
    while any(len(crafted[w]) < want[w] for w in want):
        ek = int(K[rng.integers(0, len(K))])
        z = (filter_bit(ek) << shift) | int(rng.integers(0, 1 << shift))
        key = (z * ginv) & _M64
        if key in evset or key == 0:
            continue
        where = "below" if key < lo_k else "above" if key > hi_k else "between"
        if len(crafted[where]) < want[where]:
            crafted[where].append(key)
    ck = np.array(sum(crafted.values(), []), np.uint64)
    seeded = {k for k, _ in seeds}
    free = np.flatnonzero((states == HASHED) & (pre == NONE) & ~np.isin(keys, K))
    free = rng.permutation(free)[:40 * len(ck)]
    keys[free] = ck[rng.integers(0, len(ck), len(free))]     # repeats across the steps
    twice = free[(free + 1 < len(keys))][:30]                # ... and inside one
    ok = (states[twice + 1] == HASHED) & (pre[twice + 1] == NONE) & ~np.isin(keys[twice + 1], K)
    keys[twice[ok] + 1] = keys[twice[ok]]
    assert not (seeded & set(ck.tolist()))
    claims = dict(claims, crafted=crafted)
    return keys, states, pre, seeds, chunk, claims


# ---- the reference's answer and what it says about the scans' geometry ----------------------

def reference(case, literal):
    """(step, obj, act, counts) of a case: the literal job replay, or cursor_walk + closed_form
    (+ closed_counts) for jobs too large to replay."""
    from tests.golden.make_golden import closed_form, cursor_walk, replay_identifier_job
    keys, states, pre, seeds, chunk, _ = case
    n = len(keys)
    if literal:
        step, obj, act, counts = replay_identifier_job(
            keys.tolist(), states.tolist(), chunk, existing=seeds, pre_objects=pre.tolist())
        return (np.array(step, np.int64), np.array(obj, np.int64), np.array(act, np.int64),
                [tuple(c) for c in counts])
    step, starts, _ = cursor_walk(states, n, chunk)
    obj, act = closed_form(keys, states, pre, seeds, step, starts)
    return step, obj, act, closed_counts(states, step, starts, act, chunk)


def closed_counts(states, step, starts, act, chunk):
    """Per-step (created, linked) from the closed form: every decided row in its final step, and
    a NO_CAS row that ends step k and is queried again by step k + 1 created in step k too."""
    ns = len(starts)
    created = np.bincount(step[act == 0], minlength=ns)
    linked = np.bincount(step[(act == 1) | (act == 4)], minlength=ns)
    s = np.asarray(starts, np.int64)
    again = np.flatnonzero((s[1:] == s[:-1] + chunk - 1) & (states[s[1:]] == NO_CAS))
    created[again] += 1
    return list(zip(created.tolist(), linked.tolist()))


def scan_geometry(case, step, starts, reached, obj, act):
    """From the reference's answer alone: the sorted event list and, for every hashed reached
    row, where its lookup lands (p), which event supplies its value (src) and whether that
    value is the row's answer.  Returns a dict of arrays and counts."""
    keys, states, pre, seeds, chunk, _ = case
    n = len(keys)
    idx = np.arange(n)
    ev = np.flatnonzero((states == HASHED) & (idx < reached) & (pre != NONE))
    ev = ev[np.lexsort((ev, keys[ev]))]
    ek, m = keys[ev], len(ev)
    g = {"m": m, "erows": ev, "ekeys": ek}
    rows = np.flatnonzero((states == HASHED) & (idx < reached))
    g["rows"] = rows
    if m == 0:
        return g
    head = np.r_[True, ek[1:] != ek[:-1]]
    seg = np.cumsum(head) - 1
    seg_at = np.flatnonzero(head)
    v = pre[ev].astype(np.int64)
    BIG = np.int64(1) << 33
    F = BIG - 1 - (np.maximum.accumulate(seg * BIG + (BIG - 1 - v)) - seg * BIG)   # forward scan
    newmin = head | (np.r_[True, F[1:] < F[:-1]] & (F == v))
    src_of = np.maximum.accumulate(np.where(newmin, np.arange(m), 0))             # argmin so far
    run_end = np.r_[(ek[1:] != ek[:-1]) | (step[ev[1:]] != step[ev[:-1]]), True]
    uk = ek[head]
    ns = len(starts)
    s = np.asarray(list(starts) + [NONE], np.int64)
    bound = np.where(step[rows] + 1 < ns, s[np.minimum(step[rows] + 1, ns)], NONE)
    kp = np.searchsorted(uk, keys[rows])
    kp_c = np.minimum(kp, len(uk) - 1)
    has = (kp < len(uk)) & (uk[kp_c] == keys[rows])
    comp = seg.astype(np.int64) * (1 << 32) + ev
    # the kernel's search: first event not < (key, bound) in (key, row) order
    key_lo = np.searchsorted(ek, keys[rows], side="left")
    lo = np.where(has, np.searchsorted(comp, kp_c.astype(np.int64) * (1 << 32) + bound), key_lo)
    p = lo - 1
    found = has & (p >= 0) & (seg[np.maximum(p, 0)] == kp_c)
    pc = np.maximum(p, 0)
    src = src_of[pc]
    answered = found & (act[rows] == 4) & (obj[rows] == v[src])   # no seed was smaller
    g.update(head=head, seg_at=seg_at, F=F, p=p, lo=lo, found=found, src=src, answered=answered,
             run_end=run_end, has=has)
    g["reads_inside_run"] = int((found & ~run_end[pc]).sum())
    bits = np.zeros(1 << FILTER_BITS, bool)
    with np.errstate(over="ignore"):
        bits[(uk * np.uint64(FILTER_MUL)) >> np.uint64(64 - FILTER_BITS)] = True
        passes = bits[(keys[rows] * np.uint64(FILTER_MUL)) >> np.uint64(64 - FILTER_BITS)]
    miss = passes & ~has                                           # searched, key without event
    g["miss_lo0"] = int((miss & (lo == 0)).sum())
    g["miss_lom"] = int((miss & (lo == m)).sum())
    g["miss_between"] = int((miss & (lo > 0) & (lo < m)).sum())
    g["found_not_before_bound"] = int((has & ~found).sum())       # key has events, all in later steps
    return g


def carry_count(g, e):
    """Rows whose answer the forward scan carries over event index e: supplied by an event
    before e, read at or after e."""
    return int((g["answered"] & (g["src"] < e) & (g["p"] >= e)).sum())


def stop_count(g, e):
    """Rows of the key that starts at event index e whose answer a carry leaking over e (the
    previous key's minimum) would change."""
    assert g["head"][e]
    nxt = g["seg_at"][np.searchsorted(g["seg_at"], e, side="right"):]
    end = int(nxt[0]) if len(nxt) else g["m"]
    mine = g["answered"] & (g["p"] >= e) & (g["p"] < end)
    return int((mine & (g["F"][e - 1] < g["F"][np.maximum(g["p"], 0)])).sum())


# ---- the cases both test files run: id -> (generator, args, kwargs, reference is the literal replay)
SPARSE_M = (1, 2047, 2048, 2049, 4095, 4096, 4097, 3 * SEG_TILE + 1)
CASES = {}
for _c in (7, 100, 1000):
    CASES[f"dense_tiles-chunk{_c}"] = (dense_tiles, (_c,), {}, True)
for _m in SPARSE_M:
    for _c in (7, 100, 50_000):                      # 50,000 > n: one step
        CASES[f"sparse_events-m{_m}-chunk{_c}"] = (sparse_events, (_m,), {"chunk": _c}, True)
# beyond the pattern as given: three keys of one event in front, so that a key lies ACROSS each of
# the edges 2048, 4096 and 6144 (without them the pattern's keys end on the first two)
CASES["sparse_events-m6145-lead3-chunk100"] = (sparse_events, (3 * SEG_TILE + 1,), {"lead": 3}, True)
for _r in (16_383, 16_384, 16_385, 32_768, 32_769):
    CASES[f"block_edges-reached{_r}"] = (block_edges, (_r,), {}, True)
CASES["filter_collisions"] = (filter_collisions, (), {}, True)
CASES["many_blocks"] = (many_blocks, (), {}, False)
HOST_CASES = ("sparse_events-m4097-chunk7", "block_edges-reached32769")

_built = {}


def build(case_id):
    """(case, reference) of a case id, made once per process and never written to."""
    if case_id not in _built:
        fn, args, kw, literal = CASES[case_id]
        case = fn(*args, **kw)
        ref = reference(case, literal)
        for a in case[:3] + ref[:3]:
            a.setflags(write=False)
        _built[case_id] = (case, ref)
    return _built[case_id]
