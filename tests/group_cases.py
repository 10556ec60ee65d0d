"""Inputs and the CPU model of the hash grouping's edge tests (tests/test_group_cases_cpu.py,
tests/test_group_edges_gpu.py).

The grouping (spacedrive_amd/csrc/group_hash.hip) buckets a key by the top bits of mix64(key), a
bijection, so a key for any bucket and any table slot is np_unmix64(mixed value).  Every generator
works in the mixed domain: it says how many rows and how many distinct keys each bucket gets (and,
where the partition's reservations matter, which rows of the batch they occupy) and unmixes at
the end.  `model` then derives from the keys alone which chain the batch takes and which exit of
bucket_min every bucket must take; a case's `claims` are held to it by the CPU test.

What the model cannot know is the order in which workgroups reserve rows, i.e. WHICH rows of a
full region spill and which rows of a bucket meet in one trip.  Every exit below is therefore
derived from counts that hold for every order; where that is not possible the model says so
(`claim_fail` for the 4,096-slot table, see exit_of_segment).

Numpy only: no torch, and nothing is read from the library.
"""
import numpy as np

from tests.golden.make_ws_sizes import region_capacity_nb      # group_hash.hip region_capacity_nb()

# ---- restated from the sources (each once; held to the text by test_constants_mirror_sources) ---
REGION_BITS = 8                       # sd_mix.h: SD_REGION_BITS 8
REGIONS = 1 << REGION_BITS            # sd_mix.h: REGIONS = 1u << REGION_BITS, top bits of mix64(key)
RPART_TILE = 512 * 8                  # group_hash.hip: RPART_THREADS x RPART_ITEMS (sd_region_partition)
RBIG_TILE = 1024 * 8                  # RBIG_THREADS x RBIG_ITEMS (sd_region_partition_big)
TABLE, TRIP = 4096, 512 * 4           # TABLE; MIN_THREADS x MIN_ITEMS (sd_bucket_min)
BIG_TABLE, BIG_TRIP = 12288, 1024 * 8  # BIG_TABLE; BIG_THREADS x ITEMS (sd_bucket_min_big and, with
#                                       REGION_BITS 8, REG_TABLE/REG_THREADS/REG_ITEMS of the region tables)
FILL, BIG_FILL = TABLE // 8 * 7, BIG_TABLE // 8 * 7   # bucket_min: FILL = TBL / 8 * 7 (3,584 / 10,752)
BIG_MAX_KEYS = 256 * 5632             # BIG_MAX_KEYS
TARGET_PER_BUCKET, MAX_BITS, MAX_B2, COARSE10_KEYS, RBIG_MAX_NB = 1536, 19, 9, 40_000_000, 256
HOME_LAST_LOW32 = 4_294_617_771       # smallest low32 with (low32 * 12288) >> 32 == 12287 (home_slot)

EXITS = ("empty", "one_trip", "multi_trip", "spill_lds", "own_table", "whole_input", "claim_fail")
# exits a chain can be MADE to take whatever the reservation order (see exit_of_segment for the
# 4,096-slot table's claim_fail; a region that fits its capacity holds <= 6,297 rows, one trip
# and below FILL, so the small-regions chain has neither multi_trip nor own_table)
REACHABLE = {
    "S": {"empty", "one_trip", "spill_lds", "whole_input", "claim_fail"},
    "T-fine": {"empty", "one_trip", "multi_trip", "own_table"},
    "T-big": {"empty", "one_trip", "multi_trip", "own_table", "claim_fail"},
    "B": {"empty", "one_trip", "multi_trip", "own_table"},
}

_U = np.uint64
_M1, _M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB           # sd_mix.h mix64
_I1, _I2 = pow(_M1, -1, 1 << 64), pow(_M2, -1, 1 << 64)


def np_mix64(z):
    """sd_mix.h mix64 (the splitmix64 finaliser), vectorised."""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> _U(30))) * _U(_M1)
    z = (z ^ (z >> _U(27))) * _U(_M2)
    return z ^ (z >> _U(31))


def _unxorshift(z, s):
    x = z
    for _ in range(64 // s + 1):
        x = z ^ (x >> _U(s))
    return x


def np_unmix64(m):
    """The inverse: np_mix64(np_unmix64(x)) == x."""
    m = np.asarray(m, dtype=np.uint64)
    m = _unxorshift(m, 31) * _U(_I2)
    m = _unxorshift(m, 27) * _U(_I1)
    return _unxorshift(m, 30)


def region_capacity(n):
    """group_hash.hip region_capacity(): region_capacity_nb(n, REGIONS)."""
    return region_capacity_nb(n, REGIONS)


def group_plan(n, target):
    """group_hash.hip group_plan() -> (b1, b2, big)."""
    target = target or TARGET_PER_BUCKET
    bits = 1
    while bits < MAX_BITS and (1 << bits) * target < n:
        bits += 1
    cb = 8 if n <= COARSE10_KEYS else 10
    b1 = bits if bits < cb else (bits - MAX_B2 if bits - cb > MAX_B2 else cb)
    b2 = bits - b1
    big = b2 > 0 and n <= BIG_MAX_KEYS
    return b1, (0 if big else b2), big


def pick_chain(n, target):
    """group_hash.hip pick_chain() -> 'S' (SmallRegions), 'B' (BigRegions), 'T-fine' / 'T-big'
    (TwoLevel ending in sd_bucket_min / sd_bucket_min_big), with the plan's final bucket bits."""
    b1, b2, big = group_plan(n, target)
    if target == 0 and 0 < n <= BIG_MAX_KEYS:
        return "S", REGION_BITS
    if target == 0 and not big and b2 > 0 and (1 << b1) <= RBIG_MAX_NB:
        return "B", b1 + b2
    return ("T-big" if big else "T-fine"), b1 + b2


def exit_of_segment(rows, distinct, tbl, fill, trip):
    """The exit of a bucket whose rows are a starts[] segment (no spill list).

    The table overflows to the bucket's own global table exactly when its distinct keys pass
    `fill` — the count is cumulative over the trips, so no order changes it.  A READ_FIRST claim
    fails (`claim_fail`) only in a trip that meets a full table.  Trip 1 cannot raise the flag
    (trip <= fill), so trip 2 always runs; it is certain to overfill the table when even the
    most duplicate-heavy 2 x trip rows hold more than tbl distinct keys.  For the 4,096-slot table
    2 x 2,048 rows fill it exactly and never overfill it: a claim can fail there only in trip 3,
    and only if the first two trips happened to hold <= 3,584 distinct keys — some order of any
    such bucket puts more than that first, so no input reaches it for certain.  It is reachable
    by luck, not by construction; the model reports own_table for those buckets."""
    if rows == 0:
        return "empty"
    if min(rows, 2 * trip) - (rows - distinct) > tbl:
        return "claim_fail"
    if distinct > fill:
        return "own_table"
    return "one_trip" if rows <= trip else "multi_trip"


def model(keys, target=0):
    """From the keys alone: chain, and per bucket rows / distinct / exit; for the region chains
    also capacity, spill per region and (chain S) rows per trip loop `span` = e - s and trips."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    chain, bits = pick_chain(n, target)
    mixed = np_mix64(keys)
    uniq = np.unique(mixed)
    nb = 1 << bits
    rows = np.bincount((mixed >> _U(64 - bits)).astype(np.int64), minlength=nb)
    distinct = np.bincount((uniq >> _U(64 - bits)).astype(np.int64), minlength=nb)
    m = {"chain": chain, "n": n, "bits": bits, "rows": rows, "distinct": distinct, "objects": len(uniq)}
    if chain == "S":
        cap = region_capacity(n)
        spill = np.maximum(rows - cap, 0)
        total = int(spill.sum())
        full = rows > cap
        # a full region's loop runs over its cap region rows + the WHOLE spill list (entries of
        # other regions are read as empty)
        span = np.where(full, cap + total, rows)
        exits = []
        for b in range(nb):
            if not full[b]:
                assert rows[b] <= BIG_TRIP and distinct[b] <= BIG_FILL   # cap <= 6,297 in this chain
                exits.append("empty" if rows[b] == 0 else "one_trip")
                continue
            foreign = total - int(spill[b])
            dups = int(rows[b] - distinct[b])
            if min(int(span[b]), 2 * BIG_TRIP) - foreign - dups > BIG_TABLE:
                exits.append("claim_fail")       # trips 1 + 2 hold > 12,288 distinct keys in any order
            elif distinct[b] > BIG_FILL:
                exits.append("whole_input")
            else:
                exits.append("spill_lds")
        m.update(cap=cap, spill=spill, total_spill=total, full=full, span=span,
                 trips=-(-span // BIG_TRIP), exit=exits,
                 carved=int(2 * rows[np.array([e in ("whole_input", "claim_fail") for e in exits])].sum()))
        return m
    if chain == "B":
        cap = region_capacity_nb(n, REGIONS)
        rrows = np.bincount((mixed >> _U(64 - REGION_BITS)).astype(np.int64), minlength=REGIONS)
        m.update(cap=cap, region_rows=rrows, spill=np.maximum(rrows - cap, 0), full=rrows > cap)
        m["total_spill"] = int(m["spill"].sum())
    tbl, fill, trip = (BIG_TABLE, BIG_FILL, BIG_TRIP) if chain == "T-big" else (TABLE, FILL, TRIP)
    m["exit"] = [exit_of_segment(int(r), int(d), tbl, fill, trip) for r, d in zip(rows, distinct)]
    m["trips"] = -(-rows // trip)
    return m


def bucket_of_row(keys, i, bits):
    return int(np_mix64(keys[i:i + 1])[0] >> _U(64 - bits))


# ---- building blocks (mixed domain) -------------------------------------------------------------

def mixed_keys(rng, bucket, bits, count, low32=None):
    """`count` distinct mixed values of `bucket` (its top `bits` bits); low32: an array of at
    least `count` distinct-or-not low words to plant (home slots)."""
    out = np.zeros(0, np.uint64)
    while len(out) < count:
        x = rng.integers(0, 1 << 63, 2 * count + 16, dtype=np.uint64) << _U(1)
        x = (x >> _U(bits)) | (_U(bucket) << _U(64 - bits))
        if low32 is not None:
            lw = np.asarray(low32, dtype=np.uint64)
            x = (x & ~_U(0xFFFFFFFF)) | lw[rng.integers(0, len(lw), len(x))]
        out = np.unique(np.concatenate([out, x]))
    return rng.permutation(out)[:count]


def rows_of(rng, dk, rows, hot=0.5):
    """`rows` rows over the distinct keys dk, each at least once; `hot` of the repeats are dk[0]."""
    assert rows >= len(dk)
    extra = dk[rng.integers(0, len(dk), rows - len(dk))]
    extra[rng.random(len(extra)) < hot] = dk[0]
    return np.concatenate([dk, extra])


def bucket_rows(rng, bucket, bits, rows, distinct, low32=None, hot=0.5):
    return rows_of(rng, mixed_keys(rng, bucket, bits, distinct, low32), rows, hot)


def home_last(rng, count):
    """low words whose 12,288-slot home is the last slot 12,287."""
    return rng.integers(HOME_LAST_LOW32, 1 << 32, count, dtype=np.uint64)


def filler(rng, count, avoid, bits):
    """Uniform mixed values, about 30 % of the rows repeats, none in the buckets `avoid`."""
    if count == 0:
        return np.zeros(0, np.uint64)
    pool = rng.integers(0, 1 << 63, max(1, int(count * 0.7)), dtype=np.uint64) << _U(1)
    pool |= rng.integers(0, 2, len(pool), dtype=np.uint64)
    allowed = np.setdiff1d(np.arange(1 << bits), np.asarray(list(avoid), dtype=np.int64))
    b = (pool >> _U(64 - bits)).astype(np.int64)
    bad = np.isin(b, list(avoid)) if len(avoid) else np.zeros(len(pool), bool)
    newb = allowed[rng.integers(0, len(allowed), int(bad.sum()))].astype(np.uint64)
    pool[bad] = ((pool[bad] << _U(bits)) >> _U(bits)) | (newb << _U(64 - bits))
    return pool[rng.integers(0, len(pool), count)]


def assemble(rng, n, parts, avoid, bits, placed=()):
    """n keys: `placed` = (mixed rows, lo, hi) at random rows of [lo, hi), `parts` and the filler
    (never in the buckets `avoid`) shuffled over the rest."""
    fixed = sum(len(p) for p in parts) + sum(len(a) for a, _, _ in placed)
    assert fixed <= n, (fixed, n)
    out = np.empty(n, np.uint64)
    free = np.ones(n, bool)
    for arr, lo, hi in placed:
        cand = np.flatnonzero(free[lo:hi]) + lo
        assert len(cand) >= len(arr)
        pos = rng.permutation(cand)[:len(arr)]
        out[pos] = arr
        free[pos] = False
    rest = np.concatenate(list(parts) + [filler(rng, n - fixed, avoid, bits)])
    out[free] = rng.permutation(rest)
    return np_unmix64(out)


# ---- chain S: the default plan up to BIG_MAX_KEYS ----------------------------------------------

def region_at_cap(delta, n=20_000, seed=8100):
    """Region 7 holds exactly cap + delta rows (about 100 distinct keys)."""
    rng = np.random.default_rng(seed + delta)
    cap = region_capacity(n)
    keys = assemble(rng, n, [bucket_rows(rng, 7, 8, cap + delta, 100)], {7}, 8)
    return keys, 0, {7: "spill_lds" if delta > 0 else "one_trip"}, {"spill": max(delta, 0)}


def fill_from_g_eq_cap(tiles, n=20_000, seed=8200):
    """Region 9 gets exactly cap rows from each of the first `tiles` partition tiles and none
    from any other: whichever tile reserves first, the second reservation starts at g == cap
    (the `g <= cap && g + h > cap` arm) and spills all its rows; a third starts at g > cap."""
    rng = np.random.default_rng(seed + tiles)
    cap = region_capacity(n)
    dk = mixed_keys(rng, 9, 8, 50)
    placed = [(rows_of(rng, rng.permutation(dk), cap), t * RPART_TILE, (t + 1) * RPART_TILE) for t in range(tiles)]
    keys = assemble(rng, n, [], {9}, 8, placed)
    return keys, 0, {9: "spill_lds"}, {"spill": (tiles - 1) * cap}


def fill_in_one_tile(n=20_000, seed=8300):
    """cap + 300 rows of region 11, all inside partition tile 2: g = 0, h > cap."""
    rng = np.random.default_rng(seed)
    cap = region_capacity(n)
    placed = [(bucket_rows(rng, 11, 8, cap + 300, 120), 2 * RPART_TILE, 3 * RPART_TILE)]
    return assemble(rng, n, [], {11}, 8, placed), 0, {11: "spill_lds"}, {"spill": 300}


def several_full(count, n=20_000, seed=8400):
    """`count` full regions (0 and 255 among them from 2 up), each cap + 1..40 rows of a hot key
    and some 60 others: the spill list interleaves their rows, the last of them to finish re-zeroes
    the three counters.  All 256 cannot be full (256 x (cap + 1) > n for every n: the capacity is
    above the mean); 80 of 256 is what n = 20,000 holds with room for filler."""
    rng = np.random.default_rng(seed + count)
    cap = region_capacity(n)
    regs = [0, 255, 100][:count] if count <= 3 else [0, 255] + list(rng.permutation(np.arange(1, 255))[:count - 2])
    if count == 1:
        regs = [100]
    extra = {int(r): int(rng.integers(1, 41)) for r in regs}
    parts = [bucket_rows(rng, r, 8, cap + x, 60) for r, x in extra.items()]
    keys = assemble(rng, n, parts, set(extra), 8)
    return keys, 0, {r: "spill_lds" for r in extra}, {"spill": sum(extra.values()), "full": count}


def trips(rows, n=20_000, seed=8500):
    """One full region (21) whose loop covers exactly `rows` rows (cap + its own spill; no other
    region is full): 8,192 = one trip with the lookup from registers, 8,193 = two trips with
    READ_FIRST claims and lds_find, > 16,384 = three.  100 distinct keys, 40 of them with home
    slot 12,287 (the probe chain wraps in both forms of the lookup)."""
    rng = np.random.default_rng(seed + rows)
    dk = np.concatenate([mixed_keys(rng, 21, 8, 60), mixed_keys(rng, 21, 8, 40, home_last(rng, 64))])
    keys = assemble(rng, n, [rows_of(rng, dk, rows)], {21}, 8)
    return keys, 0, {21: "spill_lds"}, {"trips": {21: -(-rows // BIG_TRIP)}, "span": {21: rows}}


def fill_edge(distinct, rows, n, seed=8600):
    """One full region (30) of `rows` rows with exactly `distinct` distinct keys."""
    rng = np.random.default_rng(seed + distinct)
    keys = assemble(rng, n, [bucket_rows(rng, 30, 8, rows, distinct, hot=0.1)], {30}, 8)
    want = "spill_lds" if distinct <= BIG_FILL else "whole_input" if distinct <= BIG_TABLE else "claim_fail"
    return keys, 0, {30: want}, {"trips": {30: -(-rows // BIG_TRIP)}}


def two_carves(n=40_000, seed=8700):
    """Regions 20 and 200 both pass FILL distinct keys: two carves of the 2n-slot global table in
    one call (2 x 11,000 slots each)."""
    rng = np.random.default_rng(seed)
    parts = [bucket_rows(rng, r, 8, 11_000, 10_800, hot=0.1) for r in (20, 200)]
    keys = assemble(rng, n, parts, {20, 200}, 8)
    return keys, 0, {20: "whole_input", 200: "whole_input"}, {"carved": 44_000}


def probe_wrap(n=20_000, seed=8800):
    """Region 33, not full: 150 distinct keys all with home slot 12,287 of the 12,288-slot table,
    180 rows: the one-trip claims wrap to slot 0 and run 150 slots on."""
    rng = np.random.default_rng(seed)
    keys = assemble(rng, n, [bucket_rows(rng, 33, 8, 180, 150, home_last(rng, 400), hot=0.2)], {33}, 8)
    return keys, 0, {33: "one_trip"}, {"home_last": (33, 150)}


def global_home_wrap(n=30_000, seed=8900):
    """Region 44 goes to whole_input with rows = 11,500, so its carved table has 23,000 slots; 300
    of its 10,900 distinct keys have the global home slot 22,999 (low32 % 23,000): g_insert and
    g_find wrap to slot 0."""
    rng = np.random.default_rng(seed)
    rows, cap_g = 11_500, 23_000
    low = (cap_g - 1) + cap_g * rng.integers(0, (1 << 32) // cap_g - 1, 4000, dtype=np.uint64)
    dk = np.concatenate([mixed_keys(rng, 44, 8, 300, low), mixed_keys(rng, 44, 8, 10_600)])
    keys = assemble(rng, n, [rows_of(rng, rng.permutation(dk), rows, hot=0.1)], {44}, 8)
    return keys, 0, {44: "whole_input"}, {"global_home_last": (44, cap_g, 300)}


def vals_edges(n=20_000, seed=9000):
    """For group_min (case_vals plants the values in every case; this one has the shapes they
    need in a full region): a hot key of some 2,900 rows and 200 other keys of region 50."""
    rng = np.random.default_rng(seed)
    keys = assemble(rng, n, [bucket_rows(rng, 50, 8, 3600, 200, hot=0.85)], {50}, 8)
    return keys, 0, {50: "spill_lds"}, {}


def dispatch_edge(n, seed=9100):
    """The same construction at n = BIG_MAX_KEYS (chain S at its largest) and one more key (chain
    B at its smallest): region 5 holds exactly cap rows and region 6 cap + 1."""
    rng = np.random.default_rng(seed)
    cap = region_capacity(n)
    assert cap == region_capacity(BIG_MAX_KEYS)
    parts = [bucket_rows(rng, 5, 8, cap, 5000, hot=0.1), bucket_rows(rng, 6, 8, cap + 1, 5000, hot=0.1)]
    keys = assemble(rng, BIG_MAX_KEYS, parts, {5, 6}, 8)
    if n == BIG_MAX_KEYS:
        return keys, 0, {5: "one_trip", 6: "spill_lds"}, {"spill": 1, "full": 1}
    assert n == BIG_MAX_KEYS + 1                # the same keys and one more, in region 77
    keys = np.concatenate([keys, np_unmix64(mixed_keys(rng, 77, 8, 1))])
    return keys, 0, {}, {"spill": 1, "full": 1, "region_rows": {5: cap, 6: cap + 1}}


# ---- chain T: set_group_method(GROUP_HASH, target) ----------------------------------------------

T_FINE = dict(n=20_000, target=1300, bits=4)     # 16 buckets, no refine, sd_bucket_min
T_BIG = dict(n=30_000, target=16, bits=8)        # 256 buckets, sd_bucket_min_big


def t_segments(kind, spec, empty=(), seed=9200):
    """spec: {bucket: (rows, distinct)}; `empty` buckets get no row at all."""
    p = T_FINE if kind == "fine" else T_BIG
    rng = np.random.default_rng(seed + sum(r * 7 + d for r, d in spec.values()) + len(empty))
    tbl, fill, trip = (TABLE, FILL, TRIP) if kind == "fine" else (BIG_TABLE, BIG_FILL, BIG_TRIP)
    parts, claims = [], {}
    for b, (rows, distinct) in spec.items():
        dk = mixed_keys(rng, b, p["bits"], distinct)
        if kind == "big" and distinct >= 40:     # some probe chains wrap at slot 12,287
            dk[:40] = mixed_keys(rng, b, p["bits"], 40, home_last(rng, 64))
            dk = np.unique(dk)
            assert len(dk) == distinct
        parts.append(rows_of(rng, dk, rows, hot=0.1))
        claims[b] = exit_of_segment(rows, distinct, tbl, fill, trip)
    for b in empty:
        claims[b] = "empty"
    keys = assemble(rng, p["n"], parts, set(spec) | set(empty), p["bits"])
    return keys, p["target"], claims, {}


# ---- chain B: the default plan above BIG_MAX_KEYS -----------------------------------------------

N_B = BIG_MAX_KEYS + 1                           # b1 = 8, b2 = 2: 1,024 fine buckets of 4 per region


def b_three_full(seed=9300):
    """Regions 0, 100 and 200 full (0 is the first, none is the last): the refine of every later
    region starts its segment at the sum of the FULL cursors before it.  Region 0 holds a key of
    20,000 copies (a fine bucket of ten trips) and 3,000 others."""
    rng = np.random.default_rng(seed)
    hot = mixed_keys(rng, 1, 10, 1)              # fine bucket 1 of region 0
    parts = [np.repeat(hot, 20_000), bucket_rows(rng, 2, 10, 3000, 3000),
             *[bucket_rows(rng, 400 + j, 10, 2250, 125) for j in range(4)],      # region 100: 9,000 rows
             *[bucket_rows(rng, 800 + j, 10, 1750, 500) for j in range(4)]]      # region 200: 7,000 rows
    keys = assemble(rng, N_B, parts, {0, 100, 200}, 8)
    cap = region_capacity_nb(N_B, REGIONS)
    return keys, 0, {1: "multi_trip", 2: "multi_trip", 400: "multi_trip", 803: "one_trip"}, {
        "full": 3, "spill": 23_000 + 9000 + 7000 - 3 * cap, "region_rows": {0: 23_000, 100: 9000, 200: 7000}}


def b_fine_fill(distinct, seed=9400):
    """Fine bucket 517 (region 129, which stays below its capacity) with 3,700 rows and `distinct`
    distinct keys: 3,584 stays in LDS, 3,585 goes to its own global table."""
    rng = np.random.default_rng(seed + distinct)
    keys = assemble(rng, N_B, [bucket_rows(rng, 517, 10, 3700, distinct, hot=0.1)], {129}, 8)
    return keys, 0, {517: "multi_trip" if distinct <= FILL else "own_table"}, {"full": 0}


# ---- sequences: calls on one engine whose leftovers would meet ---------------------------------

def seq_call(which, n=30_000, seed=9500):
    """Calls of the spill-count sequences (chain S, one n): region 60 holds only the key H.
    A: H on rows of the first third, 3 full regions, a long spill list.  A2: the two-tile
    g == cap construction with H alone (the reservation that fills starts at g == cap).
    B: H on rows of the second third, region 60 full by exactly one row.  C: no full region.
    D: H on rows of the last third, region 60 full by five rows.  A spill count (or a done count)
    left behind by an earlier call makes a later one read that call's rows of H — lower row
    numbers — from the stale head of the spill list, which lowers its representatives."""
    rng = np.random.default_rng(seed)
    cap = region_capacity(n)
    H = mixed_keys(rng, 60, 8, 1)
    rng = np.random.default_rng(seed + ord(which[0]) + len(which))
    third = n // 3
    if which == "A":
        placed = [(np.repeat(H, cap + 700), 0, third)]
        parts = [bucket_rows(rng, 61, 8, cap + 900, 300), bucket_rows(rng, 62, 8, cap + 1500, 40)]
        return assemble(rng, n, parts, {60, 61, 62}, 8, placed), 0, \
            {60: "spill_lds", 61: "spill_lds", 62: "spill_lds"}, {"spill": 3100, "full": 3}
    if which == "A2":
        placed = [(np.repeat(H, cap), t * RPART_TILE, (t + 1) * RPART_TILE) for t in range(2)]
        return assemble(rng, n, [], {60}, 8, placed), 0, {60: "spill_lds"}, {"spill": cap, "full": 1}
    if which == "B":
        placed = [(np.repeat(H, cap + 1), third, 2 * third)]
        return assemble(rng, n, [], {60}, 8, placed), 0, {60: "spill_lds"}, {"spill": 1, "full": 1}
    if which == "C":
        placed = [(np.repeat(H, cap - 3), third, 2 * third)]
        return assemble(rng, n, [], {60}, 8, placed), 0, {60: "one_trip"}, {"spill": 0, "full": 0}
    assert which == "D"
    placed = [(np.repeat(H, cap + 5), 2 * third, n)]
    parts = [bucket_rows(rng, 70, 8, cap + 9, 30)]
    return assemble(rng, n, parts, {60, 70}, 8, placed), 0, {60: "spill_lds", 70: "spill_lds"}, \
        {"spill": 14, "full": 2}


# ---- the cases: id -> (generator, args) ---------------------------------------------------------
CASES = {}
for _d in (-1, 0, 1):
    CASES[f"S-region_at_cap{_d:+d}"] = (region_at_cap, (_d,))
for _t in (2, 3):
    CASES[f"S-fill_from_g_eq_cap-{_t}tiles"] = (fill_from_g_eq_cap, (_t,))
CASES["S-fill_in_one_tile"] = (fill_in_one_tile, ())
for _c in (1, 2, 3, 80):
    CASES[f"S-several_full-{_c}"] = (several_full, (_c,))
CASES["S-trips-8192"] = (trips, (8192,))
CASES["S-trips-8193"] = (trips, (8193,))
CASES["S-trips-16500"] = (trips, (16_500, 30_000))
CASES["S-fill_edge-10752"] = (fill_edge, (10_752, 12_000, 30_000))
CASES["S-fill_edge-10753"] = (fill_edge, (10_753, 12_000, 30_000))
CASES["S-fill_edge-claim_fail"] = (fill_edge, (16_385, 16_385, 40_000))
CASES["S-fill_edge-break_at_trip3"] = (fill_edge, (24_577, 24_577, 40_000))
CASES["S-two_carves"] = (two_carves, ())
CASES["S-probe_wrap"] = (probe_wrap, ())
CASES["S-global_home_wrap"] = (global_home_wrap, ())
CASES["S-vals_edges"] = (vals_edges, ())
CASES["S-dispatch_edge"] = (dispatch_edge, (BIG_MAX_KEYS,))
CASES["B-dispatch_edge"] = (dispatch_edge, (BIG_MAX_KEYS + 1,))
CASES["T-fine-rows2048"] = (t_segments, ("fine", {3: (2048, 300)}))
CASES["T-fine-rows2049"] = (t_segments, ("fine", {3: (2049, 300)}))
CASES["T-fine-distinct3584"] = (t_segments, ("fine", {5: (3700, 3584)}))
CASES["T-fine-distinct3585"] = (t_segments, ("fine", {5: (3700, 3585)}))
CASES["T-fine-distinct4096-no_free_slot"] = (t_segments, ("fine", {6: (4096, 4096)}))
CASES["T-fine-distinct4500-third_trip"] = (t_segments, ("fine", {6: (4500, 4500)}))
CASES["T-fine-empty_bucket0"] = (t_segments, ("fine", {7: (3700, 3600)}, (0,)))
CASES["T-fine-empty_last_bucket"] = (t_segments, ("fine", {7: (3700, 3600)}, (15,)))
CASES["T-fine-last_bucket_overflows_to_n"] = (t_segments, ("fine", {15: (3900, 3800)}))
CASES["T-fine-adjacent_own_tables"] = (t_segments, ("fine", {8: (4000, 3900), 9: (4100, 4000)}))
CASES["T-big-rows8192"] = (t_segments, ("big", {17: (8192, 300)}, (0,)))          # + an empty bucket 0
CASES["T-big-rows8193"] = (t_segments, ("big", {17: (8193, 300)}, (255,)))        # + an empty last bucket
CASES["T-big-distinct10752"] = (t_segments, ("big", {18: (11_000, 10_752)}))
CASES["T-big-distinct10753"] = (t_segments, ("big", {18: (11_000, 10_753)}))
CASES["T-big-claim_fail"] = (t_segments, ("big", {19: (16_385, 16_385)}))
CASES["B-three_full"] = (b_three_full, ())
CASES["B-fine-distinct3584"] = (b_fine_fill, (3584,))
CASES["B-fine-distinct3585"] = (b_fine_fill, (3585,))
for _w in ("A", "A2", "B", "C", "D"):
    CASES[f"S-seq-{_w}"] = (seq_call, (_w,))

# x and x + 1: (case below, case above, bucket) — the two must take different exits or trip counts
EDGE_PAIRS = [
    ("S-region_at_cap+0", "S-region_at_cap+1", 7), ("S-trips-8192", "S-trips-8193", 21),
    ("S-fill_edge-10752", "S-fill_edge-10753", 30),
    ("T-fine-rows2048", "T-fine-rows2049", 3), ("T-fine-distinct3584", "T-fine-distinct3585", 5),
    ("T-big-rows8192", "T-big-rows8193", 17), ("T-big-distinct10752", "T-big-distinct10753", 18),
    ("B-fine-distinct3584", "B-fine-distinct3585", 517),
]

# calls made in this order on one engine, every one checked (tests/test_group_edges_gpu.py)
SEQUENCES = {
    "spill_count_left_over": ["S-seq-A", "S-seq-B", "S-seq-C", "S-seq-D", "S-seq-C"],
    "done_count_after_g_eq_cap": ["S-seq-A2", "S-seq-D", "S-seq-B", "S-seq-D"],
    # each with overflowing buckets; S and B cannot share one n (BIG_MAX_KEYS divides them)
    "chains_T_S_B_S": ["T-fine-adjacent_own_tables", "S-two_carves", "B-fine-distinct3585",
                       "S-fill_edge-10753"],
}

_built = {}


def case_vals(keys, seed=77):
    """group_min's values: random u32, then the edges — 0 and 0xFFFFFFFF on a few rows, the most
    frequent key's minimum on its LAST row, and a repeated key whose every value is 0xFFFFFFFF
    (the table's initial value: nothing may be stored for it)."""
    rng = np.random.default_rng(seed + len(keys))
    n = len(keys)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    vals[rng.integers(0, n, 8)] = 0
    vals[rng.integers(0, n, 8)] = 0xFFFFFFFF
    uniq, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    order = np.argsort(-cnt, kind="stable")
    hot_rows = np.flatnonzero(inv == order[0])
    vals[hot_rows] = rng.integers(1000, 1 << 32, len(hot_rows), dtype=np.uint64).astype(np.uint32)
    vals[hot_rows[-1]] = 7
    if len(order) > 1 and cnt[order[1]] > 1:
        vals[inv == order[1]] = 0xFFFFFFFF
    return vals


def reference(keys, vals):
    """(rep, objects, mins): first row per distinct key, their count, min value per key — numpy."""
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    mins = np.full(len(uniq), 0xFFFFFFFF, dtype=np.uint32)
    np.minimum.at(mins, inv, vals)
    return first[inv].astype(np.uint32), len(uniq), mins[inv]


def build(case_id):
    """dict(keys, target, claims, facts, vals, rep, objects, mins) of a case id, made once per
    process and never written to."""
    if case_id not in _built:
        fn, args = CASES[case_id]
        keys, target, claims, facts = fn(*args)
        vals = case_vals(keys)
        rep, objects, mins = reference(keys, vals)
        for a in (keys, vals, rep, mins):
            a.setflags(write=False)
        _built[case_id] = dict(keys=keys, target=target, claims=claims, facts=facts, vals=vals,
                               rep=rep, objects=objects, mins=mins)
    return _built[case_id]


def table():
    """The record's table (profiles/group_edges/README.md): per case n, chain and, for every
    bucket that is claimed or leaves the common path, rows / distinct / spill / trips / exit."""
    lines = ["| case | n | chain | full regions, rows spilled | notable buckets: rows / distinct / own spill / trips / exit |",
             "|---|---|---|---|---|"]
    for case_id in CASES:
        c = build(case_id)
        m = model(c["keys"], c["target"])
        notable = sorted(set(c["claims"]) | {b for b, e in enumerate(m["exit"]) if e not in ("one_trip", "empty")})
        if len(notable) > 6:
            notable = notable[:3] + notable[-2:]
        cells = [f"region {r}: {int(m['region_rows'][r])} rows of capacity {m['cap']}"
                 for r in sorted(c["facts"].get("region_rows", {}))]
        for b in notable:
            sp = int(m["spill"][b]) if m["chain"] == "S" else 0
            tr = int(m["trips"][b])
            cells.append(f"{b}: {int(m['rows'][b])} / {int(m['distinct'][b])} / {sp} / {tr} / {m['exit'][b]}")
        reg = f"{int(m['full'].sum())}, {m['total_spill']}" if "full" in m else "-"
        lines.append(f"| `{case_id}` | {m['n']} | {m['chain']} | {reg} | {'; '.join(cells)} |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(table())
