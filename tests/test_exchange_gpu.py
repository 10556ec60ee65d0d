"""The small kernels of the multi-GPU exchange off their happy path (MI355X): the key-range
partition above 1,024 parts and over several trips, the fixed-capacity pack / split / unpack
kernels with crafted part sizes (spill blocks in use, the overflow threshold, no spill block,
non-power-of-two and full-width G, the grid-stride loop), the emulated exchange with every
spill block carrying rows, sd_cas_multi_group with empty, starved and flooded shards, and the
radix sort's partial bit ranges.  Every comparison is exact and covers every element; the
references are numpy (tests/exchange_ref.py, pinned to HostOps by tests/test_shard_cpu.py)
and Python's big-integer range_start."""
import numpy as np
import pytest

from spacedrive_amd.shard import range_start
from tests.exchange_ref import (emulate_fixed_exchange, pack_fixed_ref, pack_senders, part_offsets,
                                range_part, split_fixed_ref, unpack_fixed_ref)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EINVAL = -1


def dev64(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def dev32(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def host32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


# ---- 1. key-range partition ---------------------------------------------------------------

def check_partition(eng, keys: np.ndarray, parts: int):
    """eng.partition twice in a row on the same context (the totals / fill workspace must be
    left clean) against range_part; returns the second call's keys_out."""
    n = len(keys)
    dk = dev64(keys)
    want_part = range_part(keys, parts)
    want_counts = np.bincount(want_part, minlength=parts)
    seg = np.repeat(np.arange(parts), want_counts)  # the part that owns each output position
    for call in range(2):
        ko = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        po = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((parts,), -1, dtype=torch.int64, device="cuda")
        eng.partition(dk, parts, ko, po, counts)
        assert (counts.cpu().numpy() == want_counts).all(), call
        k, p = host64(ko), po.cpu().numpy()
        assert p.min() >= 0 and p.max() < n and (np.bincount(p, minlength=n) == 1).all(), call
        assert (keys[p] == k).all(), call
        got_part = range_part(k, parts)
        assert (np.diff(got_part) >= 0).all(), call  # part-contiguous in part order
        assert (got_part == seg).all(), call
    return k, seg


@pytest.mark.parametrize("parts", [1, 2, 3, 5, 64, 1000, 1023, 1024, 1025, 4096, 16383, 16384])
def test_partition_every_boundary(eng, parts):
    """5,000 random keys plus the first key of every range and its predecessor: the staged
    path up to 1,024 parts (LDS carving grows with parts), the unstaged one above.  The
    boundary keys' parts are checked against Python's exact range_start, not range_part."""
    rng = np.random.default_rng(1000 + parts)
    starts = np.array([range_start(r, parts) for r in range(1, parts)], dtype=np.uint64)
    keys = np.concatenate([rng.integers(0, 2 ** 64, 5000, dtype=np.uint64), starts, starts - np.uint64(1),
                           np.array([0, 2 ** 64 - 1], dtype=np.uint64)])
    keys = keys[rng.permutation(len(keys))]
    k, seg = check_partition(eng, keys, parts)
    if parts > 1:
        r = np.arange(1, parts)
        at = np.searchsorted(starts, k)  # k == starts[at] -> the first key of range at + 1
        first = (at < len(starts)) & (starts[np.minimum(at, len(starts) - 1)] == k)
        assert first.sum() >= parts - 1 and (seg[first] == r[at[first]]).all()
        at = np.searchsorted(starts - np.uint64(1), k)
        last = (at < len(starts)) & ((starts - np.uint64(1))[np.minimum(at, len(starts) - 1)] == k)
        assert last.sum() >= parts - 1 and (seg[last] == r[at[last]] - 1).all()
    assert seg[k == 0].tolist() == [0] * int((k == 0).sum())
    assert (seg[k == np.uint64(2 ** 64 - 1)] == parts - 1).all()


@pytest.mark.parametrize("parts,n,same", [
    (1025, 3, False), (16384, 3, False),           # n below parts, most parts empty
    (8, 100_000, True), (4096, 100_000, True),     # one identical key: one part takes all
    (16384, 600_001, False),                       # blocks walk several trips, unstaged
    (8, 4_200_000, False),                         # blocks walk several trips, staged
    (1025, 4096, False), (1025, 4097, False),      # one trip of one block; one key more
])
def test_partition_shapes(eng, parts, n, same):
    rng = np.random.default_rng(2000 + parts + n)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if same:
        keys[:] = keys[0]
    check_partition(eng, keys, parts)


# ---- 2a. pack_fixed / unpack_fixed with crafted part sizes ----------------------------------

FILL = 0x5A5A5A5A  # prefill of every output: an unwritten slot shows


def raw_pack(eng, keys, pos, counts, G, cap, spill, file0, null_spill=False):
    """sd_cas_exchange_pack_fixed_dev through the raw ABI -> (rc, rows, srows, flag)"""
    rows = torch.full((max(G * cap, 1), 3), FILL, dtype=torch.int32, device="cuda")
    srows = torch.full((max(G * spill, 1), 3), FILL, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = eng.L.sd_cas_exchange_pack_fixed_dev(
        eng.h, keys.data_ptr(), pos.data_ptr(), counts.data_ptr(), G, cap, spill, file0,
        rows.data_ptr(), None if null_spill else srows.data_ptr(), flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, host32(rows), host32(srows), int(flag.item())


def raw_unpack(eng, back, sback, pos, counts, G, cap, spill, n, null_spill=False):
    rep = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    rc = eng.L.sd_cas_exchange_unpack_fixed_dev(
        eng.h, back.data_ptr(), None if null_spill else sback.data_ptr(), pos.data_ptr(),
        counts.data_ptr(), G, cap, spill, rep.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, rep.cpu().numpy()[:n]


def crafted_inputs(rng, counts):
    n = int(sum(counts))
    return rng.integers(1, 2 ** 64, n, dtype=np.uint64), rng.permutation(n).astype(np.uint32)


def check_pack_unpack(eng, rng, keys, pos, counts, G, cap, spill, file0, want_flag, null_spill=False):
    """pack_fixed and unpack_fixed against the references, slot for slot; returns the device's
    (rows, srows).  keys and pos hold sum(counts) rows, so every index the kernels form from
    counts (t < min(count, cap + spill) past the part's offset) stays inside them."""
    n = len(keys)
    assert n == sum(counts) == len(pos)
    if n:
        dk, dp = dev64(keys), dev32(pos)
    else:  # unpack_fixed takes no n and refuses NULL: an empty sender still passes real pointers
        dk, dp = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    dc = torch.tensor(list(counts), dtype=torch.int64, device="cuda")
    rc, rows, srows, flag = raw_pack(eng, dk, dp, dc, G, cap, spill, file0, null_spill)
    assert rc == 0
    wrows, wsrows, wflag = pack_fixed_ref(keys, pos, counts, G, cap, spill, file0)
    assert wflag == want_flag  # the case is what it claims to be
    assert (rows[:G * cap] == wrows).all()
    if spill:
        assert (srows[:G * spill] == wsrows).all()
    else:
        assert (srows == FILL).all()
    assert flag == wflag
    back = rng.integers(0, 2 ** 32, G * cap, dtype=np.uint64).astype(np.uint32)
    sback = rng.integers(0, 2 ** 32, max(G * spill, 1), dtype=np.uint64).astype(np.uint32)
    rc, rep = raw_unpack(eng, dev32(back), dev32(sback), dp, dc, G, cap, spill, n, null_spill)
    assert rc == 0
    wrep, defined = unpack_fixed_ref(back, sback[:G * spill], pos, counts, G, cap, spill)
    assert defined.sum() == sum(min(c, cap + spill) for c in counts)
    assert (rep[defined] == wrep[defined]).all()
    return rows[:G * cap], srows[:G * spill]


EDGE_COUNTS = [0, 1, 299, 300, 301, 339, 340, 123]  # around cap = 300 and cap + spill = 340


def test_pack_unpack_fixed_spill_edges(eng):
    """Counts at 0, 1, cap - 1, cap, cap + 1, cap + spill - 1 and cap + spill: the spill
    blocks carry real rows, nothing overflows.  cap and spill are no multiples of 64, so
    waves straddle part and block edges."""
    rng = np.random.default_rng(31)
    keys, pos = crafted_inputs(rng, EDGE_COUNTS)
    check_pack_unpack(eng, rng, keys, pos, EDGE_COUNTS, 8, 300, 40, 123_456, want_flag=0)


@pytest.mark.parametrize("part", [0, 6])
def test_pack_unpack_fixed_one_row_too_many(eng, part):
    """The same with one part (an empty one; the exactly full one) raised to cap + spill + 1:
    the flag is set, and every other part's rows are what they were without it."""
    rng = np.random.default_rng(32)
    keys, pos = crafted_inputs(rng, EDGE_COUNTS)
    base_rows, base_srows = check_pack_unpack(eng, rng, keys, pos, EDGE_COUNTS, 8, 300, 40, 7, want_flag=0)
    counts = list(EDGE_COUNTS)
    extra = 341 - counts[part]
    at = int(part_offsets(counts)[part]) + counts[part]  # the part's end: other parts keep their rows
    counts[part] = 341
    keys2 = np.insert(keys, at, rng.integers(1, 2 ** 64, extra, dtype=np.uint64))
    pos2 = np.insert(pos, at, np.arange(len(pos), len(pos) + extra, dtype=np.uint32))
    rows, srows = check_pack_unpack(eng, rng, keys2, pos2, counts, 8, 300, 40, 7, want_flag=1)
    others = np.arange(8) != part
    assert (rows.reshape(8, 300, 3)[others] == base_rows.reshape(8, 300, 3)[others]).all()
    assert (srows.reshape(8, 40, 3)[others] == base_srows.reshape(8, 40, 3)[others]).all()


def test_pack_unpack_fixed_exactly_full(eng):
    """Every count <= cap + spill, one exactly cap + spill: not an overflow."""
    rng = np.random.default_rng(33)
    counts = [128, 64, 0, 127]
    keys, pos = crafted_inputs(rng, counts)
    check_pack_unpack(eng, rng, keys, pos, counts, 4, 64, 64, 0, want_flag=0)


@pytest.mark.parametrize("counts,want_flag", [([100, 99, 0], 0), ([101, 0, 0], 1)])
def test_pack_unpack_fixed_no_spill_block(eng, counts, want_flag):
    """spill == 0 with NULL spill pointers through the raw ABI."""
    rng = np.random.default_rng(34)
    keys, pos = crafted_inputs(rng, counts)
    check_pack_unpack(eng, rng, keys, pos, counts, 3, 100, 0, 99, want_flag, null_spill=True)


@pytest.mark.parametrize("G", [1, 3, 5, 7, 1000, 1023, 1024])
def test_pack_unpack_fixed_every_sentinel(eng, G):
    """cap 3, spill 2, counts cycling through 0..6: every part's sentinel against Python's exact
    ceil((p + 1) * 2^64 / G) (the device's 64-bit arithmetic at non-power-of-two G; 0 for the
    last part, so for G = 1), and the whole LDS offset array at G = 1024."""
    rng = np.random.default_rng(35 + G)
    counts = [i % 7 for i in range(G)]
    keys, pos = crafted_inputs(rng, counts)
    rows, _ = check_pack_unpack(eng, rng, keys, pos, counts, G, 3, 2, 1_000_000, want_flag=int(G >= 7))
    sent = rows.reshape(G, 3, 3)[0]  # part 0 is empty: three sentinel rows
    want = range_start(1, G)
    assert (sent[:, 0] == want & 0xFFFFFFFF).all() and (sent[:, 1] == want >> 32).all()
    if G == 1:
        assert want == 0


def test_pack_unpack_fixed_grid_stride(eng):
    """16.8 M slots, past the launch's 65,536 x 256 lanes: the grid-stride loop's second turn.
    file0 = 2^32 - n: the u32 global index reaches 2^32 - 1 and wraps nowhere."""
    rng = np.random.default_rng(36)
    cap, spill = 8_400_000, 100
    counts = [cap + 50, 5]
    assert 2 * (cap + spill) > 65536 * 256
    keys, pos = crafted_inputs(rng, counts)
    file0 = 2 ** 32 - len(keys)
    assert file0 + int(pos.max()) == 2 ** 32 - 1
    check_pack_unpack(eng, rng, keys, pos, counts, 2, cap, spill, file0, want_flag=0)


def test_pack_unpack_fixed_refusals(eng):
    """G = 0, G = 1025, cap = 0 and file0 = 2^32: SD_CAS_EINVAL, outputs untouched."""
    rng = np.random.default_rng(37)
    counts = [3, 2]
    keys, pos = crafted_inputs(rng, counts)
    dk, dp = dev64(keys), dev32(pos)
    dc = torch.zeros(1025, dtype=torch.int64, device="cuda")
    dc[:2] = torch.tensor(counts)
    for G, cap, file0 in [(0, 4, 0), (1025, 4, 0), (2, 0, 0), (2, 4, 2 ** 32)]:
        rc, rows, srows, flag = raw_pack(eng, dk, dp, dc, G, cap, 1, file0)
        assert rc == EINVAL, (G, cap, file0)
        assert (rows == FILL).all() and (srows == FILL).all() and flag == 0
    back = dev32(np.zeros(4100, dtype=np.uint32))
    for G, cap in [(0, 4), (1025, 4), (2, 0)]:
        rc, rep = raw_unpack(eng, back, back, dp, dc, G, cap, 1, 5)
        assert rc == EINVAL and (rep == -1).all(), (G, cap)
    # a spill block without its pointer
    rc, rows, srows, flag = raw_pack(eng, dk, dp, dc, 2, 4, 1, 0, null_spill=True)
    assert rc == EINVAL and (rows == FILL).all() and flag == 0
    rc, rep = raw_unpack(eng, back, back, dp, dc, 2, 4, 1, 5, null_spill=True)
    assert rc == EINVAL and (rep == -1).all()


def test_fixed_ops_rank_without_files(eng):
    """A rank holding no file goes through partition, pack_fixed and unpack_fixed: all its
    slots are sentinels, its rep is empty.  (sd_cas_exchange_unpack_fixed_dev takes no n and
    refuses NULL pos / rep, which is what empty torch tensors hand it: HipShardOps returns
    the empty rep itself; this raised EINVAL before.)"""
    from spacedrive_amd.shard import HipShardOps
    ops = HipShardOps(eng)
    G, cap, spill = 3, 5, 2
    pk, pp, cnt = ops.partition(torch.empty(0, dtype=torch.int64, device="cuda"), G)
    assert cnt.cpu().tolist() == [0] * G
    rows, srows, ovf = ops.pack_fixed(pk, pp, cnt, G, cap, spill, 1000)
    wrows, wsrows, wflag = pack_fixed_ref(np.zeros(0, np.uint64), np.zeros(0, np.uint32), [0] * G, G, cap, spill, 1000)
    assert (host32(rows) == wrows).all() and (host32(srows) == wsrows).all() and int(ovf.item()) == wflag == 0
    back = torch.zeros(G * cap, dtype=torch.int32, device="cuda")
    sback = torch.zeros(G * spill, dtype=torch.int32, device="cuda")
    rep = ops.unpack_fixed(back, sback, pp, cnt, G, cap, spill)
    assert rep.numel() == 0 and rep.dtype == torch.int64


# ---- 2b. split_fixed ------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2047, 2048, 2049, 100_003])
def test_split_fixed_densities(eng, m):
    """Around the kernel's 2,048-row block: no sentinel row, every row, rows in the last
    (partial) block only; sentinel 0 (the last rank's) and a high one."""
    from spacedrive_amd.shard import HipShardOps
    ops = HipShardOps(eng)
    rng = np.random.default_rng(40 + m)
    last = ((m - 1) // 2048) * 2048
    for sentinel in [0, range_start(1023, 1024)]:
        for density in ["none", "all", "last block"]:
            k = rng.integers(1, 2 ** 64, m, dtype=np.uint64)
            k[k == np.uint64(sentinel)] = np.uint64(1)
            if density == "all":
                k[:] = np.uint64(sentinel)
            elif density == "last block":
                k[last:] = np.uint64(sentinel)
            rows = np.empty((m, 3), dtype=np.uint32)
            rows[:, 0], rows[:, 1] = k & np.uint64(0xFFFFFFFF), k >> np.uint64(32)
            rows[:, 2] = rng.integers(0, 2 ** 32, m, dtype=np.uint64)
            rk, rv, nsent = ops.split_fixed(dev32(rows).view(m, 3), sentinel)
            wk, wv, wn = split_fixed_ref(rows, sentinel)
            assert wn == {"none": 0, "all": m, "last block": m - last}[density]
            assert int(nsent.item()) == wn, (sentinel, density)
            assert (host64(rk) == wk).all(), (sentinel, density)
            assert (host32(rv) == wv).all(), (sentinel, density)


# ---- 2c. the emulated exchange with every spill block in use ---------------------------------

@pytest.mark.parametrize("world", [3, 8])
def test_fixed_capacity_exchange_spill_in_use(eng, oracle, world):
    """A duplicated library: 20,000 keys per sender from a 30 %-duplicate pool and one hot key
    600 times on one sender.  cap = the smallest part - 1 and spill = the largest part - cap,
    so every part of every sender puts rows in its spill block and the largest fills it
    exactly: no flag, the canonical grouping, the exact Object count.  One spill row less and
    exactly the senders holding a largest part raise the flag."""
    from spacedrive_amd.shard import HipShardOps
    ops = HipShardOps(eng)
    rng = np.random.default_rng(60 + world)
    per = 20_000
    pool = rng.integers(0, 2 ** 64, int(0.7 * per * world), dtype=np.uint64)
    for r in range(world):
        b = range_start(r, world)
        pool[2 * r: 2 * r + 2] = [b, (b - 1) % 2 ** 64]
    senders = [pool[rng.integers(0, len(pool), per)] for _ in range(world)]
    hot = world // 2
    senders[hot] = np.concatenate([senders[hot], np.full(600, pool[100], dtype=np.uint64)])
    senders[hot] = senders[hot][rng.permutation(len(senders[hot]))]
    keys = np.concatenate(senders)
    cuts = [0] + np.cumsum([len(s) for s in senders]).tolist()
    counts = np.stack([np.bincount(range_part(s, world), minlength=world) for s in senders])
    cap = max(1, int(counts.min()) - 1)
    spill = int(counts.max()) - cap
    # properties of the inputs alone: every spill block is used, the largest part fills its own
    assert (counts > cap).all() and counts.max() == cap + spill and spill > 1
    flags, objects, rep = emulate_fixed_exchange(ops, keys, world, cap, spill, cuts)
    assert flags == [0] * world
    orep, oobj = oracle.group_canonical(keys)
    assert objects == oobj
    assert (rep == orep.astype(np.int64)).all()
    sent = pack_senders(ops, keys, world, cap, spill - 1, cuts)
    want = [int(c.max() == counts.max()) for c in counts]
    assert 0 < sum(want) < world
    assert [int(s[4].item()) for s in sent] == want


# ---- 3. sd_cas_multi_group on one device ------------------------------------------------------

def check_multi(me, oracle, shard_keys):
    parts = [dev64(k) for k in shard_keys]
    file0 = [0] + np.cumsum([len(k) for k in shard_keys]).tolist()[:-1]
    reps, objects = me.group(parts, file0)
    keys = np.concatenate(shard_keys)
    orep, oobj = oracle.group_canonical(keys)
    assert objects == oobj
    assert [r.numel() for r in reps] == [len(k) for k in shard_keys]
    got = np.concatenate([r.cpu().numpy() for r in reps])
    assert (got == orep.astype(np.int64)).all()


def boundary_pool(rng, shards, size):
    pool = rng.integers(0, 2 ** 64, size, dtype=np.uint64)
    for r in range(1, shards):  # keys exactly at / next to every range boundary ceil(r * 2^64 / G)
        b = -((-(r << 64)) // shards)
        pool[r * 3: r * 3 + 3] = [b - 1, b, min(b + 1, 2 ** 64 - 1)]
    return pool


@pytest.mark.parametrize("shards", [5, 7, 8])
def test_multi_group_more_shards(eng, oracle, shards):
    from spacedrive_amd.multi import MultiEngine
    rng = np.random.default_rng(70 + shards)
    pool = boundary_pool(rng, shards, 10_000)
    keys = pool[rng.integers(0, len(pool), 30_001)]
    cuts = [len(keys) * i // shards for i in range(shards + 1)]
    me = MultiEngine([0] * shards)
    check_multi(me, oracle, [keys[cuts[i]:cuts[i + 1]] for i in range(shards)])
    me.close()


def test_multi_group_empty_shards(eng, oracle):
    """Shards without files, first and in the middle."""
    from spacedrive_amd.multi import MultiEngine
    rng = np.random.default_rng(75)
    pool = boundary_pool(rng, 4, 9_000)
    sizes = [0, 30_001, 0, 7]
    me = MultiEngine([0] * 4)
    check_multi(me, oracle, [pool[rng.integers(0, len(pool), n)] for n in sizes])
    me.close()


def test_multi_group_one_range_receives_all(eng, oracle):
    """Every key below 2^60: range 0 receives four times its own shard (its buffers regrow
    after the sort, the sorted data copied over), ranges 1-3 receive nothing."""
    from spacedrive_amd.multi import MultiEngine
    rng = np.random.default_rng(76)
    pool = rng.integers(0, 2 ** 60, 25_000, dtype=np.uint64)
    me = MultiEngine([0] * 4)
    check_multi(me, oracle, [pool[rng.integers(0, len(pool), 20_000)] for _ in range(4)])
    me.close()


def test_multi_group_reused_with_other_sizes(eng, oracle):
    """One sd_cas_multi called with 90,001, then 1,000, then 200,003 keys: the buffers are
    kept, their layout changes."""
    from spacedrive_amd.multi import MultiEngine
    rng = np.random.default_rng(77)
    me = MultiEngine([0] * 4)
    for n in [90_001, 1_000, 200_003]:
        pool = boundary_pool(rng, 4, max(n // 3, 16))
        keys = pool[rng.integers(0, len(pool), n)]
        cuts = [n * i // 4 for i in range(5)]
        check_multi(me, oracle, [keys[cuts[i]:cuts[i + 1]] for i in range(4)])
    me.close()


# ---- 5. radix sort bit ranges -------------------------------------------------------------------

@pytest.mark.parametrize("begin,end", [(0, 1), (63, 64), (0, 8), (0, 9), (0, 16), (7, 17), (31, 33),
                                       (0, 32), (5, 64), (48, 64)])
def test_sort_pairs_bit_ranges(eng, begin, end):
    """1-, 2-, 4- and 8-pass ranges (an even pass count starts in the alternate buffer), 1-bit
    digits, a range that ends at bit 64 off a byte boundary, begin_bit 63: stable on the
    masked key, with the iota and with a caller's permutation as values."""
    rng = np.random.default_rng(80 + 64 * begin + end)
    mask = np.uint64((1 << (end - begin)) - 1)
    for n in [1, 4097, 100_003]:
        k = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
        k[: n // 3] = k[n // 2]  # a third of the keys tied: stability matters
        order = np.argsort((k >> np.uint64(begin)) & mask, kind="stable")
        v = rng.permutation(n).astype(np.int32)
        for vals, want_v in [(None, order), (v, v[order])]:
            ko = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            vo = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            eng.sort_pairs(dev64(k), None if vals is None else torch.from_numpy(vals).cuda(), ko, vo, begin, end)
            assert (host64(ko) == k[order]).all(), (n, vals is None)
            assert (vo.cpu().numpy() == want_v).all(), (n, vals is None)
