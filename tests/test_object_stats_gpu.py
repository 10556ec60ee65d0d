"""Object statistics on the device (object_stats.hip): copies per Object, the eight totals
and the top duplicate sets, every comparison exact integer equality against the numpy
restatement of the definitions (tests/test_object_stats_cpu.py: np_group / np_stats / np_top,
checked there against a hand-worked example).  Under the debug library the conservation check
of the finalize pass (the heads' copies add up to the valid rows) runs in every test here."""
import numpy as np
import pytest
import torch

from spacedrive_amd import NO_OBJECT, SAMPLED_CONTENT_LEN, TOP_MAX, TOP_TILE, CasEngine, CasError
from tests.test_object_stats_cpu import STAT_NAMES, np_group, np_stats, np_top

pytestmark = pytest.mark.gpu

T = TOP_TILE  # rows per tile of the top list's stable compaction (sd_object_stats.h)
ROW_HASHED, ROW_NO_CAS, ROW_ERROR = 0, 1, 2


def dup_keys(rng, n, frac=0.3):
    """n keys of which about `frac` repeat another row's."""
    keys = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    dup = np.nonzero(rng.random(n) < frac)[0]
    keys[dup] = keys[rng.integers(0, n, len(dup))]
    return keys


def mix_sizes(keys, bits=40):
    """size = 1 + mix(key) % 2^bits: equal keys share a size."""
    z = keys * np.uint64(0x9E3779B97F4A7C15)
    z ^= z >> np.uint64(29)
    return np.uint64(1) + (z & np.uint64((1 << bits) - 1))


def d32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def d64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def h32(t):
    return t.cpu().numpy().view(np.uint32)


def h64(t):
    return t.cpu().numpy().view(np.uint64)


def device_group(eng, keys):
    k = d64(keys)
    rep = torch.empty(len(keys), dtype=torch.int32, device="cuda")
    eng.group(k, rep)
    return rep


def run_stats(eng, rep_d, sizes_d):
    copies = torch.full((rep_d.numel(),), -7, dtype=torch.int32, device="cuda")  # junk: no memset needed
    totals = eng.object_stats(rep_d, sizes_d, copies)
    return copies, totals


def run_top(eng, rep_d, sizes_d, copies_d, k):
    heads = torch.full((k,), 5, dtype=torch.int32, device="cuda")
    waste = torch.full((k,), 5, dtype=torch.int64, device="cuda")
    found = eng.top_duplicates(rep_d, sizes_d, copies_d, k, heads, waste)
    return h32(heads), h64(waste), found


def check_all(eng, keys, sizes, k=None):
    """Group on the device and in numpy, feed both to object_stats, compare copies, totals
    and (k given) the top list."""
    want_rep, want_copies = np_group(keys)
    _, want_t = np_stats(want_rep, sizes)
    sz = d64(sizes)
    rep_dev = device_group(eng, keys)
    assert (h32(rep_dev) == want_rep).all()
    for rep_d in (rep_dev, d32(want_rep)):
        copies, t = run_stats(eng, rep_d, sz)
        assert (h32(copies) == want_copies).all()
        assert t == want_t
    if k is not None:
        th, tw, found = run_top(eng, rep_d, sz, copies, k)
        wh, ww, wf = np_top(want_rep, sizes, want_copies, k)
        assert found == wf and (th == wh).all() and (tw == ww).all()
    return want_t


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1025, T - 1, T, T + 1, 2 * T + 1])
def test_sizes_of_n(eng, n):
    rng = np.random.default_rng(1000 + n)
    keys = dup_keys(rng, n)
    check_all(eng, keys, mix_sizes(keys), k=min(n, 7))


def test_no_rows(eng):
    e32 = torch.empty(0, dtype=torch.int32, device="cuda")
    e64 = torch.empty(0, dtype=torch.int64, device="cuda")
    assert eng.object_stats(e32, e64, e32) == dict.fromkeys(STAT_NAMES, 0)
    totals = torch.full((8,), 9, dtype=torch.int64, device="cuda")
    assert eng.object_stats(e32, e64, e32, totals=totals, want_totals=False) is None
    torch.cuda.synchronize()
    assert (totals == 0).all()
    th, tw, found = run_top(eng, e32, e64, e32, 3)
    assert found == 0 and (th == NO_OBJECT).all() and (tw == 0).all()


def test_all_distinct(eng):
    n = 200_003
    keys = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))  # odd multiplier: a bijection
    sizes = mix_sizes(keys)
    t = check_all(eng, keys, sizes, k=10)
    assert t["duplicate_sets"] == 0 and t["max_copies"] == 1 and t["objects"] == n
    assert t["unique_bytes"] == t["total_bytes"]
    rep = d32(np.arange(n))
    copies, _ = run_stats(eng, rep, d64(sizes))
    th, tw, found = run_top(eng, rep, d64(sizes), copies, 10)
    assert found == 0 and (th == NO_OBJECT).all() and (tw == 0).all()


def test_one_hot_key(eng):
    n, size = 200_003, 123_457
    keys = np.full(n, 0xABCDEF0123456789, dtype=np.uint64)
    sizes = np.full(n, size, dtype=np.uint64)
    t = check_all(eng, keys, sizes, k=4)
    assert t["objects"] == 1 and t["max_copies"] == n and t["rows"] == n
    rep = torch.zeros(n, dtype=torch.int32, device="cuda")
    copies, _ = run_stats(eng, rep, d64(sizes))
    assert (h32(copies) == n).all()
    th, tw, found = run_top(eng, rep, d64(sizes), copies, 4)
    assert found == 1 and th.tolist() == [0] + [NO_OBJECT] * 3 and tw.tolist() == [(n - 1) * size, 0, 0, 0]


def test_two_hot_keys_alternating(eng):
    """Neighbouring lanes never share a head: two leaders are peeled per wave."""
    n = 100_000
    keys = np.where(np.arange(n) % 2 == 0, np.uint64(11), np.uint64(22)).astype(np.uint64)
    sizes = np.where(np.arange(n) % 2 == 0, np.uint64(1000), np.uint64(3000)).astype(np.uint64)
    t = check_all(eng, keys, sizes, k=2)
    assert t["objects"] == 2 and t["max_copies"] == n // 2
    rep = d32(np.arange(n) % 2)
    copies, _ = run_stats(eng, rep, d64(sizes))
    th, tw, found = run_top(eng, rep, d64(sizes), copies, 2)
    assert found == 2 and th.tolist() == [1, 0] and tw.tolist() == [49_999 * 3000, 49_999 * 1000]


def test_many_heads_per_wave(eng):
    """More distinct heads in a wave than leaders are peeled: the per-lane fallback."""
    n = 64 * 50
    keys = (np.arange(n, dtype=np.uint64) % np.uint64(37)) + np.uint64(5)
    check_all(eng, keys, mix_sizes(keys), k=37)


def test_wide_sums(eng):
    """Sizes near 2^45: TOTAL_BYTES > 2^53 and one waste > 2^53 — no float, no 32-bit path."""
    rng = np.random.default_rng(45)
    n = 4096
    keys = dup_keys(rng, n)
    keys[rng.choice(n, 600, replace=False)] = np.uint64(0x7777777777777777)
    sizes = np.uint64(1 << 45) + mix_sizes(keys, bits=20)
    want_rep, want_copies = np_group(keys)
    wh, ww, _ = np_top(want_rep, sizes, want_copies, 50)
    t = check_all(eng, keys, sizes, k=50)
    assert t["total_bytes"] > 1 << 53 and int(ww[0]) > 1 << 53 and wh[0] != NO_OBJECT


@pytest.fixture(scope="module")
def tie_case():
    """1,000 duplicate pairs of equal waste, heads every 49 rows across two multiples of T,
    single rows between them; n = 3T + 7."""
    n = 3 * T + 7
    keys = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    heads = np.arange(1000) * 49
    assert heads[-1] + 1 < 3 * T and (heads < T).any() and ((heads > T) & (heads < 2 * T)).any() and (heads > 2 * T).any()
    keys[heads + 1] = keys[heads]
    sizes = mix_sizes(keys)
    sizes[heads] = 4096
    sizes[heads + 1] = 4096
    return keys, sizes, heads


@pytest.mark.parametrize("k", [10, 1, 1000, 1500])
def test_ties_across_the_cut_and_tiles(eng, tie_case, k):
    keys, sizes, heads = tie_case
    rep_d, sz = device_group(eng, keys), d64(sizes)
    copies, t = run_stats(eng, rep_d, sz)
    assert t["duplicate_sets"] == 1000
    th, tw, found = run_top(eng, rep_d, sz, copies, k)
    f = min(k, 1000)
    assert found == f
    assert th[:f].tolist() == heads[:f].tolist() and (tw[:f] == 4096).all()
    assert (th[f:] == NO_OBJECT).all() and (tw[f:] == 0).all()
    want_rep, want_copies = np_group(keys)
    wh, ww, wf = np_top(want_rep, sizes, want_copies, k)
    assert wf == f and (th == wh).all() and (tw == ww).all()


def test_top_k_limit(eng, tie_case):
    keys, sizes, _ = tie_case
    rep_d, sz = device_group(eng, keys), d64(sizes)
    copies, _ = run_stats(eng, rep_d, sz)
    k = TOP_MAX + 1
    heads = torch.zeros(k, dtype=torch.int32, device="cuda")
    waste = torch.zeros(k, dtype=torch.int64, device="cuda")
    with pytest.raises(CasError) as e:
        eng.top_duplicates(rep_d, sz, copies, k, heads, waste)
    assert e.value.code == -1  # SD_CAS_EINVAL
    assert eng.top_duplicates(rep_d, sz, copies, 0, heads[:0], waste[:0]) == 0


def test_mixed_waste(eng):
    rng = np.random.default_rng(77)
    n = 200_003
    keys = dup_keys(rng, n)
    sizes = mix_sizes(keys)
    check_all(eng, keys, sizes, k=100)
    # the order is fully determined: a second run gives the identical list
    rep_d, sz = device_group(eng, keys), d64(sizes)
    copies, _ = run_stats(eng, rep_d, sz)
    a = run_top(eng, rep_d, sz, copies, 100)
    b = run_top(eng, rep_d, sz, copies, 100)
    assert a[2] == b[2] == 100 and (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_more_tiles_than_one_scan_tile(eng):
    """n = 4,096 T + 5 rows (past 2^26): the compaction's tile counts no longer fit one tile of
    the device-wide scan.  Built and checked on the device / in closed form: a pair every
    1,000 rows (head 1000 j, member 1000 j + 1), size(i) = i % 7,919 + 1."""
    n = 4096 * T + 5
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    sizes = i % 7919 + 1
    member = i % 1000 == 1
    rep = torch.where(member, i - 1, i).to(torch.int32)
    want_copies = (1 + (member | (i % 1000 == 0) & (i + 1 < n)).to(torch.int32))
    pairs = int(member.sum().item())
    total = int(sizes.sum().item())
    member_bytes = int(sizes[member].sum().item())
    del i, member
    copies, t = run_stats(eng, rep, sizes)
    assert torch.equal(copies, want_copies)
    assert t == {"rows": n, "objects": n - pairs, "total_bytes": total, "unique_bytes": total - member_bytes,
                 "duplicate_sets": pairs, "max_copies": 2, "size_mismatch_rows": pairs, "bad_rows": 0}
    heads = np.arange(pairs, dtype=np.int64) * 1000
    waste = heads % 7919 + 1  # one extra copy of the head's size
    order = np.lexsort((heads, -waste))
    for k in (1, 300):
        th, tw, found = run_top(eng, rep, sizes, copies, k)
        assert found == k and th.tolist() == heads[order[:k]].tolist() and tw.tolist() == waste[order[:k]].tolist()


def test_workspace_grows_inside_top_duplicates():
    """A fresh context (1 MiB of workspace, no grouping before) and 100,000 candidates in one
    bin: the candidate and sort buffers do not fit, the workspace grows after the selection
    and the selection runs again — same answer."""
    n = 200_000
    rep = d32(np.arange(n) & ~1)  # pairs (2j, 2j + 1)
    sizes = torch.full((n,), 4096, dtype=torch.int64, device="cuda")
    e = CasEngine(0)
    try:
        copies, t = run_stats(e, rep, sizes)
        assert t["duplicate_sets"] == n // 2 and t["max_copies"] == 2 and (h32(copies) == 2).all()
        for _ in range(2):  # growing, then grown
            th, tw, found = run_top(e, rep, sizes, copies, 50)
            assert found == 50 and th.tolist() == list(range(0, 100, 2)) and (tw == 4096).all()
    finally:
        e.close()


def test_size_mismatch(eng):
    rng = np.random.default_rng(5)
    n = 3000
    keys = dup_keys(rng, n)
    sizes = mix_sizes(keys)
    rep, _ = np_group(keys)
    nonhead = np.nonzero(rep != np.arange(n))[0]
    sizes[nonhead[3]] += np.uint64(1)
    sizes[nonhead[-1]] += np.uint64(5)
    want_copies, want_t = np_stats(rep, sizes)
    assert want_t["size_mismatch_rows"] == 2
    copies, t = run_stats(eng, d32(rep), d64(sizes))
    assert t == want_t and (h32(copies) == want_copies).all()
    heads = rep == np.arange(n)
    assert t["unique_bytes"] == sum(sizes[heads].tolist())


def test_bad_rows(eng):
    """rep that is not a grouping: the rows are counted, never followed."""
    n = 1000
    keys = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    rng = np.random.default_rng(6)
    dst = np.arange(100, n)[rng.random(n - 100) < 0.4]
    keys[dst] = keys[rng.integers(40, 100, len(dst))]
    keys[5] = keys[2]  # row 5 is not a head
    sizes = mix_sizes(keys)
    rep, _ = np_group(keys)
    assert rep[5] == 2 and all(rep[r] == r and (rep == r).sum() == 1 for r in (10, 20, 30))
    rep[10], rep[20], rep[30] = 11, 1000, 5
    want_copies, want_t = np_stats(rep, sizes)
    assert want_t["bad_rows"] == 3 and want_t["rows"] == n - 3
    rep_d, sz = d32(rep), d64(sizes)
    copies = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(CasError) as e:
        eng.object_stats(rep_d, sz, copies)
    assert e.value.code == -1 and "3 rows" in str(e.value)
    copies.fill_(-1)
    totals = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    assert eng.object_stats(rep_d, sz, copies, totals=totals, want_totals=False) is None
    torch.cuda.synchronize()
    got = dict(zip(STAT_NAMES, h64(totals).tolist()))
    assert got == want_t
    c = h32(copies)
    assert (c == want_copies).all() and c[10] == c[20] == c[30] == 0
    # the top list reads heads only: it is safe, and exact over the valid heads
    th, tw, found = run_top(eng, rep_d, sz, copies, 20)
    wh, ww, wf = np_top(rep, sizes, want_copies, 20)
    assert found == wf and (th == wh).all() and (tw == ww).all()


def test_product_path(eng):
    """The fused hash + group chain's rep and the sizes its K1 read, straight into object_stats."""
    n = eng.batch_quantum
    content = torch.empty((n, SAMPLED_CONTENT_LEN), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(0x0B5, 0, n, content, sizes, SAMPLED_CONTENT_LEN, dup_permille=300)
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    rep = torch.zeros(n, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    objects = eng.hash_group_sampled(content, sizes, keys, rep, ovf)
    copies, t = run_stats(eng, rep, sizes)
    hk, hs = h64(keys), h64(sizes)
    want_rep, want_copies = np_group(hk)
    _, want_t = np_stats(want_rep, hs)
    assert (h32(rep) == want_rep).all() and (h32(copies) == want_copies).all()
    assert t == want_t and t["objects"] == objects and 0.2 * n < n - objects < 0.4 * n
    assert t["size_mismatch_rows"] == 0
    th, tw, found = run_top(eng, rep, sizes, copies, 100)
    wh, ww, wf = np_top(want_rep, hs, want_copies, 100)
    assert found == wf and (th == wh).all() and (tw == ww).all()
    del content
    torch.cuda.empty_cache()


def test_host_form(eng):
    rng = np.random.default_rng(50)
    n, k = 50_000, 64
    keys = dup_keys(rng, n)
    sizes = mix_sizes(keys)
    state = rng.choice([ROW_HASHED, ROW_NO_CAS, ROW_ERROR], n, p=[0.8, 0.1, 0.1]).astype(np.uint8)
    off = state != ROW_HASHED
    keys[off] = rng.integers(0, 1 << 63, int(off.sum()), dtype=np.uint64)  # garbage: never read
    sizes[off] = rng.integers(0, 1 << 62, int(off.sum()), dtype=np.uint64)
    idx = np.nonzero(~off)[0]
    crep, ccopies = np_group(keys[idx])
    want_rep = np.full(n, NO_OBJECT, dtype=np.uint32)
    want_rep[idx] = idx[crep]
    want_copies = np.zeros(n, dtype=np.uint32)
    want_copies[idx] = ccopies
    c2, want_t = np_stats(want_rep, sizes, hashed=~off)
    assert (c2 == want_copies).all() and want_t["rows"] == len(idx) and want_t["bad_rows"] == 0
    r = eng.duplicate_report(keys, sizes, state, k=k)
    assert (r.rep == want_rep).all() and (r.copies == want_copies).all()
    assert (r.rep[off] == NO_OBJECT).all() and (r.copies[off] == 0).all()
    assert r.totals == want_t
    wh, ww, wf = np_top(want_rep, sizes, want_copies, k)
    assert wf == k and (r.top_heads == wh).all() and (r.top_waste == ww).all()
    # every row hashed: the device path's answer
    r2 = eng.duplicate_report(keys, sizes, None, k=k)
    sz = d64(sizes)
    rep_d = device_group(eng, keys)
    copies, t = run_stats(eng, rep_d, sz)
    th, tw, _ = run_top(eng, rep_d, sz, copies, k)
    assert (r2.rep == h32(rep_d)).all() and (r2.copies == h32(copies)).all() and r2.totals == t
    assert (r2.top_heads == th).all() and (r2.top_waste == tw).all()
    # no row hashed, and outputs not wanted
    r3 = eng.duplicate_report(keys[:100], sizes[:100], np.full(100, ROW_ERROR, dtype=np.uint8), k=2)
    assert r3.totals == dict.fromkeys(STAT_NAMES, 0) and (r3.rep == NO_OBJECT).all()
    assert r3.top_heads.tolist() == [NO_OBJECT] * 2


def test_streams_and_a_second_context(eng):
    """Inputs produced on a side stream and measured there (the shared workspace is ordered
    across streams by its event); a context created afterwards gives the same answer."""
    n = 150_001
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        keys = torch.empty(n, dtype=torch.int64, device="cuda")
        eng.synth_roots(0x57A7, 0, n, keys, dup_permille=300)
        sizes = (keys & 0xFFFFFFFFFF) + 1
        rep = torch.empty(n, dtype=torch.int32, device="cuda")
        eng.group(keys, rep, want_objects=False)
        copies = torch.empty(n, dtype=torch.int32, device="cuda")
        totals = torch.empty(8, dtype=torch.int64, device="cuda")
        assert eng.object_stats(rep, sizes, copies, totals=totals, want_totals=False) is None
        # a grouping on the default stream right behind it shares the workspace
        rep0 = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().wait_stream(side)
    eng.group(keys, rep0, want_objects=False)
    side.synchronize()
    torch.cuda.synchronize()
    hk, hs = h64(keys), h64(sizes)
    want_rep, want_copies = np_group(hk)
    _, want_t = np_stats(want_rep, hs)
    assert (h32(rep) == want_rep).all() and (h32(rep0) == want_rep).all()
    assert (h32(copies) == want_copies).all()
    assert dict(zip(STAT_NAMES, h64(totals).tolist())) == want_t
    assert 0.2 * n < n - want_t["objects"] < 0.4 * n
    e2 = CasEngine(0)
    try:
        rep2 = torch.empty(n, dtype=torch.int32, device="cuda")
        e2.group(keys, rep2)
        copies2 = torch.empty(n, dtype=torch.int32, device="cuda")
        assert e2.object_stats(rep2, sizes, copies2) == want_t
        assert torch.equal(copies2, copies)
        a = run_top(eng, rep, sizes, copies, 50)
        b = run_top(e2, rep2, sizes, copies2, 50)
        wh, ww, wf = np_top(want_rep, hs, want_copies, 50)
        assert a[2] == b[2] == wf and (a[0] == b[0]).all() and (a[0] == wh).all() and (a[1] == ww).all()
        assert (b[1] == ww).all()
    finally:
        e2.close()
