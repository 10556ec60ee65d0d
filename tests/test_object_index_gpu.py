"""GPU tests of the library-resident Object index (sd_cas_index_*, spacedrive_amd/csrc/
object_index.hip) and of the link emission that reads it (sd_cas_identifier_links_indexed[_dev]).

Every result is compared with the dict model of tests/index_cases.py: `check` compares the
exported pairs as a set and ENTRIES with the model after every step.  Probe chains are built with
the inverse of the table's hash, and LAST_MAX_PROBE says that a chain really was what the case
claims.  Caller buffers sit behind the fences of tests/fence.py.  The indexed link emission is
held to the seeded one given the index's exported pairs, output for output."""
import ctypes

import numpy as np
import pytest

from tests import index_cases as ic
from tests import links_cases as lc
from tests.fence import DevFence, DevInput, check_all

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EINVAL = -1
BATCHES = (1, 63, 64, 65, 1000)


def u64(a):
    return np.asarray(a, dtype=np.uint64).reshape(-1)


def u32(a):
    return np.asarray(a, dtype=np.uint32).reshape(-1)


def dev64(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()


def dev32(a):
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def put(ix, model, keys, ids, stream=None):
    """insert_dev behind fences.  The ids' guards hold 2^31: an id read past the batch would
    refuse it."""
    k, i = DevInput(u64(keys), np.uint64(0)), DevInput(u32(ids), np.uint32(1 << 31))
    ix.insert(k.t, i.t, stream=stream)
    model.insert(u64(keys), u32(ids))
    check_all(k, i)


def find(ix, keys):
    k, out = DevInput(u64(keys), np.uint64(0)), DevFence(np.uint32, len(u64(keys)))
    ix.lookup(k.t, out=out.t)
    got = out.host()
    check_all(k, out)
    return got


def drop(ix, model, keys):
    k = DevInput(u64(keys), np.uint64(0))
    ix.erase(k.t)
    model.erase(u64(keys))
    check_all(k)


def exported(eng, ix, cap):
    """sd_cas_index_export_dev into fenced buffers of `cap` pairs: (rc, n, keys, ids)."""
    fk, fo = DevFence(np.uint64, cap), DevFence(np.uint32, cap)
    n = ctypes.c_uint64(0xDEAD)
    rc = eng.L.sd_cas_index_export_dev(eng.h, ix.handle, fk.ptr if cap else None, fo.ptr if cap else None,
                                       cap, ctypes.byref(n), int(torch.cuda.current_stream().cuda_stream))
    k, o = fk.host(), fo.host()
    check_all(fk, fo)
    return rc, int(n.value), k, o


def check(eng, ix, model):
    """The index is the model: ENTRIES, the exported pairs as a set, and a lookup of every key."""
    st = ix.stats()
    assert st["entries"] == len(model) == len(ix)
    rc, n, k, o = exported(eng, ix, len(model))
    assert rc == 0 and n == len(model)
    pairs = list(zip(k.tolist(), o.tolist()))
    assert len(set(pairs)) == len(pairs) and set(pairs) == model.pairs()
    if model:
        keys = u64(list(model))
        assert (find(ix, keys) == model.lookup(keys)).all()
    return st


def log2_slots(ix):
    return ix.stats()["slots"].bit_length() - 1


# ---- keys, minima, chains, tombstones -------------------------------------------------------

def test_special_keys_insert_lookup_erase_insert(eng):
    """0, 1, 2^64 - 1 and 2^64 - 2 (the words the table reserves) and the pre-images of 0, 1 and
    2^64 - 1 under the hash (slot 0 and the last slot)."""
    sp = ic.special_keys()
    with eng.object_index() as ix:
        model = ic.Model()
        put(ix, model, sp, 100 + np.arange(len(sp)))
        check(eng, ix, model)
        assert (find(ix, sp) == model.lookup(sp)).all() and ic.NONE not in find(ix, sp)
        drop(ix, model, sp)
        assert not model and (find(ix, sp) == ic.NONE).all()
        check(eng, ix, model)
        put(ix, model, sp, 7000 - np.arange(len(sp)))          # larger ids than before: no stale minimum
        check(eng, ix, model)
        put(ix, model, sp[2:4], [5, 6])                        # the side keys take a minimum too
        assert find(ix, sp[2:4]).tolist() == [5, 6]
        check(eng, ix, model)


def test_one_key_many_times_the_minimum_wins(eng):
    key = 0x1234_5678_9ABC_DEF0
    with eng.object_index() as ix:
        model = ic.Model()
        put(ix, model, [key] * 4096, 10_000 - np.arange(4096))   # descending: 64 waves, the last holds the min
        assert find(ix, [key]).tolist() == [10_000 - 4095]
        assert check(eng, ix, model)["entries"] == 1
        for ids in ([900], [300], [600]):                        # and across batches
            put(ix, model, [key], ids)
        assert find(ix, [key]).tolist() == [300]
        check(eng, ix, model)


@pytest.mark.parametrize("case", ["one_home_64_two_batches", "one_home_200", "wraps", "runs_into_next",
                                  "full_wave"])
def test_probe_chains(eng, case):
    with eng.object_index() as ix:
        model = ic.Model()
        lg = log2_slots(ix)
        slots = 1 << lg
        if case == "one_home_64_two_batches":
            keys = ic.keys_with_home(517, lg, 64)
            put(ix, model, keys[:32], np.arange(32))
            put(ix, model, keys[32:], 32 + np.arange(32))
            built = 64
        elif case == "one_home_200":
            keys = ic.keys_with_home(517, lg, 200)
            put(ix, model, keys, np.arange(200))
            built = 200
        elif case == "wraps":                                    # home = the last slot
            keys = ic.keys_with_home(slots - 1, lg, 64)
            put(ix, model, keys, np.arange(64))
            built = 64
        elif case == "runs_into_next":                           # 40 keys at h, then 30 at h + 1
            a, b = ic.keys_with_home(300, lg, 40), ic.keys_with_home(301, lg, 30)
            put(ix, model, a, np.arange(40))
            put(ix, model, b, 40 + np.arange(30))
            keys, built = np.concatenate([a, b]), 39 + 30        # h + 1's last key walks over both
        else:                                                    # one wave, 64 lanes, one home
            keys = ic.keys_with_home(9, lg, 64)
            put(ix, model, keys, 64 - np.arange(64))
            built = 64
        assert ix.stats()["last_max_probe"] >= built             # of that insert
        assert (find(ix, keys) == model.lookup(keys)).all()
        assert ix.stats()["last_max_probe"] >= built             # of that lookup
        absent = ic.keys_with_home(ic.home(int(keys[-1]), lg), lg, 3, first=1000)
        assert (find(ix, absent) == ic.NONE).all()               # walks the chain to its end
        st = check(eng, ix, model)
        assert st["slots"] == slots and st["rehashes"] == 0


def test_tombstones_do_not_cut_a_chain(eng):
    with eng.object_index() as ix:
        model = ic.Model()
        lg = log2_slots(ix)
        keys = ic.keys_with_home(77, lg, 64)
        put(ix, model, keys, 1000 + np.arange(64))
        gone = keys[[0, 31, 63]]
        drop(ix, model, gone)
        assert (find(ix, keys) == model.lookup(keys)).all() and (find(ix, gone) == ic.NONE).all()
        check(eng, ix, model)
        drop(ix, model, ic.keys_with_home(77, lg, 2, first=500))   # absent: a no-op
        drop(ix, model, [keys[5]] * 130)                           # repeated in one batch, over waves
        st = check(eng, ix, model)
        assert st["tombstones"] == 4 and st["entries"] == 60
        put(ix, model, [keys[0]], [999_999])                       # back, with a larger id than it had
        assert find(ix, [keys[0]]).tolist() == [999_999]
        st = check(eng, ix, model)
        assert st["tombstones"] == 4                               # a tombstone is never reused
        assert ix.stats()["last_max_probe"] >= 61                  # the lookups walk over them


# ---- growth and compaction -------------------------------------------------------------------

def test_growth_loses_nothing(eng):
    rng = np.random.default_rng(20)
    keys = np.unique(rng.integers(0, 1 << 64, 5200, dtype=np.uint64))[:5000]
    keys = rng.permutation(keys)
    ids = rng.integers(0, 1 << 31, 5000, dtype=np.uint32)
    with eng.object_index() as ix:
        model = ic.Model()
        assert ix.stats()["slots"] == ic.MIN_SLOTS
        at = k = 0
        while at < 5000:
            n = min(BATCHES[k % len(BATCHES)], 5000 - at)
            put(ix, model, keys[at:at + n], ids[at:at + n])
            at, k = at + n, k + 1
        st = check(eng, ix, model)
        assert st["rehashes"] >= 3 and st["entries"] == 5000 and st["tombstones"] == 0
        assert st["slots"] > 5000 and st["slots"] & (st["slots"] - 1) == 0


def test_batch_that_trips_the_bound_carries_present_keys(eng):
    rng = np.random.default_rng(21)
    keys = rng.permutation(np.unique(rng.integers(0, 1 << 64, 700, dtype=np.uint64))[:600])
    with eng.object_index() as ix:
        model = ic.Model()
        put(ix, model, keys[:400], 1000 + np.arange(400))
        before = ix.stats()
        # 200 keys the table holds (half with a smaller id, half with a larger) + 200 new ones
        batch = np.concatenate([keys[:200], keys[400:]])
        ids = np.concatenate([np.arange(100), 5000 + np.arange(100), 9000 + np.arange(200)])
        order = rng.permutation(400)
        put(ix, model, batch[order], ids[order])
        st = check(eng, ix, model)
        assert st["entries"] == 600 and st["rehashes"] == before["rehashes"] + 1 and st["slots"] > before["slots"]
        assert find(ix, keys[[0, 150]]).tolist() == [0, 1150]


def test_compaction_keeps_the_table_small(eng):
    rng = np.random.default_rng(22)
    keys = np.unique(rng.integers(0, 1 << 64, 6100, dtype=np.uint64))[:6000].reshape(10, 600)
    with eng.object_index() as ix, eng.object_index() as fresh:
        model = ic.Model()
        for c in range(10):
            put(ix, model, keys[c], np.arange(600) + c)
            drop(ix, model, keys[c])
        st = check(eng, ix, model)                               # the live set is empty: so is `fresh`
        assert st["entries"] == 0 and st["rehashes"] >= 2
        assert st["slots"] <= 2 * fresh.stats()["slots"]
        assert (find(ix, keys.reshape(-1)) == ic.NONE).all()


# ---- refusals ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [1 << 31, ic.NONE])
def test_bad_id_refuses_the_whole_batch(eng, bad):
    rng = np.random.default_rng(23)
    keys = np.unique(rng.integers(0, 1 << 64, 400, dtype=np.uint64))[:350]
    with eng.object_index() as ix:
        model = ic.Model()
        put(ix, model, keys[:50], np.arange(50))
        ids = np.arange(300, dtype=np.uint32)
        ids[150] = bad
        k, i = DevInput(keys[50:], np.uint64(0)), DevInput(ids, np.uint32(0))
        rc = eng.L.sd_cas_index_insert_dev(eng.h, ix.handle, k.ptr, i.ptr, 300,
                                           int(torch.cuda.current_stream().cuda_stream))
        assert rc == EINVAL and b"2^31" in eng.L.sd_cas_last_error(eng.h)
        check_all(k, i)
        check(eng, ix, model)                                    # unchanged: nothing was inserted
        hk, hi = np.ascontiguousarray(keys[50:]), np.ascontiguousarray(ids)
        assert eng.L.sd_cas_index_insert(eng.h, ix.handle, hk.ctypes.data, hi.ctypes.data, 300) == EINVAL
        assert (find(ix, keys[50:]) == ic.NONE).all()
        check(eng, ix, model)
        with pytest.raises(ValueError):
            ix.insert(hk, hi.astype(np.int64))                   # the Python host form checks first


def test_handle_errors():
    """An unknown or destroyed handle is SD_CAS_EINVAL in every call, and so is the 65th create."""
    from spacedrive_amd import CasEngine, CasError
    from spacedrive_amd.cas import INDEX_MAX
    e = CasEngine(0)
    try:
        L, s = e.L, e.stream
        buf = DevFence(np.uint64, 64)                            # no refused call touches it
        p = buf.ptr
        out8, n64 = np.zeros(8, np.uint64), ctypes.c_uint64(0)
        ix = e.object_index()
        dead = ix.handle
        ix.close()
        for h in (dead, 5, INDEX_MAX, 0xFFFFFFFF):
            assert L.sd_cas_index_stats(e.h, h, out8.ctypes.data) == EINVAL
            assert L.sd_cas_index_clear(e.h, h, s) == EINVAL
            assert L.sd_cas_index_destroy(e.h, h) == EINVAL
            assert L.sd_cas_index_insert_dev(e.h, h, p, p, 4, s) == EINVAL
            assert L.sd_cas_index_insert(e.h, h, out8.ctypes.data, out8.ctypes.data, 2) == EINVAL
            assert L.sd_cas_index_lookup_dev(e.h, h, p, 4, p, s) == EINVAL
            assert L.sd_cas_index_lookup(e.h, h, out8.ctypes.data, 2, out8.ctypes.data) == EINVAL
            assert L.sd_cas_index_erase_dev(e.h, h, p, 4, s) == EINVAL
            assert L.sd_cas_index_erase(e.h, h, out8.ctypes.data, 2) == EINVAL
            assert L.sd_cas_index_export_dev(e.h, h, p, p, 4, ctypes.byref(n64), s) == EINVAL
            assert L.sd_cas_identifier_links_indexed_dev(e.h, p, None, 4, 100, h, None, p, p, p,
                                                         out8.ctypes.data, 4, ctypes.byref(n64), s) == EINVAL
            assert L.sd_cas_identifier_links_indexed(e.h, out8.ctypes.data, None, 4, 100, h, None,
                                                     out8.ctypes.data, out8.ctypes.data, out8.ctypes.data,
                                                     out8.ctypes.data, 4, ctypes.byref(n64)) == EINVAL
        with pytest.raises(ValueError):
            ix.stats()                                           # closed on the Python side
        many = [e.object_index() for _ in range(INDEX_MAX)]
        assert sorted(m.handle for m in many) == list(range(INDEX_MAX))
        with pytest.raises(CasError):
            e.object_index()
        many[17].close()
        again = e.object_index()                                 # a destroyed handle's place is free again
        assert again.handle == 17 and len(again) == 0
        many[3].insert(np.array([9], np.uint64), [4])
        assert len(many[3]) == 1 and len(many[4]) == 0           # indexes do not share anything
        model = ic.Model()
        model.insert([9], [4])
        check(e, many[3], model)
        check(e, many[4], ic.Model())
        check(e, again, ic.Model())
        check_all(buf)
        assert (buf.host().view(np.uint8) == 0xC3).all()
    finally:
        e.close()                                                # destroys the rest


def test_empty_calls_clear_and_small_export(eng):
    with eng.object_index() as ix:
        model = ic.Model()
        empty64, empty32 = dev64([]), dev32([])
        ix.insert(empty64, empty32)
        assert ix.lookup(empty64).numel() == 0
        ix.erase(empty64)
        ix.insert(np.zeros(0, np.uint64), [])
        assert len(ix.lookup(np.zeros(0, np.uint64))) == 0
        ix.erase(np.zeros(0, np.uint64))
        assert exported(eng, ix, 0)[:2] == (0, 0)
        check(eng, ix, model)
        keys = ic.keys_with_home(3, log2_slots(ix), 20)
        put(ix, model, keys, np.arange(20))
        assert ix.stats()["last_max_probe"] >= 20
        ix.lookup(empty64)
        assert ix.stats()["last_max_probe"] == 0                 # the last call had n == 0
        # export into too little room: refused, the count reported, nothing written
        rc, n, k, o = exported(eng, ix, 19)
        assert rc == EINVAL and n == 20
        assert (k.view(np.uint8) == 0xC3).all() and (o.view(np.uint8) == 0xC3).all()
        # the host forms
        hk = np.array([keys[3], 12345, keys[7]], np.uint64)
        assert ix.lookup(hk).tolist() == [3, ic.NONE, 7]
        ix.erase(hk[:1])
        model.erase(hk[:1])
        ix.insert(hk[1:2], [77])
        model.insert(hk[1:2], [77])
        check(eng, ix, model)
        slots = ix.stats()["slots"]
        ix.clear()
        model.clear()
        st = check(eng, ix, model)
        assert st == dict(entries=0, slots=slots, tombstones=0, rehashes=0, last_max_probe=0)
        assert (find(ix, keys) == ic.NONE).all()
        put(ix, model, keys[:5], [9, 8, 7, 6, 5])                # and it works on
        check(eng, ix, model)


def test_calls_on_two_streams_see_each_other(eng):
    """insert on one stream, erase on another, lookup on the first, none of them synchronised by
    the caller: the library orders the calls on an index."""
    rng = np.random.default_rng(24)
    n = 30_000
    keys = np.unique(rng.integers(0, 1 << 64, n + 500, dtype=np.uint64))[:n]
    ids = rng.integers(0, 1 << 31, n, dtype=np.uint32)
    dk, di = DevInput(keys, np.uint64(0)), DevInput(ids, np.uint32(1 << 31))
    half = DevInput(keys[::2], np.uint64(0))
    out1, out2 = DevFence(np.uint32, n), DevFence(np.uint32, n)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()                                     # the caller's buffers are complete
    with eng.object_index(n) as ix:
        ix.insert(dk.t, di.t, stream=s1.cuda_stream)
        ix.lookup(dk.t, out=out1.t, stream=s2.cuda_stream)
        ix.erase(half.t, stream=s1.cuda_stream)
        ix.lookup(dk.t, out=out2.t, stream=s2.cuda_stream)
        s2.synchronize()
        s1.synchronize()
        assert (out1.host() == ids).all()
        want = ids.copy()
        want[::2] = ic.NONE
        assert (out2.host() == want).all()
        check_all(dk, di, half, out1, out2)
        model = ic.Model()
        model.insert(keys[1::2], ids[1::2])
        check(eng, ix, model)


@pytest.mark.parametrize("percent", [30, 70])
def test_another_maximum_load_changes_sizes_only(monkeypatch, percent):
    """SD_CAS_INDEX_LOAD_PERCENT, read when the context is created: the table sizes follow it
    (live keys + tombstones never pass that share of the slots), every result is the model's."""
    from spacedrive_amd import CasEngine
    monkeypatch.setenv("SD_CAS_INDEX_LOAD_PERCENT", str(percent))
    e = CasEngine(0)
    monkeypatch.delenv("SD_CAS_INDEX_LOAD_PERCENT")               # read once: later calls do not look
    try:
        with e.object_index(3000) as sized:                      # 3,000 keys under 30 % / 70 %
            assert sized.stats()["slots"] == {30: 16384, 70: 8192}[percent]
        rng = np.random.default_rng(26 + percent)
        keys = rng.permutation(np.unique(rng.integers(0, 1 << 64, 5200, dtype=np.uint64))[:5000])
        ids = rng.integers(0, 1 << 31, 5000, dtype=np.uint32)
        with e.object_index() as ix:
            model = ic.Model()
            at = k = 0
            while at < 5000:
                n = min(BATCHES[k % len(BATCHES)], 5000 - at)
                put(ix, model, keys[at:at + n], ids[at:at + n])
                st = ix.stats()
                assert 100 * (st["entries"] + st["tombstones"]) <= percent * st["slots"]
                if k % 3 == 2:
                    drop(ix, model, keys[at:at + n:2])
                at, k = at + n, k + 1
            st = check(e, ix, model)
            assert st["rehashes"] >= 3 and st["slots"] >= {30: 16384, 70: 4096}[percent]
            assert (find(ix, keys) == model.lookup(keys)).all()
        jk, js, jp, sk, so = random_job(4097, 7, 31 + percent)
        links_equal(e, jk, js, jp, sk, so, 7, f"random job at {percent} %")
    finally:
        e.close()


# ---- the link emission over an index ----------------------------------------------------------

def case_of(case_id):
    """A tests/links_cases.py case without its CPU reference (shared with the tests that built it)."""
    if case_id in lc._built:
        return lc._built[case_id][0]
    fn, args, kw, _ = lc.CASES[case_id]
    return fn(*args, **kw)


def random_job(n, chunk, seed):
    """Rows in all three states, some owning an Object, over a small key pool; seed pairs that
    repeat keys (so the minimum matters) and include keys no row has."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 64, max(2, n // 3) + 8, dtype=np.uint64))
    keys = pool[rng.integers(0, len(pool), n)]
    states = lc._states(rng, n, chunk, 0.1)
    ids = rng.permutation(max(8 * n, 4096)).astype(np.uint32)
    pre = np.where(rng.random(n) < 0.1, ids[:n], ic.NONE).astype(np.uint32)
    held = pool[rng.random(len(pool)) < 0.3]
    absent = rng.integers(0, 1 << 64, 50, dtype=np.uint64)
    sk = np.concatenate([held, held, absent, held[: len(held) // 2]])
    so = ids[n:n + len(sk)] if len(ids) >= n + len(sk) else rng.integers(0, 1 << 31, len(sk), dtype=np.uint32)
    return keys, states, pre, sk, u32(so)


def same(a, b, what):
    for name, x, y in zip(("step", "object", "action", "counts"), a, b):
        x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        if x.size == 0:
            continue
        x, y = x.astype(np.int64) & 0xFFFFFFFF, y.astype(np.int64) & 0xFFFFFFFF   # int32 tensors, u32 arrays
        bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), bad[:8].tolist())


def links_equal(eng, keys, states, pre, sk, so, chunk, what, host=False):
    """links_indexed == identifier_links with existing = export(index) == with the pairs the
    index was filled from, in every output and count; outputs of the indexed call fenced."""
    n = len(keys)
    with eng.object_index() as ix:
        model = ic.Model()
        half = len(sk) // 2
        put(ix, model, sk[:half], so[:half])                      # filled in two calls, as Objects
        put(ix, model, sk[half:], so[half:])                      # are created over time
        check(eng, ix, model)
        ek, eo = ix.export()
        dk, ds, dp = dev64(keys), torch.from_numpy(np.array(states)).cuda(), dev32(pre)
        fs, fo, fa = DevFence(np.uint32, n), DevFence(np.uint32, n), DevFence(np.uint8, n)
        got = eng.identifier_links(dk, ds, chunk, index=ix, pre_objects=dp, out=(fs.t, fo.t, fa.t))
        check_all(fs, fo, fa)
        want = eng.identifier_links(dk, ds, chunk, existing=(ek, eo), pre_objects=dp)
        same(got, want, what)
        same(got, eng.identifier_links(dk, ds, chunk, existing=(dev64(sk), dev32(so)), pre_objects=dp), what)
        if host:
            hgot = eng.identifier_links_host(keys, states, chunk, index=ix, pre_objects=pre)
            same(hgot, want, what + " (host)")
            hwant = eng.identifier_links_host(keys, states, chunk, pre_objects=pre,
                                              existing=(ek.cpu().numpy().view(np.uint64),
                                                        eo.cpu().numpy().view(np.uint32)))
            same(hgot, hwant, what + " (host forms)")
        check(eng, ix, model)                                     # the index was only read


@pytest.mark.parametrize("case_id", list(lc.CASES))
def test_links_indexed_equals_seeded_on_the_edge_cases(eng, case_id):
    keys, states, pre, seeds, chunk, _ = case_of(case_id)
    sk = np.array([k for k, _ in seeds], np.uint64)
    so = np.array([o for _, o in seeds], np.uint32)
    links_equal(eng, keys, states, pre, sk, so, chunk, case_id, host=case_id in lc.HOST_CASES)


@pytest.mark.parametrize("chunk", [1, 7, 100])
@pytest.mark.parametrize("n", [1, 99, 100, 101, 4097, 40_000])
def test_links_indexed_equals_seeded_on_random_jobs(eng, n, chunk):
    keys, states, pre, sk, so = random_job(n, chunk, 9000 + 10 * n + chunk)
    links_equal(eng, keys, states, pre, sk, so, chunk, f"random n={n} chunk={chunk}", host=True)


@pytest.mark.parametrize("with_state", [False, True])
def test_empty_index_is_the_fresh_library_call(eng, with_state):
    keys, states, _, _, _ = random_job(4097, 100, 77)
    dk = dev64(keys)
    ds = torch.from_numpy(states).cuda() if with_state else None
    n = len(keys)
    with eng.object_index() as ix:
        fs, fo, fa = DevFence(np.uint32, n), DevFence(np.uint32, n), DevFence(np.uint8, n)
        got = eng.identifier_links(dk, ds, 100, index=ix, out=(fs.t, fo.t, fa.t))
        check_all(fs, fo, fa)
        same(got, eng.identifier_links(dk, ds, 100), "empty index")
        check(eng, ix, ic.Model())
        hs = states if with_state else None
        same(eng.identifier_links_host(keys, hs, 100, index=ix), eng.identifier_links_host(keys, hs, 100),
             "empty index (host)")
        with pytest.raises(ValueError):
            eng.identifier_links(dk, ds, 100, index=ix, existing=(dk, dev32(np.arange(4097))))
        check(eng, ix, ic.Model())                                # read only, and still empty


def test_python_index_and_job_step_on_real_files(eng, tmp_path):
    """ObjectIndex through numpy arrays and cas_id strings' keys, and identifier_job_step(index=)
    against identifier_job_step(existing=) on a handful of files."""
    from spacedrive_amd import cas_id_to_key, identifier_job_step
    rng = np.random.default_rng(25)
    blobs = [b"", rng.bytes(10), rng.bytes(5000), rng.bytes(150_000), rng.bytes(300_000)]
    contents = [blobs[1], blobs[2], blobs[0], blobs[3], blobs[2], blobs[4], blobs[1], blobs[3]]
    paths = []
    for j, c in enumerate(contents):
        p = tmp_path / f"f{j}.bin"
        p.write_bytes(c)
        paths.append(str(p))
    paths.insert(4, str(tmp_path / "missing.bin"))
    fresh = identifier_job_step(paths, chunk=3, eng=eng)
    cas = {i: m.cas_id for i, m in fresh.metadata.items() if m.cas_id}
    held = [cas[1], cas[3], cas[1], "00000000deadbeef"]          # two Objects carry f1's cas_id
    ids = [40, 12, 31, 5]
    with eng.object_index() as ix:
        model = ic.Model()
        held_keys = np.array([cas_id_to_key(c) for c in held], np.uint64)
        ix.insert(held_keys, ids)
        model.insert(held_keys, ids)
        assert len(ix) == 3
        check(eng, ix, model)
        assert ix.lookup([cas_id_to_key(cas[1]), cas_id_to_key(cas[0])]).tolist() == [31, ic.NONE]
        a = identifier_job_step(paths, chunk=3, eng=eng, index=ix)
        b = identifier_job_step(paths, chunk=3, eng=eng, existing=(held, ids))
        assert a == b
        assert a.existing_of and set(a.existing_of.values()) == {31, 12}
        assert a != fresh
        check(eng, ix, model)                                    # the job steps only read it
        ix.erase([cas_id_to_key(cas[1])])                        # re-identified: the DB's remaining pair
        ix.insert([cas_id_to_key(cas[1])], [40])
        model.erase([cas_id_to_key(cas[1])])
        model.insert([cas_id_to_key(cas[1])], [40])
        check(eng, ix, model)
        c = identifier_job_step(paths, chunk=3, eng=eng, index=ix)
        assert set(c.existing_of.values()) == {40, 12}
        with pytest.raises(ValueError):
            identifier_job_step(paths, eng=eng, index=ix, existing=(held, ids))
