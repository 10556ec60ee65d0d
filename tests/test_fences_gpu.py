"""Every caller buffer of the ABI between guards (MI355X): the outputs of each entry point are
allocated at exactly their documented extent with a patterned guard before and after
(tests/fence.py), the const inputs sit between guards that hold adversarial values, and every
case asserts three things — the outputs equal the reference the suite already uses (the
oracle, numpy, the job replay, tests/exchange_ref.py), no guard byte changed, and the inputs
are bit for bit what they were.  The shapes are the smallest at which the tail code of each
kernel runs: 1, a tile - 1, a tile + 1, the threshold between two kernels.

Each case takes a fresh context and closes it, so on the debug library (whose allocations have
no 1 MiB floor and end in a checked tail) every layout used here ends exactly at
a tail: tests/conftest.py fails the case if a tail changed."""
import ctypes
import os
import time

import numpy as np
import pytest

from oracle.pyoracle import MINIMUM_FILE_SIZE, SAMPLED_CONTENT_LEN
from spacedrive_amd import CasEngine
from spacedrive_amd.cas import MAX_PACKED_CONTENT_LEN, NO_OBJECT
from spacedrive_amd.shard import range_start
from tests.exchange_ref import pack_fixed_ref, range_part, split_fixed_ref, unpack_fixed_ref
from tests.fence import DevFence, DevInput, HostFence, HostInput, check_all
from tests.golden.make_golden import replay_identifier_job
from tests.test_object_stats_cpu import STAT_NAMES, np_group, np_stats, np_top

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U8, U32, U64, I32 = np.uint8, np.uint32, np.uint64, np.int32
L = SAMPLED_CONTENT_LEN
FILL64 = 0xC3C3C3C3C3C3C3C3  # a u64 of the fences' payload prefill (0xC3)


@pytest.fixture
def feng():
    """A context of this case's own, closed when the case ends."""
    assert torch.cuda.is_available(), "GPU tests need a gfx950 device"
    e = CasEngine(0)
    yield e
    e.close()


def _s() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def ok(eng, rc, what):
    eng._check(rc, what)


def dup_keys(rng, n):
    pool = rng.integers(0, 2 ** 64, max(1, n * 7 // 10), dtype=U64)
    return pool[rng.integers(0, len(pool), n)]


def key_input(keys):
    """keys between guards of a key that occurs in them: a tail read would join its group"""
    return DevInput(keys, guard=keys[len(keys) // 2])


def up16(x):
    return (x + 15) // 16 * 16


def test_context_cost_is_small():
    """What a fresh context per case costs (printed into the log; a context is three streams, a
    dozen events and three small allocations).  The bound is generous: a case may afford it."""
    assert torch.cuda.is_available()
    CasEngine(0).close()
    t0 = time.perf_counter()
    for _ in range(10):
        CasEngine(0).close()
    per = (time.perf_counter() - t0) / 10
    print(f"context create + destroy: {per * 1e3:.2f} ms")
    assert per < 0.25


# ---- sort -------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_vals", [False, True])
@pytest.mark.parametrize("bits", [(0, 64), (56, 64), (3, 23)])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 16383, 16385])
def test_sort_pairs(feng, n, bits, with_vals):
    """8, 1 and 3 passes: the ping-pong ends in the caller's arrays after an even and an odd
    number of passes."""
    rng = np.random.default_rng(1000 + n + bits[0])
    k = rng.integers(0, 2 ** 64, n, dtype=U64)
    k[: n // 3] = k[n // 2]
    v = rng.permutation(n).astype(U32)
    kin, vin = key_input(k), DevInput(v, guard=0) if with_vals else None
    ko, vo = DevFence(U64, n), DevFence(U32, n)
    feng.sort_pairs(kin.t, vin.t if with_vals else None, ko.t, vo.t, *bits)
    torch.cuda.synchronize()
    mask = U64((1 << (bits[1] - bits[0])) - 1)
    order = np.argsort((k >> U64(bits[0])) & mask, kind="stable")
    assert (ko.host() == k[order]).all()
    assert (vo.host() == (v[order] if with_vals else order.astype(U32))).all()
    check_all(kin, vin, ko, vo)


# ---- grouping ---------------------------------------------------------------------------------

GROUP_CASES = ([("auto", 0, n) for n in (1, 4095, 4097, 1_441_792, 1_441_793)] +
               [("sort", 0, n) for n in (1, 4095, 4097, 16385)] +
               [("hash", 16, 4097), ("hash", 16, 300_001)])
METHOD = {"auto": 0, "hash": 1, "sort": 2}


@pytest.mark.parametrize("method,target,n", GROUP_CASES)
def test_group_family(feng, oracle, method, target, n):
    """group, group_min with caller values and sort_pairs + group_sorted: the small region
    chain, the last small and the first big-region shape, forced SORT, and the classical
    two-level hash chain (bucket target 16)."""
    rng = np.random.default_rng(2000 + n + target)
    keys = dup_keys(rng, n)
    orep, oobj = oracle.group_canonical(keys)
    feng.set_group_method(METHOD[method], target)
    kin = key_input(keys)
    rep = DevFence(U32, n)
    assert feng.group(kin.t, rep.t) == oobj
    assert (rep.host() == orep).all()
    check_all(kin, rep)
    # group_min: a guard value of 0 would lower a minimum it joined
    vals = rng.integers(1, 2 ** 32, n, dtype=U64).astype(U32)
    vin = DevInput(vals, guard=0)
    out = DevFence(U32, n)
    objects = feng.group_min(kin.t, vin.t, out.t)
    uniq, inv = np.unique(keys, return_inverse=True)
    mins = np.full(len(uniq), 0xFFFFFFFF, dtype=U32)
    np.minimum.at(mins, inv.reshape(-1), vals)
    assert objects == len(uniq) == oobj
    assert (out.host() == mins[inv.reshape(-1)]).all()
    check_all(kin, vin, out)
    # group_sorted over the stably sorted pairs
    order = np.argsort(keys, kind="stable")
    sk = DevInput(keys[order], guard=keys[order][-1])
    sv = DevInput(order.astype(U32), guard=0)
    rep2 = DevFence(U32, n)
    assert feng.group_sorted(sk.t, sv.t, rep2.t) == oobj
    assert (rep2.host() == orep).all()
    check_all(sk, sv, rep2)


def test_copy_objects_one_word(feng, oracle):
    rng = np.random.default_rng(2100)
    keys = dup_keys(rng, 5000)
    _, oobj = oracle.group_canonical(keys)
    kin, rep = key_input(keys), DevFence(U32, 5000)
    feng.group(kin.t, rep.t, want_objects=False)
    word = DevFence(U64, 1)
    ok(feng, feng.L.sd_cas_copy_objects_dev(feng.h, word.ptr, _s()), "copy_objects")
    torch.cuda.synchronize()
    assert int(word.host()[0]) == oobj
    check_all(kin, rep, word)


@pytest.mark.parametrize("chunk_kind", ["1", "100", "n+5"])
@pytest.mark.parametrize("n", [1, 8191, 8193])
def test_group_chunked(feng, oracle, n, chunk_kind):
    chunk = {"1": 1, "100": 100, "n+5": n + 5}[chunk_kind]
    rng = np.random.default_rng(2200 + n)
    keys = dup_keys(rng, n)
    orep, _ = oracle.group_canonical(keys)
    crep, cc, cl = oracle.group_chunked(keys, chunk)
    rin = DevInput(orep, guard=0)
    out = DevFence(U32, n)
    assert feng.group_chunked(rin.t, out.t, chunk) == (cc, cl)
    assert (out.host() == crep).all()
    check_all(rin, out)


# ---- exchange ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 4095, 4097])
@pytest.mark.parametrize("parts", [1, 3, 1024, 1025])
def test_partition(feng, parts, n):
    """d_counts is exactly `parts` words."""
    rng = np.random.default_rng(3000 + parts + n)
    keys = rng.integers(0, 2 ** 64, n, dtype=U64)
    kin = key_input(keys)
    ko, po, counts = DevFence(U64, n), DevFence(U32, n), DevFence(U64, parts)
    feng.partition(kin.t, parts, ko.t, po.t, counts.t)
    torch.cuda.synchronize()
    want_part = range_part(keys, parts)
    want_counts = np.bincount(want_part, minlength=parts)
    assert (counts.host() == want_counts.astype(U64)).all()
    k, p = ko.host(), po.host().astype(np.int64)
    assert (np.bincount(p, minlength=n) == 1).all() and len(p) == n
    assert (keys[p] == k).all()
    assert (range_part(k, parts) == np.repeat(np.arange(parts), want_counts)).all()
    check_all(kin, ko, po, counts)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_exchange_pack_split_unpack(feng, n):
    rng = np.random.default_rng(3100 + n)
    keys = rng.integers(0, 2 ** 64, n, dtype=U64)
    pos = rng.permutation(n).astype(U32)
    file0 = 123_456
    kin, pin = key_input(keys), DevInput(pos, guard=0)
    rows = DevFence(U32, 3 * n)
    feng.exchange_pack(kin.t, pin.t, file0, rows.t)
    torch.cuda.synchronize()
    want = np.stack([(keys & U64(0xFFFFFFFF)).astype(U32), (keys >> U64(32)).astype(U32),
                     pos + U32(file0)], axis=1).reshape(-1)
    assert (rows.host() == want).all()
    check_all(kin, pin, rows)
    rin = DevInput(want, guard=0)
    k2, v2 = DevFence(U64, n), DevFence(U32, n)
    feng.exchange_split(rin.t, k2.t, v2.t)
    torch.cuda.synchronize()
    assert (k2.host() == keys).all() and (v2.host() == pos + U32(file0)).all()
    check_all(rin, k2, v2)
    back = rng.integers(0, 2 ** 32, n, dtype=U64).astype(U32)
    bin_ = DevInput(back, guard=0)
    rep = DevFence(U64, n)
    feng.exchange_unpack(bin_.t, pin.t, rep.t)
    torch.cuda.synchronize()
    wrep = np.zeros(n, dtype=U64)
    wrep[pos] = back
    assert (rep.host() == wrep).all()
    check_all(bin_, pin, rep)


@pytest.mark.parametrize("G", [3, 1024])
def test_exchange_pack_unpack_fixed(feng, G):
    """cap 37 and spill 5 (off the multiples of 64), part sizes cycling through 0..cap + spill
    (G = 3: an empty, a full and a spilling part): rows, spill rows and the one overflow word
    each between guards, and the mirror's rep."""
    cap, spill, file0 = 37, 5, 1_000_000
    rng = np.random.default_rng(3200 + G)
    counts = [0, cap + spill, cap + 1] if G == 3 else [(5 * i) % (cap + spill + 1) for i in range(G)]
    n = sum(counts)
    keys = rng.integers(1, 2 ** 64, n, dtype=U64)
    pos = rng.permutation(n).astype(U32)
    kin, pin = key_input(keys), DevInput(pos, guard=0)
    cin = DevInput(np.array(counts, dtype=U64), guard=1 << 40)
    rows, srows = DevFence(U32, G * cap * 3), DevFence(U32, G * spill * 3)
    flag = DevFence(U32, 1, fill=0)
    ok(feng, feng.L.sd_cas_exchange_pack_fixed_dev(feng.h, kin.ptr, pin.ptr, cin.ptr, G, cap, spill, file0,
                                                   rows.ptr, srows.ptr, flag.ptr, _s()), "pack_fixed")
    torch.cuda.synchronize()
    wrows, wsrows, wflag = pack_fixed_ref(keys, pos, counts, G, cap, spill, file0)
    assert wflag == 0
    assert (rows.host().reshape(-1, 3) == wrows).all()
    assert (srows.host().reshape(-1, 3) == wsrows).all()
    assert int(flag.host()[0]) == 0
    check_all(kin, pin, cin, rows, srows, flag)
    back = rng.integers(0, 2 ** 32, G * cap, dtype=U64).astype(U32)
    sback = rng.integers(0, 2 ** 32, G * spill, dtype=U64).astype(U32)
    bin_, sbin = DevInput(back, guard=0), DevInput(sback, guard=0)
    rep = DevFence(U64, n)
    ok(feng, feng.L.sd_cas_exchange_unpack_fixed_dev(feng.h, bin_.ptr, sbin.ptr, pin.ptr, cin.ptr, G, cap, spill,
                                                     rep.ptr, _s()), "unpack_fixed")
    torch.cuda.synchronize()
    wrep, defined = unpack_fixed_ref(back, sback, pos, counts, G, cap, spill)
    assert defined.all()
    assert (rep.host() == wrep.astype(U64)).all()
    check_all(bin_, sbin, pin, cin, rep)


@pytest.mark.parametrize("m", [1, 2047, 2049])
def test_exchange_split_fixed(feng, m):
    """Around the kernel's 2,048-row block, a third of the rows sentinels; the sentinel-row
    counter is one fenced u64."""
    rng = np.random.default_rng(3300 + m)
    sentinel = range_start(3, 7)
    k = rng.integers(1, 2 ** 64, m, dtype=U64)
    k[k == U64(sentinel)] = U64(1)
    k[rng.random(m) < 0.33] = U64(sentinel)
    k[m - 1] = U64(sentinel)
    rows = np.empty((m, 3), dtype=U32)
    rows[:, 0], rows[:, 1] = k & U64(0xFFFFFFFF), k >> U64(32)
    rows[:, 2] = rng.integers(0, 2 ** 32, m, dtype=U64)
    rin = DevInput(rows.reshape(-1), guard=0)
    ko, vo = DevFence(U64, m), DevFence(U32, m)
    nsent = DevFence(U64, 1, fill=0)
    ok(feng, feng.L.sd_cas_exchange_split_fixed_dev(feng.h, rin.ptr, m, sentinel, ko.ptr, vo.ptr, nsent.ptr, _s()),
       "split_fixed")
    torch.cuda.synchronize()
    wk, wv, wn = split_fixed_ref(rows, sentinel)
    assert int(nsent.host()[0]) == wn >= 1
    assert (ko.host() == wk).all() and (vo.host() == wv).all()
    check_all(rin, ko, vo, nsent)


def test_multi_group_three_shards(oracle):
    """sd_cas_multi_group on one device, 3 shards: each d_rep[i] between guards."""
    from spacedrive_amd.multi import MultiEngine
    rng = np.random.default_rng(3400)
    pool = rng.integers(0, 2 ** 64, 6000, dtype=U64)
    shard_keys = [pool[rng.integers(0, len(pool), n)] for n in (4097, 1, 2047)]
    kins = [key_input(k) for k in shard_keys]
    reps = [DevFence(U64, len(k)) for k in shard_keys]
    file0 = [0, 4097, 4098]
    me = MultiEngine([0, 0, 0])
    try:
        torch.cuda.synchronize()
        kp = (ctypes.c_void_p * 3)(*[k.ptr for k in kins])
        rp = (ctypes.c_void_p * 3)(*[r.ptr for r in reps])
        ns = (ctypes.c_size_t * 3)(*[len(k) for k in shard_keys])
        f0 = (ctypes.c_uint64 * 3)(*file0)
        obj = HostFence(U64, 1)
        me._check(me.L.sd_cas_multi_group(me.h, kp, ns, f0, rp, obj.ptr), "multi_group")
    finally:
        me.close()
    orep, oobj = oracle.group_canonical(np.concatenate(shard_keys))
    assert int(obj.a[0]) == oobj
    assert (np.concatenate([r.host() for r in reps]) == orep.astype(U64)).all()
    check_all(*kins, *reps, obj)


# ---- link emission ----------------------------------------------------------------------------

def links_case(rng, n, chunk):
    keys = dup_keys(rng, n)
    states = rng.choice(np.array([0, 1, 2], dtype=U8), n, p=[0.9, 0.05, 0.05])
    last = np.arange(chunk - 1, n, chunk)
    if chunk > 1:
        states[last[rng.random(len(last)) < 0.3]] = 2
        states[last[rng.random(len(last)) < 0.2]] = 1
    else:  # every row ends its chunk: rows that stay orphan only at the end (the step budget)
        states[:] = 0
        states[-3:] = [1, 0, 2][-min(n, 3):]
    return keys, states


def run_links(eng, symbol, keys, states, chunk, seeds=None, pre=None, extra_steps=0):
    """One raw-ABI call of a device form: d_step / d_object / d_action between guards,
    h_step_counts a fenced host array of exactly 2 * max_steps words with out_steps beside
    it.  Returns (step, object, action, counts words, steps) after checking every fence."""
    n = len(keys)
    kin = key_input(keys)
    sin = DevInput(states, guard=0) if states is not None else None  # 0 = HASHED
    ms = int(eng.L.sd_cas_identifier_max_steps(n, chunk)) + extra_steps
    step, obj, act = DevFence(U32, n), DevFence(U32, n), DevFence(U8, n)
    counts, steps = HostFence(U64, 2 * ms), HostFence(U64, 1)
    ins = [kin, sin]
    args = [eng.h, kin.ptr, sin.ptr if sin else None, n, chunk]
    if symbol != "sd_cas_identifier_links_dev":
        sk, so = seeds if seeds is not None else (np.zeros(0, U64), np.zeros(0, U32))
        skin = DevInput(sk, guard=keys[0]) if len(sk) else None
        soin = DevInput(so, guard=0) if len(sk) else None  # 0 = the smallest Object
        ins += [skin, soin]
        args += [skin.ptr if skin else None, soin.ptr if soin else None, len(sk)]
    if symbol == "sd_cas_identifier_links_ex_dev":
        prein = DevInput(pre, guard=0) if pre is not None else None
        ins.append(prein)
        args.append(prein.ptr if prein else None)
    args += [step.ptr, obj.ptr, act.ptr, counts.ptr, ms, steps.ptr, _s()]
    ok(eng, getattr(eng.L, symbol)(*args), symbol)
    torch.cuda.synchronize()
    check_all(*ins, step, obj, act, counts, steps)
    return step.host(), obj.host(), act.host(), counts.a.copy(), int(steps.a[0])


def assert_links(got, want, total_steps):
    step, obj, act, words, steps = got
    want_step, want_obj, want_act, want_counts = want
    assert steps == len(want_counts) <= total_steps
    assert [tuple(c) for c in words[:2 * steps].reshape(-1, 2).tolist()] == want_counts
    assert (words[2 * steps:2 * total_steps] == 0).all()  # the steps the job did not run
    assert (step == np.array(want_step, dtype=U32)).all()
    assert (obj == np.array(want_obj, dtype=U32)).all()
    assert (act == np.array(want_act, dtype=U8)).all()


@pytest.mark.parametrize("chunk", [1, 7, 100])
@pytest.mark.parametrize("n", [1, 255, 257, 16383, 16385])
def test_identifier_links_dev_forms(n, chunk):
    """sd_cas_identifier_links_dev, _seeded_dev and _ex_dev against the job replay, a fresh
    context each.  At n = 16,385 the rows owning an Object are chosen so that the events (hashed
    rows holding one) number 2,047 and 2,049: the segmented scan's tile - 1 and + 1."""
    rng = np.random.default_rng(4000 + n + chunk)
    keys, states = links_case(rng, n, chunk)
    lk, ls = [int(k) for k in keys], [int(s) for s in states]
    total = -(-n // chunk)
    with CasEngine(0) as eng:
        assert_links(run_links(eng, "sd_cas_identifier_links_dev", keys, states, chunk),
                     replay_identifier_job(lk, ls, chunk), total)
    with CasEngine(0) as eng:  # no states: every row hashed
        assert_links(run_links(eng, "sd_cas_identifier_links_dev", keys, None, chunk),
                     replay_identifier_job(lk, [0] * n, chunk), total)
    ids = rng.permutation(4 * n + 8).astype(U32)
    sk = np.concatenate([keys[rng.random(n) < 0.2], [U64(12345)]]).astype(U64)
    so = ids[:len(sk)]
    existing = list(zip((int(k) for k in sk), (int(o) for o in so)))
    with CasEngine(0) as eng:
        assert_links(run_links(eng, "sd_cas_identifier_links_seeded_dev", keys, states, chunk, (sk, so)),
                     replay_identifier_job(lk, ls, chunk, existing=existing), total)
    hashed = np.flatnonzero(states == 0)
    for events in ([2047, 2049] if n == 16385 else [max(1, len(hashed) // 10)]):
        events = min(events, len(hashed))
        pre = np.full(n, NO_OBJECT, dtype=U32)
        own = rng.choice(hashed, events, replace=False) if events else hashed[:0]
        pre[own] = ids[len(sk):len(sk) + events]
        pre_list = [None if int(p) == NO_OBJECT else int(p) for p in pre]
        with CasEngine(0) as eng:
            assert_links(run_links(eng, "sd_cas_identifier_links_ex_dev", keys, states, chunk, (sk, so), pre),
                         replay_identifier_job(lk, ls, chunk, existing=existing, pre_objects=pre_list), total)


def test_identifier_links_step_counts_extent(feng):
    """What include/sd_hip_cas.h says of h_step_counts: the first 2 * ceil(n / chunk) words are
    written — the executed steps' pairs, zeros for the steps the job did not run — and with a
    larger max_steps the words past them are not touched."""
    rng = np.random.default_rng(4100)
    n, chunk, extra = 257, 7, 3
    keys, states = links_case(rng, n, chunk)
    got = run_links(feng, "sd_cas_identifier_links_dev", keys, states, chunk, extra_steps=extra)
    total = -(-n // chunk)
    assert_links(got, replay_identifier_job([int(k) for k in keys], [int(s) for s in states], chunk), total)
    assert len(got[3]) == 2 * (total + extra)
    assert (got[3][2 * total:] == U64(FILL64)).all()


@pytest.mark.parametrize("form", ["plain", "seeded", "ex"])
def test_identifier_links_host_forms(feng, form):
    """The host forms through the raw ABI at n = 257: every array in numpy memory between
    guards, the optional inputs given and NULL."""
    rng = np.random.default_rng(4200)
    n, chunk = 257, 7
    keys, states = links_case(rng, n, chunk)
    lk = [int(k) for k in keys]
    ids = rng.permutation(4 * n).astype(U32)
    sk = keys[rng.random(n) < 0.2].astype(U64)
    so = ids[:len(sk)]
    pre = np.where(rng.random(n) < 0.1, ids[n:2 * n], NO_OBJECT).astype(U32)
    for with_state in (True, False):
        st = states if with_state else None
        ls = [int(s) for s in states] if with_state else [0] * n
        kin = HostInput(keys, guard=keys[n // 2])
        sin = HostInput(st, guard=0) if with_state else None
        step, obj, act = HostFence(U32, n), HostFence(U32, n), HostFence(U8, n)
        ms = -(-n // chunk)
        counts, steps = HostFence(U64, 2 * ms), HostFence(U64, 1)
        args = [feng.h, kin.ptr, sin.ptr if sin else None, n, chunk]
        ins, kw = [kin, sin], {}
        if form != "plain":
            skin, soin = HostInput(sk, guard=keys[0]), HostInput(so, guard=0)
            ins += [skin, soin]
            args += [skin.ptr, soin.ptr, len(sk)]
            kw["existing"] = list(zip((int(k) for k in sk), (int(o) for o in so)))
        if form == "ex":
            pin = HostInput(pre, guard=0)
            ins.append(pin)
            args.append(pin.ptr)
            kw["pre_objects"] = [None if int(p) == NO_OBJECT else int(p) for p in pre]
        args += [step.ptr, obj.ptr, act.ptr, counts.ptr, ms, steps.ptr]
        symbol = {"plain": "sd_cas_identifier_links", "seeded": "sd_cas_identifier_links_seeded",
                  "ex": "sd_cas_identifier_links_ex"}[form]
        ok(feng, getattr(feng.L, symbol)(*args), symbol)
        check_all(*ins, step, obj, act, counts, steps)
        assert_links((step.a, obj.a, act.a, counts.a, int(steps.a[0])),
                     replay_identifier_job(lk, ls, chunk, **kw), ms)


# ---- Object statistics ------------------------------------------------------------------------

def stats_case(rng, n):
    keys = dup_keys(rng, n)
    sizes = (keys >> U64(24)) + U64(1)  # a function of the key: no size mismatch
    rep, _ = np_group(keys)
    return keys, sizes, rep


@pytest.mark.parametrize("n", [1, 255, 257, 1023, 1025, 2047, 2049])
def test_object_stats(feng, n):
    """Around the count kernel's 1,024-row and the finalize kernel's 2,048-row tile: d_copies
    has n entries, d_totals 8 words on the device, out_totals[8] on the host."""
    rng = np.random.default_rng(5000 + n)
    _, sizes, rep = stats_case(rng, n)
    wcopies, wtot = np_stats(rep, sizes)
    rin, zin = DevInput(rep, guard=0), DevInput(sizes, guard=1 << 40)
    copies, totals = DevFence(U32, n), DevFence(U64, 8)
    out = HostFence(U64, 8)
    ok(feng, feng.L.sd_cas_object_stats_dev(feng.h, rin.ptr, zin.ptr, n, copies.ptr, totals.ptr, out.ptr, _s()),
       "object_stats")
    torch.cuda.synchronize()
    assert (copies.host() == wcopies).all()
    want = [wtot[k] for k in STAT_NAMES]
    assert out.a.tolist() == want and totals.host().tolist() == want
    check_all(rin, zin, copies, totals, out)
    # the context's own totals (d_totals NULL), asynchronous
    copies2 = DevFence(U32, n)
    ok(feng, feng.L.sd_cas_object_stats_dev(feng.h, rin.ptr, zin.ptr, n, copies2.ptr, None, None, _s()),
       "object_stats")
    torch.cuda.synchronize()
    assert (copies2.host() == wcopies).all()
    check_all(rin, zin, copies2)


@pytest.mark.parametrize("k_kind", ["1", "5", "above"])
@pytest.mark.parametrize("n", [16383, 16385])
def test_top_duplicates(feng, n, k_kind):
    """Around the top list's 16,384-row compaction tile; heads and waste are exactly k entries,
    also for a k above the sets found."""
    rng = np.random.default_rng(5100 + n)
    _, sizes, rep = stats_case(rng, n)
    wcopies, wtot = np_stats(rep, sizes)
    k = {"1": 1, "5": 5, "above": wtot["duplicate_sets"] + 3}[k_kind]
    rin, zin, cin = DevInput(rep, guard=0), DevInput(sizes, guard=1 << 40), DevInput(wcopies, guard=2)
    heads, waste = DevFence(U32, k), DevFence(U64, k)
    found = HostFence(U64, 1)
    ok(feng, feng.L.sd_cas_top_duplicates_dev(feng.h, rin.ptr, zin.ptr, cin.ptr, n, k, heads.ptr, waste.ptr,
                                              found.ptr, _s()), "top_duplicates")
    torch.cuda.synchronize()
    th, tw, nf = np_top(rep, sizes, wcopies, k)
    assert int(found.a[0]) == nf == min(k, wtot["duplicate_sets"])
    assert (heads.host() == th).all() and (waste.host() == tw).all()
    check_all(rin, zin, cin, heads, waste, found)


@pytest.mark.parametrize("given", ["all", "rep", "copies", "totals", "top", "none"])
def test_duplicate_report_optional_outputs(feng, given):
    """sd_cas_duplicate_report through the raw ABI at n = 257, row states included: every
    optional output once given (between guards) and once NULL."""
    rng = np.random.default_rng(5200)
    n, k = 257, 5
    keys = dup_keys(rng, n)
    sizes = (keys >> U64(24)) + U64(1)
    states = rng.choice(np.array([0, 1, 2], dtype=U8), n, p=[0.8, 0.1, 0.1])
    hashed = states == 0
    wrep = np.full(n, NO_OBJECT, dtype=U32)
    rows = np.flatnonzero(hashed)
    wrep[rows] = rows[np_group(keys[rows])[0]]
    wcopies, wtot = np_stats(np.where(hashed, wrep, 0), sizes, hashed)
    th, tw, nf = np_top(np.where(hashed, wrep, NO_OBJECT), sizes, wcopies, k)
    kin, zin, sin = HostInput(keys, keys[n // 2]), HostInput(sizes, 1 << 40), HostInput(states, 0)
    want = lambda name: given in ("all", name)  # noqa: E731
    rep = HostFence(U32, n) if want("rep") else None
    copies = HostFence(U32, n) if want("copies") else None
    totals = HostFence(U64, 8) if want("totals") else None
    heads, waste, found = ((HostFence(U32, k), HostFence(U64, k), HostFence(U64, 1)) if want("top")
                           else (None, None, None))
    p = lambda f: f.ptr if f is not None else None  # noqa: E731
    ok(feng, feng.L.sd_cas_duplicate_report(feng.h, kin.ptr, zin.ptr, sin.ptr, n, p(rep), p(copies), p(totals), k,
                                            p(heads), p(waste), p(found)), "duplicate_report")
    if rep:
        assert (rep.a == wrep).all()
    if copies:
        assert (copies.a == wcopies).all()
    if totals:
        assert totals.a.tolist() == [wtot[q] for q in STAT_NAMES]
    if heads:
        assert int(found.a[0]) == nf and (heads.a == th).all() and (waste.a == tw).all()
    check_all(kin, zin, sin, rep, copies, totals, heads, waste, found)


# ---- cas_id strings ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 257])
def test_keys_to_hex_and_thumbnail_paths(feng, n):
    """d_out of exactly 16 n bytes; thumbnail records at the tight stride with prefixes of 0, 5
    and 37 bytes."""
    from tests.test_thumbnail import hex_table, records, roundup16
    rng = np.random.default_rng(6000 + n)
    keys = rng.integers(0, 2 ** 64, n, dtype=U64)
    hexes = hex_table(keys)
    kin = key_input(keys)
    out = DevFence(U8, 16 * n)
    feng.keys_to_hex(kin.t, out.t)
    torch.cuda.synchronize()
    assert (out.host().reshape(n, 16) == hexes).all()
    check_all(kin, out)
    for plen in (0, 5, 37):
        prefix = rng.integers(1, 256, plen, dtype=U8).tobytes()
        stride = roundup16(plen + 26)
        rec = DevFence(U8, n * stride)
        ok(feng, feng.L.sd_cas_thumbnail_paths_dev(feng.h, kin.ptr, n, prefix, stride, rec.ptr, _s()),
           "thumbnail_paths")
        torch.cuda.synchronize()
        assert (rec.host().reshape(n, stride) == records(prefix, hexes, stride)).all(), plen
        check_all(kin, rec)


def test_key_to_hex_and_shard_hex_host():
    """17 and 4 bytes, no more."""
    from spacedrive_amd import _native
    lib = _native.lib()
    for key in (0, 0x0123456789ABCDEF, 2 ** 64 - 1):
        out, shard = HostFence(U8, 17), HostFence(U8, 4)
        lib.sd_cas_key_to_hex(key, ctypes.cast(out.ptr, ctypes.c_char_p))
        lib.sd_cas_shard_hex(key, ctypes.cast(shard.ptr, ctypes.c_char_p))
        assert out.a.tobytes() == f"{key:016x}".encode() + b"\0"
        assert shard.a.tobytes() == f"{key:016x}"[:3].encode() + b"\0"
        check_all(out, shard)


# ---- hashing ----------------------------------------------------------------------------------

def sampled_inputs(rng, n, fill):
    content = rng.integers(0, 256, (n, L), dtype=U8)
    sizes = rng.integers(MINIMUM_FILE_SIZE + 1, 2 ** 40, n, dtype=U64)
    return content, sizes, DevInput(content.reshape(-1), guard=fill), DevInput(sizes, guard=1 << 40)


SAMPLED_SHAPES = ([("lane", n) for n in (1, 255, 257, 513)] +
                  [(shape, n) for shape in ("wave", "seg16") for n in (1, 3, 4, 5, 63, 65)])


@pytest.mark.parametrize("shape,n", SAMPLED_SHAPES)
def test_hash_sampled(oracle, shape, n):
    """K1 (lane path forced) and both chunk-parallel shapes at the default threshold.  The
    guards around the content hold 0xFF, then 0x00: the keys are the oracle's both times."""
    got = []
    for fill in (0xFF, 0x00):
        content, sizes, cin, zin = sampled_inputs(np.random.default_rng(7000 + n), n, fill)
        with CasEngine(0) as eng:
            if shape == "lane":
                eng.set_latency_threshold(0, 0)
            else:
                eng.set_chunkpar_split(*((1 << 40, 1 << 40) if shape == "wave" else (0, 0)))
            keys = DevFence(U64, n)
            eng.hash_sampled(cin.t, zin.t, keys.t, stride=L, n=n)
            torch.cuda.synchronize()
        check_all(cin, zin, keys)
        got.append(keys.host())
    want = oracle.fast_cas_keys_strided(content.reshape(-1), L, L, sizes, 4)
    assert (got[0] == want).all() and (got[1] == want).all()


@pytest.fixture(scope="module")
def quanta():
    """2 quanta + 77 synthetic sampled files between two guards of 0xFF (made once; the shape
    tests/test_k1_pipeline.py builds), their sizes between guards of 2^40, and snapshots."""
    from tests.fence import GUARD
    with CasEngine(0) as eng:
        q = eng.batch_quantum
        n = 2 * q + 77
        buf = torch.full((GUARD + n * L + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        zbuf = torch.full((GUARD // 8 + n + GUARD // 8,), 1 << 40, dtype=torch.int64, device="cuda")
        content = buf[GUARD:GUARD + n * L]
        sizes = zbuf[GUARD // 8:GUARD // 8 + n]
        eng.synth_sampled(0x4B32, 0, n, content, sizes, L, dup_permille=300)
        torch.cuda.synchronize()
    csum = buf.view(torch.int64).sum().item()  # the content's snapshot: its wrapping word sum
    yield q, n, buf, content, zbuf, zbuf.clone(), sizes, csum
    del buf, content
    torch.cuda.empty_cache()


def quanta_unchanged(quanta):
    q, n, buf, content, zbuf, zsnap, sizes, csum = quanta
    assert torch.equal(zbuf, zsnap), "sizes or their guards changed"
    assert buf.view(torch.int64).sum().item() == csum, "content or its guards changed"
    assert bool((buf[:64] == 0xFF).all()) and bool((buf[-64:] == 0xFF).all())


def oracle_rows(oracle, quanta, rows):
    q, n, buf, content, zbuf, zsnap, sizes, csum = quanta
    idx = torch.from_numpy(rows).cuda()
    sub = content.view(n, L)[idx].cpu().numpy()
    return oracle.fast_cas_keys_strided(sub.reshape(-1), L, L, sizes[idx].cpu().numpy().view(U64), 8)


def test_hash_sampled_two_quanta_plus(feng, oracle, quanta):
    """One default-dispatch batch of two quanta + 77 (K1 over the quanta, K1L over the rest):
    600 rows around the quantum boundaries against the oracle, every fence in full."""
    q, n, buf, content, zbuf, zsnap, sizes, csum = quanta
    keys = DevFence(U64, n)
    feng.hash_sampled(content, sizes, keys.t, stride=L, n=n)
    torch.cuda.synchronize()
    rows = np.concatenate([np.arange(0, 100), np.arange(q - 100, q + 100), np.arange(2 * q - 123, n),
                           np.arange(q // 2, q // 2 + 100)])
    assert len(rows) == 600
    assert (keys.host()[rows] == oracle_rows(oracle, quanta, rows)).all()
    assert not (keys.host() == U64(FILL64)).any()  # every key was written
    check_all(keys)
    quanta_unchanged(quanta)


@pytest.mark.parametrize("split", [False, True])
def test_hash_group_one_quantum(oracle, quanta, split):
    """The fused chain on one quantum (hash_group_sampled; hash_regions + group_regions): keys,
    rep and the overflow word between guards.  Keys against the oracle on 400 rows, rep against
    the oracle's canonical grouping of the device's keys."""
    q, n, buf, content, zbuf, zsnap, sizes, csum = quanta
    c, z = content[:q * L].view(q, L), sizes[:q]
    keys, rep, ovf = DevFence(U64, q), DevFence(U32, q), DevFence(U32, 1, fill=0)
    with CasEngine(0) as eng:
        if split:
            eng.hash_regions_sampled(c, z, keys.t, rep.t, ovf.t)
            objects = eng.group_regions(q, rep.t)
        else:
            objects = eng.hash_group_sampled(c, z, keys.t, rep.t, ovf.t)
        torch.cuda.synchronize()
    rows = np.concatenate([np.arange(0, 200), np.arange(q - 200, q)])
    got = keys.host()
    assert (got[rows] == oracle_rows(oracle, quanta, rows)).all()
    orep, oobj = oracle.group_canonical(got)
    assert objects == oobj < q and (rep.host() == orep).all()
    assert int(ovf.host()[0]) == 0
    check_all(keys, rep, ovf)
    quanta_unchanged(quanta)


def packed_case(rng, lens, fill):
    """contents back to back at 16-B aligned offsets, padding = fill, in an arena that ends at
    the last content's 16-B round-up (or 16 bytes after its start); guards of fill around it"""
    offs, o = [], 0
    for ln in lens:
        offs.append(o)
        o += max(up16(ln), 16)
    arena = np.full(o, fill, dtype=U8)
    for ln, off in zip(lens, offs):
        arena[off:off + ln] = rng.integers(0, 256, ln, dtype=U8)
    return arena, np.array(offs, dtype=U64)


PACKED_SHAPES = [("lane", n) for n in (1, 255, 257)] + [("chunkpar", n) for n in (1, 3, 5)]


@pytest.mark.parametrize("shape,n", PACKED_SHAPES)
def test_hash_packed(oracle, shape, n):
    """K2 (lane path forced) and the chunk-parallel kernel over ragged lengths, 0 and the
    maximum among them; padding and guards 0xFF then 0x00."""
    lens = ([0, MAX_PACKED_CONTENT_LEN, 1, 1016, 1017, 102400][:n] +
            [int(x) for x in np.random.default_rng(7100 + n).integers(0, 30_000, max(0, n - 6))])
    if n == 1:
        lens = [MAX_PACKED_CONTENT_LEN]
    sizes = np.array([ln if ln <= MINIMUM_FILE_SIZE else ln * 3 + 200_000 for ln in lens], dtype=U64)
    got = []
    for fill in (0xFF, 0x00):
        arena, offs = packed_case(np.random.default_rng(7200 + n), lens, fill)
        ain, oin = DevInput(arena, guard=fill), DevInput(offs, guard=0)
        lin, zin = DevInput(np.array(lens, dtype=U32), guard=MAX_PACKED_CONTENT_LEN), DevInput(sizes, guard=1 << 40)
        keys = DevFence(U64, n)
        with CasEngine(0) as eng:
            if shape == "lane":
                eng.set_latency_threshold(0, 0)
            eng.hash_packed(ain.t, oin.t, lin.t, zin.t, keys.t)
            torch.cuda.synchronize()
        check_all(ain, oin, lin, zin, keys)
        got.append(keys.host())
        want = oracle.cas_keys(arena, offs, np.array(lens, dtype=U64), sizes)
        assert (got[-1] == want).all(), fill
    assert (got[0] == got[1]).all()


# ---- checksums --------------------------------------------------------------------------------

@pytest.mark.parametrize("length", [0, 1, 1024, 1025, (1 << 20) + 1])
def test_checksum_dev(oracle, length):
    """out[32] on the host between guards; the data readable to its 16-B round-up, the
    round-up bytes and guards 0xFF then 0x00."""
    data = np.random.default_rng(8000 + length).integers(0, 256, length, dtype=U8)
    want = oracle.blake3(data.tobytes())
    for fill in (0xFF, 0x00):
        din = DevInput(data, guard=fill, slack=up16(length) - length)
        out = HostFence(U8, 32)
        with CasEngine(0) as eng:
            ok(eng, eng.L.sd_cas_checksum_dev(eng.h, din.ptr, length, out.ptr, _s()), "checksum")
        assert out.a.tobytes() == want, fill
        check_all(din, out)


def ragged_arena(eng, lens, seed):
    offs, o = [], 0
    for ln in lens:
        offs.append(o)
        o += max(up16(ln), 16)
    arena = torch.empty(o, dtype=torch.uint8, device="cuda")
    eng.synth_stream(seed, 1, 0, o, arena)
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    return host, np.array(offs, dtype=U64)


@pytest.mark.parametrize("n", [1, 3, 300, 65_537])
def test_checksums_dev(feng, oracle, n):
    """d_out is exactly 32 n bytes.  n = 65,537 buffers of 0..2 KiB take the lane path."""
    rng = np.random.default_rng(8100 + n)
    if n == 65_537:
        lens = [int(x) for x in rng.integers(0, 2049, n)]
    else:
        lens = ([(1 << 20) + 1, 0, 1025][:n] + [int(x) for x in rng.integers(0, 70_000, max(0, n - 3))])
    host, offs = ragged_arena(feng, lens, 81)
    ain, oin = DevInput(host, guard=0xFF), DevInput(offs, guard=0)
    lin = DevInput(np.array(lens, dtype=U64), guard=1 << 40)
    out = DevFence(U8, 32 * n)
    feng.checksums_dev(ain.t, oin.t, lin.t, out.t, arena_bytes=len(host))
    torch.cuda.synchronize()
    got = out.host().reshape(n, 32)
    check = range(n) if n <= 300 else rng.choice(n, 400, replace=False).tolist() + [0, n - 1]
    for i in check:
        assert got[i].tobytes() == oracle.blake3(host[int(offs[i]):int(offs[i]) + lens[i]].tobytes()), (i, lens[i])
    check_all(ain, oin, lin, out)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_hash_contents_and_identify_validate(feng, oracle, n):
    """Whole and sampled sizes mixed: keys of exactly n words, digests of exactly 32 n bytes."""
    from tests.test_inplace_gpu import want_keys
    rng = np.random.default_rng(8200 + n)
    base = [150_001, 0, 1, 102_400, 102_401, 1017]
    lens = (base + [int(x) for x in rng.integers(0, 140_000, max(0, n - len(base)))])[:n]
    host, offs = ragged_arena(feng, lens, 82)
    wkeys = want_keys(oracle, host, offs, lens)
    ain, oin = DevInput(host, guard=0xFF), DevInput(offs, guard=0)
    lin = DevInput(np.array(lens, dtype=U64), guard=1 << 40)
    keys = DevFence(U64, n)
    feng.hash_contents(ain.t, oin.t, lin.t, keys.t, arena_bytes=len(host))
    torch.cuda.synchronize()
    assert (keys.host() == wkeys).all()
    check_all(ain, oin, lin, keys)
    keys2, dig = DevFence(U64, n), DevFence(U8, 32 * n)
    feng.identify_validate_dev(ain.t, oin.t, lin.t, keys2.t, dig.t, arena_bytes=len(host))
    torch.cuda.synchronize()
    assert (keys2.host() == wkeys).all()
    got = dig.host().reshape(n, 32)
    for i in range(n):
        assert got[i].tobytes() == oracle.blake3(host[int(offs[i]):int(offs[i]) + lens[i]].tobytes()), i
    check_all(ain, oin, lin, keys2, dig)


# ---- the path entry points --------------------------------------------------------------------

@pytest.fixture(scope="module")
def files():
    """~20 files on tmpfs, whole and sampled sizes, an empty one, and a path that is missing."""
    import shutil
    d = ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp") + f"/sdcas_fence_{os.getpid()}"
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(9000)
    sizes = [0, 1, 1017, 4096, 57_344, 102_399, 102_400, 102_401, 150_001, 250_000, (1 << 20) + 3,
             3 * (1 << 20) + 5] + [int(x) for x in rng.integers(1, 200_000, 7)]
    paths = []
    for i, s in enumerate(sizes):
        p = os.path.join(d, f"f{i:02d}.bin")
        with open(p, "wb") as fh:
            fh.write(rng.integers(0, 256, s, dtype=U8).tobytes())
        paths.append(p)
    paths.insert(5, os.path.join(d, "missing.bin"))
    sizes.insert(5, 777)
    yield paths, sizes
    shutil.rmtree(d, ignore_errors=True)


def path_array(paths):
    keep = [os.fsencode(p) for p in paths]
    arr = (ctypes.c_char_p * len(keep))(*keep)
    return (keep, arr), ctypes.cast(arr, ctypes.c_void_p).value


def want_paths(oracle, paths, sizes):
    """(keys, cas status, sizes, hex digests, checksum status) as the path entry points document"""
    import errno
    keys, cst, osz, hexes, kst = [], [], [], [], []
    for p, s in zip(paths, sizes):
        if not os.path.exists(p):
            keys.append(0), cst.append(-errno.ENOENT), osz.append(0), hexes.append(""), kst.append(-errno.ENOENT)
            continue
        real = os.path.getsize(p)
        osz.append(real)
        hexes.append(oracle.file_checksum(p))
        kst.append(0)
        if real == 0:
            keys.append(0), cst.append(1)
        else:
            keys.append(int(oracle.generate_cas_id(p, real), 16)), cst.append(0)
    return (np.array(keys, dtype=U64), np.array(cst, dtype=I32), np.array(osz, dtype=U64), hexes,
            np.array(kst, dtype=I32))


def hex_records(fence, n):
    return [bytes(r).split(b"\0")[0].decode() for r in fence.a.reshape(n, 65)]


def test_path_entry_points(feng, oracle, files):
    """generate_cas_ids_from_paths (sizes given and NULL), file_metadata_from_paths,
    file_checksum (out_hex[65]), file_checksums and identify_validate_paths through the raw ABI,
    every host output between guards."""
    paths, given = files
    n = len(paths)
    keep, parr = path_array(paths)
    wk, wc, wz, whex, wks = want_paths(oracle, paths, given)
    real = np.where(wc < 0, 777, wz).astype(U64)
    for sizes in (real, None):
        zin = HostInput(sizes, guard=1 << 40) if sizes is not None else None
        keys, status = HostFence(U64, n), HostFence(I32, n)
        ok(feng, feng.L.sd_cas_generate_cas_ids_from_paths(feng.h, parr, zin.ptr if zin else None, n, keys.ptr,
                                                           status.ptr), "from_paths")
        assert (keys.a == wk).all() and (status.a == wc).all()
        check_all(zin, keys, status)
    keys, status, osz = HostFence(U64, n), HostFence(I32, n), HostFence(U64, n)
    ok(feng, feng.L.sd_cas_file_metadata_from_paths(feng.h, parr, n, keys.ptr, status.ptr, osz.ptr), "metadata")
    assert (keys.a == wk).all() and (status.a == wc).all() and (osz.a == wz).all()
    check_all(keys, status, osz)
    for i in (1, 9, 11, 12):  # a whole file, a sampled one, more than 1 MiB, several MiB
        out = HostFence(U8, 65)
        err = ctypes.c_int(0)
        ok(feng, feng.L.sd_cas_file_checksum(feng.h, os.fsencode(paths[i]), ctypes.cast(out.ptr, ctypes.c_char_p),
                                             ctypes.byref(err)), "file_checksum")
        assert out.a.tobytes() == whex[i].encode() + b"\0"
        out.check("out_hex[65]")
    hexes, kst = HostFence(U8, 65 * n), HostFence(I32, n)
    ok(feng, feng.L.sd_cas_file_checksums(feng.h, parr, n, hexes.ptr, kst.ptr), "file_checksums")
    assert hex_records(hexes, n) == whex and (kst.a == wks).all()
    check_all(hexes, kst)
    keys, status, osz = HostFence(U64, n), HostFence(I32, n), HostFence(U64, n)
    hexes, kst = HostFence(U8, 65 * n), HostFence(I32, n)
    ok(feng, feng.L.sd_cas_identify_validate_paths(feng.h, parr, n, keys.ptr, status.ptr, osz.ptr, hexes.ptr,
                                                   kst.ptr), "identify_validate_paths")
    assert (keys.a == wk).all() and (status.a == wc).all() and (osz.a == wz).all()
    assert hex_records(hexes, n) == whex and (kst.a == wks).all()
    check_all(keys, status, osz, hexes, kst)


def test_generate_cas_ids_host_buffers(feng, oracle):
    """sd_cas_generate_cas_ids: out_keys of exactly n words."""
    rng = np.random.default_rng(9100)
    lens = [0, 1, 1017, 50_000, 102_400, L, L]
    sizes = np.array([0, 1, 1017, 50_000, 102_400, 102_401, 1 << 33], dtype=U64)
    bufs = [rng.integers(0, 256, ln, dtype=U8).tobytes() for ln in lens]
    ptrs = (ctypes.c_char_p * len(bufs))(*bufs)
    lin, zin = HostInput(np.array(lens, dtype=U64), 1 << 40), HostInput(sizes, 1 << 40)
    keys = HostFence(U64, len(bufs))
    ok(feng, feng.L.sd_cas_generate_cas_ids(feng.h, ctypes.cast(ptrs, ctypes.c_void_p), lin.ptr, zin.ptr, len(bufs),
                                            keys.ptr), "generate_cas_ids")
    assert keys.a.tolist() == [oracle.cas_key(b, int(s)) for b, s in zip(bufs, sizes)]
    check_all(lin, zin, keys)


@pytest.mark.parametrize("ring", [False, True])
def test_hash_sampled_host(feng, oracle, ring):
    """sd_cas_hash_sampled_host / _host_ring: 300 files in batches of 128 (a partial last
    batch), h_keys of exactly n words; the ring holds 7 contents."""
    rng = np.random.default_rng(9200)
    n, files_in_ring = 300, 7
    m = files_in_ring if ring else n
    content = rng.integers(0, 256, (m, L), dtype=U8)
    sizes = rng.integers(MINIMUM_FILE_SIZE + 1, 2 ** 40, n, dtype=U64)
    cin, zin = HostInput(content.reshape(-1), 0xFF), HostInput(sizes, 1 << 40)
    keys = HostFence(U64, n)
    if ring:
        rc = feng.L.sd_cas_hash_sampled_host_ring(feng.h, cin.ptr, L, m, zin.ptr, n, keys.ptr, 128)
    else:
        rc = feng.L.sd_cas_hash_sampled_host(feng.h, cin.ptr, L, zin.ptr, n, keys.ptr, 128)
    ok(feng, rc, "hash_sampled_host")
    full = content[np.arange(n) % m]
    assert (keys.a == oracle.fast_cas_keys_strided(full.reshape(-1), L, L, sizes, 4)).all()
    check_all(cin, zin, keys)


# ---- the synthetic generators -----------------------------------------------------------------

@pytest.mark.parametrize("length", [1, 7, 8, 9, (1 << 20) + 3])
def test_synth_stream(feng, oracle, length):
    """d_out is writable to the 8-B round-up of len: the guard starts after it."""
    out = DevFence(U8, length, slack=(-length) % 8)
    feng.synth_stream(55, 3, 4096, length, out.t)
    torch.cuda.synchronize()
    assert (out.host() == oracle.fill_content_range(55, 3, 4096, length)).all()
    check_all(out)


@pytest.mark.parametrize("n", [1, 65])
def test_synth_sampled_and_roots(feng, oracle, n):
    seed, file0 = 12345, 1000
    content, sizes, roots = DevFence(U8, n * L), DevFence(U64, n), DevFence(U64, n)
    feng.synth_sampled(seed, file0, n, content.t, sizes.t, L, dup_permille=300)
    feng.synth_roots(seed, file0, n, roots.t, dup_permille=300)
    torch.cuda.synchronize()
    c, z, r = content.host().reshape(n, L), sizes.host(), roots.host()
    for i in range(n):
        root = oracle.synth_root(seed, file0 + i, 300)
        assert int(r[i]) == root
        assert c[i].tobytes() == oracle.fill_content(seed, root, L)
        assert int(z[i]) == oracle.synth_size(seed, root, 0)
    check_all(content, sizes, roots)


@pytest.mark.parametrize("n", [1, 257])
def test_synth_small(feng, oracle, n):
    """sizes, lens, offs of n entries; the arena's guard starts after the bytes synth_small
    reports.  The keys of the generated files are the oracle's."""
    seed = 777
    sizes, lens, offs = DevFence(U64, n), DevFence(U32, n), DevFence(U64, n)
    need = feng.synth_small(seed, 0, n, sizes.t, lens.t, offs.t, None)
    check_all(sizes, lens, offs)
    arena = DevFence(U8, need)
    assert feng.synth_small(seed, 0, n, sizes.t, lens.t, offs.t, arena.t) == need
    torch.cuda.synchronize()
    check_all(sizes, lens, offs, arena)
    hl, ho, hz, ha = lens.host(), offs.host(), sizes.host(), arena.host()
    assert (ho % 128 == 0).all() and int(ho[-1]) + int(hl[-1]) <= need
    for i in range(n):
        root = oracle.synth_root(seed, i, 0)
        assert int(hz[i]) == int(hl[i]) == oracle.synth_size(seed, root, 1), i
        assert ha[int(ho[i]):int(ho[i]) + int(hl[i])].tobytes() == oracle.fill_content(seed, root, int(hl[i])), i
    # the content alone at the same offsets (the quad holding a tail is written whole)
    oin, lin = DevInput(ho, guard=0), DevInput(hl, guard=0)
    arena2 = DevFence(U8, need)
    feng.synth_small_content(seed, 0, n, oin.t, lin.t, arena2.t)
    torch.cuda.synchronize()
    ha2 = arena2.host()
    for i in range(n):
        assert (ha2[int(ho[i]):int(ho[i]) + int(hl[i])] == ha[int(ho[i]):int(ho[i]) + int(hl[i])]).all(), i
    check_all(oin, lin, arena2)
