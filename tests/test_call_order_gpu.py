"""What a call leaves behind for the next one (MI355X).  The chains of one context share its
workspace, staging and io buffers, the "zero on entry, left zero" bucket totals and region
cursors, the two alternating region sets and the scalar block; the rest of the suite runs on
one session context in one fixed order, so a chain that leaves state behind is seen only if the
test that happens to follow trips over it.  Here every ordered pair (X, P) — X any probe or
disturber, P any probe — runs on a context of its own: X, then P on the same stream with no
synchronize between them where both are asynchronous, and P must be exact.  A probe is a small
call with a fixed input whose reference (oracle, numpy, the job replay) is computed once; a
disturber is a call whose own result is not the point: a refusal after work was queued, an
overflow, a workspace regrow inside a call, a setting switched and switched back."""
import numpy as np
import pytest

from oracle.pyoracle import MINIMUM_FILE_SIZE, SAMPLED_CONTENT_LEN
from spacedrive_amd import CasEngine, CasError
from spacedrive_amd.cas import NO_OBJECT
from tests.exchange_ref import range_part
from tests.golden.make_golden import replay_identifier_job
from tests.test_object_stats_cpu import STAT_NAMES, np_group, np_stats, np_top

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
L = SAMPLED_CONTENT_LEN
EINVAL = -1


def d64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).cuda()


def d32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U32).view(np.int32)).cuda()


def d8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U8)).cuda()


def h64(t):
    return t.cpu().numpy().view(U64)


def h32(t):
    return t.cpu().numpy().view(U32)


def out64(n):
    return torch.full((n,), -1, dtype=torch.int64, device="cuda")


def out32(n):
    return torch.full((n,), -1, dtype=torch.int32, device="cuda")


def _s():
    return int(torch.cuda.current_stream().cuda_stream)


def dup_keys(rng, n, frac=0.3):
    pool = rng.integers(0, 2 ** 64, max(1, int(n * (1 - frac))), dtype=U64)
    return pool[rng.integers(0, len(pool), n)]


def same(a, b) -> bool:
    """results are tuples of numpy arrays and ints"""
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


class Call:
    """launch(eng) enqueues the call with fresh outputs and returns fetch(): synchronise and
    return the result as a tuple.  A probe carries `want`; a disturber only launches."""

    def __init__(self, name, launch, want=None):
        self.name, self.launch, self.want = name, launch, want


# ---- the probes -------------------------------------------------------------------------------

def make_probes(oracle):
    rng = np.random.default_rng(20_000)
    probes = []

    keys = dup_keys(rng, 5000)
    dk = d64(keys)
    orep, oobj = oracle.group_canonical(keys)

    def group(eng):
        rep = out32(5000)
        eng.group(dk, rep, want_objects=False)
        cnt = out64(1)
        eng._check(eng.L.sd_cas_copy_objects_dev(eng.h, cnt.data_ptr(), _s()), "copy_objects")
        return lambda: (h32(rep), int(cnt.cpu()[0]))
    probes.append(Call("group", group, (orep, oobj)))

    def group_sort(eng):
        rep = out32(5000)
        eng.set_group_method(eng.GROUP_SORT)
        try:
            eng.group(dk, rep, want_objects=False)
        finally:
            eng.set_group_method()
        return lambda: (h32(rep),)
    probes.append(Call("group_sort", group_sort, (orep,)))

    vals = rng.integers(0, 2 ** 32, 5000, dtype=U64).astype(U32)
    dv = d32(vals)
    uniq, inv = np.unique(keys, return_inverse=True)
    mins = np.full(len(uniq), 0xFFFFFFFF, dtype=U32)
    np.minimum.at(mins, inv.reshape(-1), vals)

    def group_min(eng):
        out = out32(5000)
        eng.group_min(dk, dv, out, want_objects=False)
        return lambda: (h32(out),)
    probes.append(Call("group_min", group_min, (mins[inv.reshape(-1)],)))

    skeys = rng.integers(0, 2 ** 64, 4097, dtype=U64)
    skeys[:1000] = skeys[2000]
    dsk = d64(skeys)
    order = np.argsort(skeys, kind="stable")

    def sort_pairs(eng):
        ko, vo = out64(4097), out32(4097)
        eng.sort_pairs(dsk, None, ko, vo)
        return lambda: (h64(ko), h32(vo))
    probes.append(Call("sort_pairs", sort_pairs, (skeys[order], order.astype(U32))))

    part = range_part(keys, 7)
    pcounts = np.bincount(part, minlength=7).astype(U64)
    porder = np.lexsort((np.arange(5000), part))  # by part, then by input position

    def partition(eng):
        ko, po, counts = out64(5000), out32(5000), out64(7)
        eng.partition(dk, 7, ko, po, counts)

        def fetch():  # the order inside a part is unspecified: by position inside each part
            k, p = h64(ko), h32(po).astype(np.int64)
            o = np.lexsort((p, range_part(k, 7)))
            return k[o], p[o].astype(U32), h64(counts)
        return fetch
    probes.append(Call("partition", partition, (keys[porder], porder.astype(U32), pcounts)))

    lens = [0, 1, 1017, 102_400] + [int(x) for x in rng.integers(0, 40_000, 296)]
    offs, o = [], 0
    for ln in lens:
        offs.append(o)
        o += (ln + 15) // 16 * 16 + 16
    arena = rng.integers(0, 256, o + 16, dtype=U8)
    psizes = np.array(lens, dtype=U64)
    poffs = np.array(offs, dtype=U64)
    pwant = oracle.cas_keys(arena, poffs, psizes, psizes)
    da, dpo, dpl, dpz = d8(arena), d64(poffs), d32(np.array(lens, dtype=U32)), d64(psizes)

    def hash_packed(eng):
        k = out64(300)
        eng.hash_packed(da, dpo, dpl, dpz, k)
        return lambda: (h64(k),)
    probes.append(Call("hash_packed", hash_packed, (pwant,)))

    content = rng.integers(0, 256, (77, L), dtype=U8)
    ssizes = rng.integers(MINIMUM_FILE_SIZE + 1, 2 ** 40, 77, dtype=U64)
    swant = oracle.fast_cas_keys_strided(content.reshape(-1), L, L, ssizes, 4)
    dc, dz = d8(content), d64(ssizes)

    def hash_sampled(eng):
        k = out64(77)
        eng.hash_sampled(dc, dz, k)
        return lambda: (h64(k),)
    probes.append(Call("hash_sampled", hash_sampled, (swant,)))

    clens = [0, 1, 1025, (1 << 20) + 1] + [int(x) for x in rng.integers(0, 200_000, 36)]
    coffs = (np.cumsum([0] + [(ln + 15) // 16 * 16 + 16 for ln in clens])[:-1]).astype(U64)
    carena = rng.integers(0, 256, int(coffs[-1]) + (clens[-1] + 15) // 16 * 16 + 16, dtype=U8)
    cwant = np.frombuffer(b"".join(oracle.blake3(carena[int(f):int(f) + ln].tobytes())
                                   for f, ln in zip(coffs, clens)), dtype=U8)
    dca, dco, dcl = d8(carena), d64(coffs), d64(np.array(clens, dtype=U64))

    def checksums(eng):
        out = torch.zeros(40 * 32, dtype=torch.uint8, device="cuda")
        eng.checksums_dev(dca, dco, dcl, out)
        return lambda: (out.cpu().numpy(),)
    probes.append(Call("checksums", checksums, (cwant,)))

    from tests.test_inplace_gpu import want_keys
    hlens = [150_001, 0, 1017, 102_401] + [int(x) for x in rng.integers(0, 200_000, 16)]
    hoffs = (np.cumsum([0] + [(ln + 15) // 16 * 16 + 16 for ln in hlens])[:-1]).astype(U64)
    harena = rng.integers(0, 256, int(hoffs[-1]) + (hlens[-1] + 15) // 16 * 16 + 16, dtype=U8)
    hwant = want_keys(oracle, harena, hoffs, hlens)
    dha, dho, dhl = d8(harena), d64(hoffs), d64(np.array(hlens, dtype=U64))

    def hash_contents(eng):
        k = out64(20)
        eng.hash_contents(dha, dho, dhl, k)
        return lambda: (h64(k),)
    probes.append(Call("hash_contents", hash_contents, (hwant,)))

    n = 3000
    lkeys = dup_keys(rng, n)
    states = rng.choice(np.array([0, 1, 2], dtype=U8), n, p=[0.9, 0.05, 0.05])
    ids = rng.permutation(4 * n).astype(U32)
    sk = lkeys[rng.random(n) < 0.2].astype(U64)
    so = ids[:len(sk)]
    pre = np.where(rng.random(n) < 0.1, ids[n:2 * n], NO_OBJECT).astype(U32)
    ws, wo, wa, wc = replay_identifier_job(
        [int(k) for k in lkeys], [int(s) for s in states], 7,
        existing=list(zip((int(k) for k in sk), (int(x) for x in so))),
        pre_objects=[None if int(p) == NO_OBJECT else int(p) for p in pre])
    dlk, dst, dsk2, dso, dpre = d64(lkeys), d8(states), d64(sk), d32(so), d32(pre)

    def links(eng):
        step, obj, act, counts = eng.identifier_links(dlk, dst, 7, existing=(dsk2, dso), pre_objects=dpre)
        return lambda: (h32(step), h32(obj), act.cpu().numpy(), counts)
    probes.append(Call("identifier_links_ex", links,
                       (np.array(ws, dtype=U32), np.array(wo, dtype=U32), np.array(wa, dtype=U8),
                        np.array(wc, dtype=np.int64).reshape(-1, 2))))

    rep, _ = np_group(keys)
    zsizes = (keys >> U64(24)) + U64(1)
    wcopies, wtot = np_stats(rep, zsizes)
    th, tw, nf = np_top(rep, zsizes, wcopies, 9)
    drep, dzs = d32(rep), d64(zsizes)

    def stats_top(eng):
        copies, heads, waste = out32(5000), out32(9), out64(9)
        totals = eng.object_stats(drep, dzs, copies)
        found = eng.top_duplicates(drep, dzs, copies, 9, heads, waste)
        return lambda: (h32(copies), np.array(list(totals.values()), dtype=U64), h32(heads), h64(waste), found)
    probes.append(Call("stats_top", stats_top,
                       (wcopies, np.array([wtot[q] for q in STAT_NAMES], dtype=U64), th, tw, nf)))

    from tests.test_thumbnail import hex_table, records
    prefix = b"/data/thumbnails/ephemeral/"
    stride = (len(prefix) + 26 + 15) // 16 * 16
    twant = records(prefix, hex_table(keys), stride).reshape(-1)

    def thumbs(eng):
        out = torch.full((5000 * stride,), 0xAB, dtype=torch.uint8, device="cuda")
        eng._check(eng.L.sd_cas_thumbnail_paths_dev(eng.h, dk.data_ptr(), 5000, prefix, stride, out.data_ptr(),
                                                    _s()), "thumbnail_paths")
        return lambda: (out.cpu().numpy(),)
    probes.append(Call("thumbnail_paths", thumbs, (twant,)))
    return probes


@pytest.fixture(scope="module")
def world(oracle):
    """The probes and disturbers with their inputs on the device and their references (made
    once per module, read-only), one quantum of sampled content among them."""
    assert torch.cuda.is_available(), "GPU tests need a gfx950 device"
    probes = make_probes(oracle)
    with CasEngine(0) as eng:
        q = eng.batch_quantum
        content = torch.empty((q, L), dtype=torch.uint8, device="cuda")
        sizes = torch.empty(q, dtype=torch.int64, device="cuda")
        eng.synth_sampled(0x4B33, 0, q, content, sizes, L, dup_permille=300)
        torch.cuda.synchronize()
        host = content.cpu().numpy()
        qkeys = oracle.fast_cas_keys_strided(host.reshape(-1), L, L, h64(sizes), 16)
        del host
        # the same quantum with one file copied 3,000 times: a coarse bucket outgrows its region
        hot = content.clone()
        hsizes = sizes.clone()
        idx = torch.from_numpy(np.random.default_rng(5).choice(np.arange(1, q), 3000, replace=False)).cuda()
        hot[idx] = hot[0].clone()
        hsizes[idx] = hsizes[0].clone()
        torch.cuda.synchronize()
    qrep, qobj = oracle.group_canonical(qkeys)

    def fused(eng):
        keys, rep = out64(q), out32(q)
        ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.hash_group_sampled(content, sizes, keys, rep, ovf, want_objects=False)
        cnt = out64(1)
        eng._check(eng.L.sd_cas_copy_objects_dev(eng.h, cnt.data_ptr(), _s()), "copy_objects")
        return lambda: (h64(keys), h32(rep), int(ovf.cpu()[0]), int(cnt.cpu()[0]))
    probes.append(Call("hash_group_sampled", fused, (qkeys, qrep, 0, qobj)))

    # ---- the disturbers
    rng = np.random.default_rng(20_001)
    disturbers = []

    def refused(fn):
        def launch(eng):
            with pytest.raises(CasError) as e:
                fn(eng)
            assert e.value.code == EINVAL
            return lambda: ()
        return launch

    coffs = np.array([0, 4096 + 8, 8192], dtype=U64)  # the second offset is misaligned
    carena = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    dco, dcl = d64(coffs), d64(np.array([100, 200, 300], dtype=U64))
    disturbers.append(Call("refused checksums", refused(
        lambda eng: eng.checksums_dev(carena, dco, dcl, torch.zeros(96, dtype=torch.uint8, device="cuda")))))

    bk = d64(rng.integers(0, 2 ** 64, 3000, dtype=U64))
    bst = d8(np.zeros(3000, dtype=U8))
    bad_pre = np.full(3000, NO_OBJECT, dtype=U32)
    bad_pre[[5, 2999]] = [7, 2 ** 31]
    dbad = d32(bad_pre)
    disturbers.append(Call("refused links", refused(
        lambda eng: eng.identifier_links(bk, bst, 7, pre_objects=dbad))))

    brep = np.arange(1000, dtype=U32)
    brep[[10, 20, 30]] = [11, 1000, 5]
    dbrep, dbsz = d32(brep), d64(np.full(1000, 4096, dtype=U64))
    disturbers.append(Call("refused stats", refused(
        lambda eng: eng.object_stats(dbrep, dbsz, out32(1000)))))

    def pack_1025(eng):
        rows = out32(3 * 4100)
        eng._check(eng.L.sd_cas_exchange_pack_fixed_dev(
            eng.h, bk.data_ptr(), dbrep.data_ptr(), dbsz.data_ptr(), 1025, 4, 0, 0, rows.data_ptr(), None,
            torch.zeros(1, dtype=torch.int32, device="cuda").data_ptr(), _s()), "pack_fixed")
    disturbers.append(Call("refused pack_fixed", refused(pack_1025)))

    def hot_key(eng):
        keys, rep = out64(q), out32(q)
        ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.hash_group_sampled(hot, hsizes, keys, rep, ovf, want_objects=False)
        return lambda: (int(ovf.cpu()[0]),)
    disturbers.append(Call("fused overflow", hot_key, (1,)))

    from tests.test_gpu_parity import unmix64
    crafted = d64(np.array([unmix64(int(x) >> 3) for x in rng.integers(0, 2 ** 63, 8000, dtype=U64)], dtype=U64))

    def one_bucket(eng):
        eng.group(crafted, out32(8000), want_objects=False)
        return lambda: ()
    disturbers.append(Call("one-bucket group", one_bucket))

    m = 200_000  # 100,000 candidates in one bin: the workspace regrows inside the call
    trep = d32(np.arange(m) & ~1)
    tsz = torch.full((m,), 4096, dtype=torch.int64, device="cuda")

    def regrow(eng):
        copies = out32(m)
        eng.object_stats(trep, tsz, copies, want_totals=False)
        assert eng.top_duplicates(trep, tsz, copies, 50, out32(50), out64(50)) == 50
        return lambda: ()
    disturbers.append(Call("top_duplicates regrow", regrow))

    def switch(eng):
        eng.set_group_method(eng.GROUP_HASH, 16)
        eng.set_group_method(eng.GROUP_SORT)
        eng.set_group_method()
        return lambda: ()
    disturbers.append(Call("group method switched back", switch))

    calls = {c.name: c for c in probes + disturbers}
    yield calls
    del content, hot
    torch.cuda.empty_cache()


PROBES = ["group", "group_sort", "group_min", "sort_pairs", "partition", "hash_packed", "hash_sampled",
          "checksums", "hash_contents", "identifier_links_ex", "stats_top", "thumbnail_paths",
          "hash_group_sampled"]
DISTURBERS = ["refused checksums", "refused links", "refused stats", "refused pack_fixed", "fused overflow",
              "one-bucket group", "top_duplicates regrow", "group method switched back"]


def test_the_lists_name_every_call(world):
    assert sorted(world) == sorted(PROBES + DISTURBERS)
    assert all(world[p].want is not None for p in PROBES)


def test_disturbers_do_what_they_claim(world):
    """The overflow disturber raises its flag (the refusals assert their own EINVAL)."""
    with CasEngine(0) as eng:
        assert world["fused overflow"].launch(eng)() == world["fused overflow"].want


@pytest.mark.parametrize("p", PROBES)
@pytest.mark.parametrize("x", PROBES + DISTURBERS)
def test_probe_after(world, x, p):
    """X, then P on the same stream of a fresh context, nothing awaited in between: P exact."""
    with CasEngine(0) as eng:
        keep = world[x].launch(eng)  # (X's outputs stay allocated while P runs)
        got = world[p].launch(eng)()
        del keep
    assert same(got, world[p].want), f"{p} after {x}"


FIXED = dict(zip(PROBES, (DISTURBERS * 2)[:len(PROBES)]))


@pytest.mark.parametrize("p", PROBES)
def test_probe_disturber_probe(world, p):
    """P, X, P with one fixed disturber per probe: both results exact and identical."""
    x = FIXED[p]
    with CasEngine(0) as eng:
        first = world[p].launch(eng)()
        keep = world[x].launch(eng)
        second = world[p].launch(eng)()
        del keep
    assert same(first, world[p].want), f"{p} before {x}"
    assert same(second, first), f"{p} after {x}"
