"""Plain-numpy references of the fixed-capacity exchange kernels, and the one-GPU emulation
of the exchange that the GPU tests share (tests/test_gpu_parity.py, tests/test_exchange_gpu.py).

`pack_fixed_ref` / `unpack_fixed_ref` state the contracts of
sd_cas_exchange_{pack,unpack}_fixed_dev slice by slice, so they stay usable at millions of
slots; tests/test_shard_cpu.py pins them to HostOps' slot-by-slot Python loops.  Sentinels
come from Python's exact big-integer `range_start`."""
import numpy as np

from spacedrive_amd.shard import range_start
from tests.test_shard_cpu import range_part  # noqa: F401  (re-exported: the partition's contract)


def part_offsets(counts) -> np.ndarray:
    c = np.asarray(counts, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64)


def sentinels(parts: int) -> np.ndarray:
    """sentinel of part p = first key of range p + 1 (the last part's wraps to 0), exact"""
    return np.array([range_start(p + 1, parts) for p in range(parts)], dtype=np.uint64)


def _u32(a) -> np.ndarray:
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.int32 else a.astype(np.uint32)


def pack_fixed_ref(keys, pos, counts, parts: int, cap: int, spill: int, file0: int):
    """(rows u32 [parts*cap, 3], spill rows u32 [parts*spill, 3], overflow flag): slot t of
    part p (main block for t < cap, spill block after) holds row t of the part
    (key lo, key hi, u32(file0 + pos)) for t < counts[p], else (sentinel(p), 0xFFFFFFFF)."""
    k = np.asarray(keys, dtype=np.uint64)
    v = ((np.asarray(pos).astype(np.uint64) + np.uint64(file0)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c = np.asarray(counts, dtype=np.int64)
    off = part_offsets(c)
    sent = sentinels(parts)
    lo, hi = (sent & np.uint64(0xFFFFFFFF)).astype(np.uint32), (sent >> np.uint64(32)).astype(np.uint32)
    klo, khi = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32), (k >> np.uint64(32)).astype(np.uint32)
    out = []
    for width in (cap, spill):
        r = np.empty((parts, width, 3), dtype=np.uint32)
        r[:, :, 0] = lo[:, None]
        r[:, :, 1] = hi[:, None]
        r[:, :, 2] = 0xFFFFFFFF
        out.append(r)
    rows, srows = out
    for q in range(parts):
        m = int(min(c[q], cap))            # real rows of the main block
        s = int(min(c[q], cap + spill)) - m  # real rows of the spill block
        a = int(off[q])
        rows[q, :m, 0], rows[q, :m, 1], rows[q, :m, 2] = klo[a:a + m], khi[a:a + m], v[a:a + m]
        if s:
            b = a + m
            srows[q, :s, 0], srows[q, :s, 1], srows[q, :s, 2] = klo[b:b + s], khi[b:b + s], v[b:b + s]
    return rows.reshape(parts * cap, 3), srows.reshape(parts * spill, 3), int((c > cap + spill).any())


def unpack_fixed_ref(back, spill_back, pos, counts, parts: int, cap: int, spill: int):
    """(rep int64 [n], defined bool [n]): rep[pos[o_p + t]] = the slot's u32 for
    t < min(counts[p], cap + spill); `defined` marks the positions the contract writes."""
    b = _u32(back)
    sb = np.zeros(0, dtype=np.uint32) if spill_back is None else _u32(spill_back)
    p = np.asarray(pos).astype(np.int64)
    c = np.asarray(counts, dtype=np.int64)
    off = part_offsets(c)
    rep = np.full(len(p), -1, dtype=np.int64)
    defined = np.zeros(len(p), dtype=bool)
    for q in range(parts):
        m = int(min(c[q], cap))
        s = int(min(c[q], cap + spill)) - m
        a = int(off[q])
        rep[p[a:a + m]] = b[q * cap: q * cap + m]
        if s:
            rep[p[a + m:a + m + s]] = sb[q * spill: q * spill + s]
        defined[p[a:a + m + s]] = True
    return rep, defined


def split_fixed_ref(rows, sentinel: int):
    """(keys u64, vals u32, sentinel rows): row j with key == sentinel gets key sentinel + j"""
    r = np.asarray(rows).view(np.uint32).reshape(-1, 3)
    k = r[:, 0].astype(np.uint64) | (r[:, 1].astype(np.uint64) << np.uint64(32))
    hit = k == np.uint64(sentinel)
    j = np.arange(len(k), dtype=np.uint64)
    return np.where(hit, np.uint64(sentinel) + j, k), r[:, 2].copy(), int(hit.sum())


# ---- `world` ranks of the fixed-capacity exchange emulated on one GPU -------------------

def pack_senders(ops, keys, world: int, cap: int, spill: int, cuts):
    """Every sender's partition + pack_fixed: [(pos, counts, rows [world, cap, 3],
    spill rows [world, spill, 3], overflow flag tensor)] (device tensors)."""
    import torch
    sent = []
    for r in range(world):
        k = torch.from_numpy(np.ascontiguousarray(keys[cuts[r]:cuts[r + 1]], dtype=np.uint64).view(np.int64)).cuda()
        pk, pp, cnt = ops.partition(k, world)
        rows, srows, ovf = ops.pack_fixed(pk, pp, cnt, world, cap, spill, cuts[r])
        sent.append((pp, cnt, rows.view(world, cap, 3), srows.view(world, spill, 3), ovf))
    return sent


def emulate_fixed_exchange(ops, keys, world: int, cap: int, spill: int, cuts=None):
    """The sync-free exchange with `world` ranks in one process: the all_to_all of equal
    blocks is a block transpose.  Sender r holds keys[cuts[r]:cuts[r+1]] (default: equal
    slices) as global files cuts[r]...  Checks every receiver's split against the sentinel
    rule on the way.  Returns (overflow flags, Objects after subtracting the sentinel rows,
    rep of every file in global order as int64)."""
    import torch
    if cuts is None:
        cuts = [len(keys) * r // world for r in range(world + 1)]
    sent = pack_senders(ops, keys, world, cap, spill, cuts)
    flags = [int(s[4].item()) for s in sent]
    backs = []
    objects = 0
    for d in range(world):  # receiver d: block d of every sender, main then spill
        rr = torch.cat([s[2][d] for s in sent] + [s[3][d] for s in sent])
        rk, rv, nsent = ops.split_fixed(rr, range_start(d + 1, world))
        want, wvals, wsent = split_fixed_ref(rr.cpu().numpy(), range_start(d + 1, world))
        assert int(nsent.item()) == wsent
        # padding spread to distinct keys, real keys untouched
        assert (rk.cpu().numpy().view(np.uint64) == want).all()
        assert (rv.cpu().numpy().view(np.uint32) == wvals).all()
        out, obj = ops.group_min_dev(rk, rv)
        objects += int(obj.item()) - int(nsent.item())
        backs.append(out)
    reps = []
    for r in range(world):  # mirror: sender r gets block r of every receiver's reps
        back = torch.cat([b[:world * cap].view(world, cap)[r] for b in backs])
        sback = torch.cat([b[world * cap:].view(world, spill)[r] for b in backs])
        rep = ops.unpack_fixed(back, sback, sent[r][0], sent[r][1], world, cap, spill)
        reps.append(rep.cpu().numpy())
    return flags, objects, np.concatenate(reps)
