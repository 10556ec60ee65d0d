"""Planted duplicates for the tests of the fused chain's duplicate verification (dup_verify.hip K1V),
and an independent model of what the chain must make of them (test infrastructure; the logic is
plain numpy, torch is imported only by the functions that touch the device).

* probe_np / probe_states: a port of csrc/sd_dup_probe.h, and collide_last_word, which crafts a
  true 64-bit probe collision between two different probe inputs.
* A plan is a list of Group: byte-identical copies of one file, edited per member.  apply() writes
  a plan into device tensors, expect() says from the plan alone what rep, the counters and the
  key classes must be: it never looks at a byte or at a key.
* sweep_plan: one pair per byte offset, the copy one bit apart at that offset.
* fused / check: the helpers of test_dup_verify_gpu.py and test_dup_groups_gpu.py.

expect() relies on the base batch holding pairwise different files with pairwise different
probes (synthetic files of dup_permille = 0), and on a plan's groups being disjoint."""
from dataclasses import dataclass, field

import numpy as np

L = 57_344           # SAMPLED_CONTENT_LEN, sd_dup_probe.h DUP_PROBE_ROW, sd_dup_runs.h DUP_ROW_BYTES
EDGE = 32            # DUP_PROBE_EDGE
TAIL = L - EDGE      # DUP_PROBE_TAIL = 57,312
LAST_WORD = L - 8    # the probe's last chained word: bytes [57,336, 57,344)
PROBE_SEED = 0x5344445550564552
SAMPLE = 2048
M64 = (1 << 64) - 1

# sd_dup_runs.h (its static_asserts: 7 slices of 8 KiB are a row; a slice is 64 lanes x 8 quads)
RUN_K = 16           # DUP_RUN_K: entries of list C per compare task
WAVE = 64            # DUP_WAVE
SLICE_QUADS = 8      # DUP_SLICE_QUADS
SLICE_BYTES = WAVE * SLICE_QUADS * 16
SLICES = L // SLICE_BYTES
MIN_CANDIDATE_SHARE = 32  # ctx_internal.h DUPV_MIN_CANDIDATE_SHARE


# ---- the probe -----------------------------------------------------------------------------

def _mix_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def probe_np(sizes, rows_first32, rows_last32):
    """dup_probe of n files: sizes [n] (any 64-bit integer type), the rows' bytes [0, 32) and
    [57,312, 57,344) as uint8 [n, 32] each.  Returns uint64 [n]."""
    sizes = np.ascontiguousarray(sizes).view(np.uint64).reshape(-1)
    w = np.concatenate([np.ascontiguousarray(rows_first32, dtype=np.uint8).reshape(-1, EDGE),
                        np.ascontiguousarray(rows_last32, dtype=np.uint8).reshape(-1, EDGE)], axis=1)
    w = np.ascontiguousarray(w).view("<u8")  # [n, 8]
    assert w.shape == (len(sizes), 8)
    with np.errstate(over="ignore"):
        h = _mix_np(sizes ^ np.uint64(PROBE_SEED))
        for i in range(8):
            h = _mix_np(h ^ w[:, i])
    return h


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def probe_words(row):
    """The probe's 8 little-endian words of a row (uint8 [57,344])."""
    row = np.asarray(row, dtype=np.uint8)
    assert row.shape == (L,)
    return [int.from_bytes(bytes(row[o:o + 8]), "little")
            for o in list(range(0, EDGE, 8)) + list(range(TAIL, L, 8))]


def probe_states(size, row):
    """The chain's 9 states: [0] after the size, [i + 1] after word i; [8] is the probe."""
    h = [_mix((int(size) & M64) ^ PROBE_SEED)]
    for w in probe_words(row):
        h.append(_mix(h[-1] ^ w))
    return h


def collide_last_word(size_a, row_a, size_b, row_b):
    """Rewrites bytes [57,336, 57,344) of row_b (in place) so that dup_probe(size_b, row_b) ==
    dup_probe(size_a, row_a): with h6, h6' the states before the last word, w7' = w7 ^ h6 ^ h6'."""
    h6 = probe_states(size_a, row_a)[7]
    h6b = probe_states(size_b, row_b)[7]
    w7 = probe_words(row_a)[7] ^ h6 ^ h6b
    row_b[LAST_WORD:] = np.frombuffer(w7.to_bytes(8, "little"), dtype=np.uint8)
    return row_b


def collide_last_words_np(sizes_a, edges_a, sizes_b, edges_b):
    """collide_last_word for n pairs: edges_x are uint8 [n, 64], a row's bytes [0, 32) then
    [57,312, 57,344).  Returns the n crafted last words as uint8 [n, 8]."""
    def h6(sizes, edges):
        w = np.ascontiguousarray(edges, dtype=np.uint8).reshape(-1, 2 * EDGE).view("<u8")
        with np.errstate(over="ignore"):
            h = _mix_np(np.ascontiguousarray(sizes).view(np.uint64).reshape(-1) ^ np.uint64(PROBE_SEED))
            for i in range(7):
                h = _mix_np(h ^ w[:, i])
        return h, w[:, 7]
    ha, w7 = h6(sizes_a, edges_a)
    hb, _ = h6(sizes_b, edges_b)
    return np.ascontiguousarray((w7 ^ ha ^ hb).astype("<u8")).view(np.uint8).reshape(-1, 8)


def in_probe_edge(off):
    return off < EDGE or off >= TAIL


# ---- plans ---------------------------------------------------------------------------------

@dataclass
class Group:
    """Files that start as byte-identical copies of members' smallest index, which stays
    unedited.  flips[f] = {offset: xor mask}, dsize[f] = size delta (mod 2^64), and a member in
    collide gets its last probe word crafted so that its probe equals the original's."""
    members: list
    flips: dict = field(default_factory=dict)
    dsize: dict = field(default_factory=dict)
    collide: set = field(default_factory=set)

    def __post_init__(self):
        self.members = [int(f) for f in self.members]
        o = min(self.members)
        assert len(set(self.members)) == len(self.members)
        for f in list(self.flips) + list(self.dsize) + list(self.collide):
            assert f in self.members and f != o, "the original stays unedited"
        for f in self.collide:
            assert all(off < LAST_WORD for off in self.flips.get(f, {})), "the crafted word is not flipped"

    @property
    def original(self):
        return min(self.members)

    def _edits(self, f):
        fl = tuple(sorted((int(o), int(m) & 0xFF) for o, m in self.flips.get(f, {}).items() if int(m) & 0xFF))
        assert all(0 <= o < L for o, _ in fl)
        return fl, int(self.dsize.get(f, 0)) & M64

    def content_id(self, f):
        """Equal for two members exactly when their sizes and 57,344 bytes are equal."""
        fl, ds = self._edits(f)
        probe_moved = ds != 0 or any(in_probe_edge(o) for o, _ in fl)
        return fl, ds, bool(f in self.collide and probe_moved)  # (the crafted word is a function of the rest)

    def probe_id(self, f):
        """Equal for two members exactly when their probes are equal: the size and the edge
        bytes [0, 32) and [57,312, 57,344) only, or the original's by a crafted collision."""
        fl, ds = self._edits(f)
        if f in self.collide:
            return (), 0
        return tuple((o, m) for o, m in fl if in_probe_edge(o)), ds


@dataclass
class Expected:
    rep: np.ndarray        # int32 [n]: the smallest index with identical size and bytes
    candidates: int
    verified: int
    rehashed: int
    groups: int
    objects: int
    cand: np.ndarray       # int64 [n]: the smallest index of the file's probe class
    planted: np.ndarray    # every member of every group, sorted

    @property
    def counters(self):
        return self.candidates, self.verified, self.rehashed


def _check_disjoint(plan, n):
    seen = np.zeros(n, dtype=bool)
    for g in plan:
        m = np.asarray(g.members)
        assert m.min() >= 0 and m.max() < n and not seen[m].any(), "groups are disjoint"
        seen[m] = True
    return seen


def expect(plan, n):
    """What the fused chain must report for a base batch of n different files with `plan`
    applied — from the construction alone."""
    seen = _check_disjoint(plan, n)
    rep = np.arange(n, dtype=np.int64)
    cand = np.arange(n, dtype=np.int64)
    candidates = verified = groups = 0
    for g in plan:
        first_content, first_probe = {}, {}
        for f in sorted(g.members):
            rep[f] = first_content.setdefault(g.content_id(f), f)
            cand[f] = first_probe.setdefault(g.probe_id(f), f)
        heads = set()
        for f in g.members:
            if cand[f] != f:
                candidates += 1
                heads.add(int(cand[f]))
                verified += g.content_id(f) == g.content_id(int(cand[f]))
        groups += len(heads)
    return Expected(rep.astype(np.int32), candidates, verified, candidates - verified, groups,
                    int((rep == np.arange(n)).sum()), cand, np.flatnonzero(seen))


def apply(plan, content, sizes):
    """Writes the plan into the device tensors content [n, stride >= 57,344] (uint8) and sizes
    [n] (int64), in place: a few batched index_put calls, whatever the plan's length."""
    import torch
    n = int(sizes.numel())
    _check_disjoint(plan, n)
    dev = content.device
    src, dst, dsz, frow, fcol, fmask, crow = [], [], [], [], [], [], []
    for g in plan:
        o = g.original
        for f in g.members:
            if f == o:
                continue
            src.append(o)
            dst.append(f)
            fl, ds = g._edits(f)
            dsz.append(ds)
            for off, m in fl:
                frow.append(f)
                fcol.append(off)
                fmask.append(m)
            if f in g.collide:
                crow.append((f, o))
    if not dst:
        return
    t = lambda a, dt=torch.int64: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev).to(dt)  # noqa: E731
    src_t, dst_t = t(src), t(dst)
    rows = content[:, :L]  # (a view: the stride padding after a row is never written)
    step = 8192  # rows per copy: bounds the gather's temporary to ~0.5 GB
    for i in range(0, len(dst), step):
        rows.index_put_((dst_t[i:i + step],), content[src_t[i:i + step], :L])
    new_sizes = (sizes[src_t].cpu().numpy().view(np.uint64) + np.asarray(dsz, dtype=np.uint64)).view(np.int64)
    sizes.index_put_((dst_t,), torch.from_numpy(new_sizes).to(dev))
    if frow:
        r, c = t(frow), t(fcol)
        content.index_put_((r, c), content[r, c] ^ t(fmask, torch.uint8))
    if crow:
        f_t, o_t = t([f for f, _ in crow]), t([o for _, o in crow])
        edges = lambda r: torch.cat([content[r, :EDGE], content[r, TAIL:L]], dim=1).cpu().numpy()  # noqa: E731
        words = collide_last_words_np(sizes[o_t].cpu().numpy(), edges(o_t), sizes[f_t].cpu().numpy(), edges(f_t))
        content[:, LAST_WORD:L].index_put_((f_t,), torch.from_numpy(words).to(dev))


def apply_np(plan, content, sizes):
    """apply() on host arrays content uint8 [n, 57,344] and sizes uint64 [n] (the CPU tests)."""
    for g in plan:
        o = g.original
        for f in g.members:
            if f == o:
                continue
            content[f] = content[o]
            fl, ds = g._edits(f)
            with np.errstate(over="ignore"):
                sizes[f] = sizes[o] + np.uint64(ds)
            for off, m in fl:
                content[f, off] ^= np.uint8(m)
            if f in g.collide:
                collide_last_word(int(sizes[o]), content[o], int(sizes[f]), content[f])


def sweep_bit(off):
    return 1 << ((off + off // 16) % 8)


def sweep_plan(offsets, n, seed):
    """One pair per offset, both files at shuffled indices: the copy (the larger index) differs
    from its original in exactly one bit, sweep_bit(off), of byte off."""
    offsets = [int(o) for o in offsets]
    assert 2 * len(offsets) <= n
    perm = np.random.default_rng(seed).permutation(n)
    plan = []
    for i, off in enumerate(offsets):
        a, b = sorted((int(perm[2 * i]), int(perm[2 * i + 1])))
        plan.append(Group([a, b], flips={b: {off: sweep_bit(off)}}))
    return plan


# the plans of test_dup_sweep_gpu.py::test_every_byte_offset: (batch quanta, offsets, seed).  One
# quantum launches the 256-lane mixed kernel, two the 512-lane one; each sees every offset once.
SWEEPS = {
    "narrow-lo": (1, range(0, L // 2), 11),
    "narrow-hi": (1, range(L // 2, L), 12),
    "wide": (2, range(0, L), 13),
}


def sweep_case(name, quantum):
    quanta, offsets, seed = SWEEPS[name]
    return sweep_plan(offsets, quanta * quantum, seed)


def locate(off):
    """(slice, quad, lane, word, byte in word) of a row offset in a compare task's loads: the
    inverse of sd_dup_runs.h dup_slice_quad_offset(s, u, lane) + 4 word + byte."""
    s, r = divmod(int(off), SLICE_BYTES)
    q, b = divmod(r, 16)
    u, lane = divmod(q, WAVE)
    return s, u, lane, b // 4, b % 4


def describe(off, mask=None):
    s, u, lane, word, byte = locate(off)
    mask = sweep_bit(off) if mask is None else mask
    bit = 8 * byte + int(mask).bit_length() - 1
    return f"offset {off}: (slice {s}, quad {u}, lane {lane}, word {'xyzw'[word]}, bit {bit})"


# ---- the device helpers of test_dup_verify_gpu.py / test_dup_groups_gpu.py ---------------------

def fused(eng, content, sizes):
    import torch
    n = int(sizes.numel())
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    rep = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    objects = eng.hash_group_sampled(content, sizes, keys, rep, ovf)
    return keys, rep, objects, eng.dup_verify_counters()


def oracle_keys(oracle, content, sizes, idx, threads=8):
    """The oracle's keys of files idx (a sorted, duplicate-free int64 array)."""
    import torch
    host = content[torch.from_numpy(idx).cuda()][:, :L].contiguous().cpu().numpy()
    hs = sizes.cpu().numpy().view(np.uint64)[idx]
    return oracle.cas_keys_strided(host.reshape(-1), L, L, hs, threads)


def check(eng, oracle, content, sizes, keys, rep, objects, edited=()):
    import torch
    n = int(sizes.numel())
    rng = np.random.default_rng(n + len(edited))
    idx = np.unique(np.concatenate([np.asarray(edited, dtype=np.int64), rng.integers(0, n, SAMPLE + 256)]))
    assert len(idx) >= SAMPLE
    want = oracle_keys(oracle, content, sizes, idx, threads=1)
    got = keys.cpu().numpy().view(np.uint64)
    assert (got[idx] == want).all()
    rep2 = torch.empty(n, dtype=torch.int32, device="cuda")
    assert eng.group(keys, rep2) == objects
    assert torch.equal(rep, rep2)
    return got
