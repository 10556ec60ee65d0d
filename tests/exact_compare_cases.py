"""Inputs, reference and round model of the whole-content compare's tests
(tests/test_exact_compare_cpu.py, tests/test_exact_compare_gpu.py).

A case is (rep, blobs): one u32 label and one bytes object per row.  `reference` is the answer
from the bytes alone, a dict keyed by (rep value, length, bytes).  `model_rounds` replays what the
library does (pivot election round by round, the cap's hand-over to the digest route) on content
identities, so the GPU tests' expected round counts and counters come from here and the CPU test
holds the model to the reference.  `pack` lays the blobs into an arena the way the layout's rules
allow: 16-B aligned offsets, and different garbage in every row's padding up to the 16-B
round-up and in the 16 bytes after it."""
import ctypes

import numpy as np

NO = 0xFFFFFFFF


def constants():
    """(SLICE, PIECE, RUN_K, default max_rounds) from the library's own header."""
    from spacedrive_amd import _native
    out = (ctypes.c_uint64 * 4)()
    fn = _native.lib().sd_content_tasks_constants
    fn.restype, fn.argtypes = None, [ctypes.c_void_p]
    fn(out)
    return tuple(int(v) for v in out)


def reference(rep, blobs):
    """rep_exact[i] = min{ j : rep[j] == rep[i], len j == len i, bytes j == bytes i }."""
    first, out = {}, np.zeros(len(blobs), dtype=np.uint32)
    for i, b in enumerate(blobs):
        out[i] = first.setdefault((int(rep[i]), len(b), b), i)
    return out


def content_ids(blobs):
    ids = {}
    return np.array([ids.setdefault(b, len(ids)) for b in blobs], dtype=np.int64)


def model_rounds(rep, blobs, max_rounds):
    """(rep_exact, rounds, compares, unequal, digest_rows) as the library computes them."""
    n = len(blobs)
    cid = content_ids(blobs)
    lens = np.array([len(b) for b in blobs], dtype=np.int64)
    first = {}
    piv = np.array([first.setdefault((int(rep[i]), int(lens[i])), i) for i in range(n)], dtype=np.int64)
    rep_exact = np.arange(n, dtype=np.int64)
    unres = np.flatnonzero(piv != np.arange(n))
    rounds = compares = unequal = 0
    while len(unres) and not (max_rounds and rounds >= max_rounds):
        rounds += 1
        compares += len(unres)
        eq = cid[unres] == cid[piv[unres]]
        rep_exact[unres[eq]] = piv[unres[eq]]
        ne = unres[~eq]
        unequal += len(ne)
        slot = np.full(n, n, dtype=np.int64)
        np.minimum.at(slot, piv[ne], ne)  # the smallest unequal row of each pivot
        h = slot[piv[ne]]
        rep_exact[ne[h == ne]] = ne[h == ne]
        unres = ne[h != ne]
        piv[unres] = h[h != ne]
    digest_rows = len(unres)
    if digest_rows:  # the rows and their pivots, in row order, split by (pivot value, content)
        val = {int(r): int(piv[r]) for r in unres}
        for p in set(val.values()):
            val[p] = p
        seen = {}
        for r in sorted(val):
            rep_exact[r] = seen.setdefault((val[r], int(cid[r])), r)
    return rep_exact.astype(np.uint32), rounds, compares, unequal, digest_rows


def pack(blobs, seed=1, tail=0):
    """(arena uint8, offs uint64, lens uint64): blob i at a 16-B aligned offset, garbage after it
    to the round-up and for 16 bytes more; `tail` more garbage bytes at the arena's end."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    room = ((lens.astype(np.int64) + 15) & ~15) + 16
    offs = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64) if len(blobs) else np.zeros(0, np.uint64)
    total = int(room.sum()) + tail
    arena = rng.integers(0, 256, max(total, 16), dtype=np.uint8)
    for b, o in zip(blobs, offs.tolist()):
        arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return arena, offs, lens


def flipped(blob, at, x=0xFF):
    b = bytearray(blob)
    b[at] ^= x
    return bytes(b)


def lengths_case(slice_b, piece_b):
    """One class per (L, b): {P, an equal copy, a copy differing in byte b}.  Returns (rep, blobs,
    cases)."""
    rng = np.random.default_rng(20)
    S, P = slice_b, piece_b
    lengths = [1, 15, 16, 17, 31, 32, 33, 1023, 1025, S - 1, S, S + 1, P - 1, P, P + 1, 2 * P + 17]
    rep, blobs, cases = [], [], []
    for L in lengths:
        base = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        at = {0, L - 1}
        for edge in list(range(S, L + 1, S)) + list(range(P, L + 1, P)):
            at |= {x for x in (edge - 1, edge) if 0 <= x < L}
        for b in sorted(at):
            rep += [len(cases)] * 3
            blobs += [base, base, flipped(base, b, 1 << (b % 8))]
            cases.append((L, b))
    return np.array(rep, dtype=np.uint32), blobs, cases


def sweep_case():
    """A 4,101-byte content: one pair (original, copy with byte p flipped) for every p, then one
    equal pair."""
    rng = np.random.default_rng(21)
    L = 4101
    base = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
    rep, blobs = [], []
    for p in range(L):
        rep += [p, p]
        blobs += [base, flipped(base, p, 1 << (p % 8))]
    rep += [L, L]
    blobs += [base, base]
    return np.array(rep, dtype=np.uint32), blobs


def abc_case():
    rng = np.random.default_rng(22)
    a, b, c = (rng.integers(0, 256, 20_000, dtype=np.uint8).tobytes() for _ in range(3))
    return np.full(8, 9, dtype=np.uint32), [a, b, a, c, b, a, c, c]


def classes_case(run_k, slice_b):
    """Classes of 1, 2, K - 1, K, K + 1 and 2 K + 1 copies of an original with the one unequal
    copy first, last and in the middle; two classes whose rows interleave; 40 pairwise-distinct
    rows of one class."""
    rng = np.random.default_rng(23)
    L = slice_b + 100
    rep, blobs, label = [], [], 100
    for copies in (1, 2, run_k - 1, run_k, run_k + 1, 2 * run_k + 1):
        for where in ("first", "last", "middle"):
            base = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
            bad = {"first": 0, "last": copies - 1, "middle": copies // 2}[where]
            rep += [label] * (copies + 1)
            blobs += [base] + [flipped(base, L - 1) if j == bad else base for j in range(copies)]
            label += 1
    x, y = (rng.integers(0, 256, L, dtype=np.uint8).tobytes() for _ in range(2))
    for j in range(12):  # interleaved: x x' y y' ... with every third one changed
        rep += [label, label + 1]
        blobs += [flipped(x, 5) if j % 3 == 2 else x, flipped(y, L // 2) if j % 3 == 1 else y]
    label += 2
    base = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
    for j in range(40):  # pairwise distinct, in the unsampled middle, the first and the last byte
        rep.append(label)
        blobs.append(flipped(base, (j * 211) % L, 1 + j))
    return np.array(rep, dtype=np.uint32), blobs


RANDOM_SEED = 3


def random_case(seed=RANDOM_SEED, n=6000):
    """60 % fresh contents of U(0, 40 KiB) bytes, 25 % equal copies of an earlier row, 15 % copies
    of an earlier row with one byte changed at a uniform position; rep inherited from the copied
    row (a fresh row's rep is its own index)."""
    rng = np.random.default_rng(seed)
    rep, blobs = np.zeros(n, dtype=np.uint32), []
    for i in range(n):
        kind = rng.random()
        if i == 0 or kind < 0.60:
            rep[i] = i
            blobs.append(rng.integers(0, 256, int(rng.integers(0, 40 * 1024 + 1)), dtype=np.uint8).tobytes())
            continue
        src = int(rng.integers(0, i))
        rep[i] = rep[src]
        b = blobs[src]
        if kind >= 0.85 and len(b):
            b = flipped(b, int(rng.integers(0, len(b))), int(rng.integers(1, 256)))
        blobs.append(b)
    return rep, blobs


def random_case_facts(rep, want):
    """(rows with rep_exact < i, rows with rep_exact == i although rep < i, classes with three or
    more distinct contents) of a reference answer."""
    i = np.arange(len(want))
    distinct = {}
    for r, w in zip(rep.tolist(), want.tolist()):
        distinct.setdefault(r, set()).add(w)
    return (int((want < i).sum()), int(((want == i) & (rep < i)).sum()),
            sum(len(v) >= 3 for v in distinct.values()))
