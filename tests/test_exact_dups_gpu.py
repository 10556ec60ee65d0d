"""GPU tests of the exact duplicate grouping: sd_cas_group_exact_dev (a grouping split by
32-byte whole-content digest, fast key + verify or the word-wise path), the host report
sd_cas_duplicate_report_exact, CasEngine.exact_duplicates over real files and the C example's
--exact flag.  The reference answer of a grouping is numpy in this file: np.unique over the
structured (rep, digest) rows, mapped to the first index of each distinct row.

The fast key is le64(digest[0..8]) ^ rep * 0x9E3779B97F4A7C15 (include/sd_hip_cas.h), so rows
of one rep whose digests differ in bytes 8..32 only collide by construction: that is how these
tests reach the word-wise path under EXACT_AUTO."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import spacedrive_amd as sa
from spacedrive_amd import CasError
from tests.fence import DevFence, DevInput, HostFence, check_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = sa.NO_OBJECT
ROW = np.dtype([("r", "<u4"), ("w0", "<u8"), ("w1", "<u8"), ("w2", "<u8"), ("w3", "<u8")])


def ref_group(rep, dig):
    """(rep_exact, objects) by numpy: dig uint8 [n, 32], rep uint32 [n] or None."""
    n = len(dig)
    rows = np.zeros(n, dtype=ROW)
    if n == 0:
        return np.zeros(0, dtype=np.uint32), 0
    if rep is not None:
        rows["r"] = rep
    w = np.ascontiguousarray(dig).view("<u8").reshape(n, 4)
    for j in range(4):
        rows[f"w{j}"] = w[:, j]
    _, first, inv = np.unique(rows, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.uint32), len(first)


@pytest.fixture
def methods(eng):
    """Leaves the shared engine on its defaults whatever a test set."""
    yield eng
    eng.set_group_method(eng.GROUP_AUTO, 0)
    eng.set_exact_method(sa.EXACT_AUTO)


def run(eng, rep, dig, exact_method, want=None):
    """One fenced group_exact call; returns (rep_exact, objects, counters) and compares with
    `want` = ref_group's answer when given."""
    n = len(dig)
    flat = np.ascontiguousarray(dig, dtype=np.uint8).reshape(-1)
    d_dig = DevInput(flat, guard=int(flat[0]) if n else 0)
    d_rep = None if rep is None else DevInput(np.ascontiguousarray(rep, dtype=np.uint32),
                                              guard=int(rep[0]) if n else 0)
    out = DevFence(np.uint32, n)
    eng.set_exact_method(exact_method)
    objects = eng.group_exact(None if d_rep is None else d_rep.t, d_dig.t, out.t)
    counters = eng.group_exact_counters()
    check_all(out, d_dig, d_rep)
    got = out.host()
    if want is not None:
        assert objects == want[1]
        assert (got == want[0]).all(), np.flatnonzero(got != want[0])[:8]
    if exact_method == sa.EXACT_WORDS:
        assert counters == (0, 1 if n else 0)
    return got, objects, counters


def pooled(rng, n):
    """n digests from a pool of n/3 values, a prior rep from a smaller pool."""
    pool = rng.integers(0, 256, (max(1, n // 3), 32), dtype=np.uint8)
    dig = pool[rng.integers(0, len(pool), n)]
    reps = rng.integers(0, 2 ** 32, max(1, n // 8), dtype=np.uint64).astype(np.uint32)
    return reps[rng.integers(0, len(reps), n)], dig


@pytest.mark.parametrize("group_method", [0, 1, 2], ids=["auto", "hash", "sort"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_edge_sizes(methods, n, group_method):
    eng = methods
    rng = np.random.default_rng(1000 + n)
    rep, dig = pooled(rng, n)
    want = ref_group(rep, dig)
    want_norep = ref_group(None, dig)
    eng.set_group_method(group_method, 0)
    for em in (sa.EXACT_AUTO, sa.EXACT_WORDS):
        run(eng, rep, dig, em, want)
        run(eng, None, dig, em, want_norep)


def sweep_rows():
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    dig = np.tile(base, (257, 1))
    for k in range(1, 257):
        b = k - 1
        dig[k, b // 8] ^= np.uint8(1 << (b % 8))
    return dig


def test_bit_sweep(methods):
    """Row 0 a base digest, row k the base with bit k - 1 flipped: 257 Objects.  Bits 64..255
    are outside the fast key, so those 192 rows collide with row 0 there and AUTO must fall back."""
    eng = methods
    dig = sweep_rows()
    rep = np.full(257, 5, dtype=np.uint32)
    want = ref_group(rep, dig)
    assert want[1] == 257 and (want[0] == np.arange(257)).all()
    _, _, (mismatched, fallbacks) = run(eng, rep, dig, sa.EXACT_AUTO, want)
    assert fallbacks == 1 and mismatched >= 192
    run(eng, rep, dig, sa.EXACT_WORDS, want)


@pytest.mark.parametrize("order", ["interleaved", "reversed"])
def test_bit_sweep_with_copies(methods, order):
    """Each row duplicated once and interleaved (heads at even indices); then the whole array
    reversed, so every copy pair's FIRST row in the new order must become the head."""
    eng = methods
    dig = np.repeat(sweep_rows(), 2, axis=0)
    if order == "reversed":
        dig = dig[::-1].copy()
    rep = np.full(514, 0x80000001, dtype=np.uint32)
    want = ref_group(rep, dig)
    assert want[1] == 257 and (want[0] == (np.arange(514) & ~1)).all()
    for em in (sa.EXACT_AUTO, sa.EXACT_WORDS):
        got, _, (mismatched, fallbacks) = run(eng, rep, dig, em, want)
        if em == sa.EXACT_AUTO:
            assert fallbacks == 1 and mismatched >= 192


def test_prior_rep_separates_and_null_merges(methods):
    eng = methods
    d = np.random.default_rng(3).integers(0, 256, 32, dtype=np.uint8)
    dig = np.tile(d, (6, 1))
    rep = np.array([1, 2, 1, 2, 3, 1], dtype=np.uint32)
    for em in (sa.EXACT_AUTO, sa.EXACT_WORDS):
        got, objects, _ = run(eng, rep, dig, em, ref_group(rep, dig))
        assert got.tolist() == [0, 1, 0, 1, 4, 0] and objects == 3
        got, objects, _ = run(eng, None, dig, em, ref_group(None, dig))
        assert got.tolist() == [0] * 6 and objects == 1


def test_prior_rep_is_a_value_not_an_index(methods):
    """rep holds 0xFFFFFFFF and values >= n: never dereferenced, grouped as plain values."""
    eng = methods
    n = 1000
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    dig = pool[rng.integers(0, 40, n)]
    vals = np.array([0xFFFFFFFF, 0xFFFFFFFE, n, n + 5, 1 << 31, 0], dtype=np.uint32)
    rep = vals[rng.integers(0, len(vals), n)]
    want = ref_group(rep, dig)
    for em in (sa.EXACT_AUTO, sa.EXACT_WORDS):
        run(eng, rep, dig, em, want)


def test_classes_cut_by_every_word(methods):
    """Rows that share (rep, d0) and differ only in d1, only in d2 or only in d3 (fast-key
    collisions), and rows that share d1..d3 and differ in d0, words drawn from tiny pools so
    every word value is shared across classes; shuffled.  Both methods give numpy's answer."""
    eng = methods
    rng = np.random.default_rng(5)
    small = [rng.integers(0, 2 ** 63, 3, dtype=np.uint64) for _ in range(4)]
    rows = []
    for b in range(341):
        r = b % 5
        w = [rng.integers(0, 2 ** 63, dtype=np.uint64) if j == 0 else small[j][rng.integers(0, 3)] for j in range(4)]
        variants = [list(w)]
        for j in (1, 2, 3):  # only word j differs
            v = list(w)
            v[j] = small[j][(int(np.flatnonzero(small[j] == w[j])[0]) + 1) % 3]
            variants.append(v)
        for t in (0, 1):  # only d0 differs
            v = list(w)
            v[0] = small[0][t]
            variants.append(v)
        for v in variants:
            rows += [(r, v), (r, v)]
    perm = rng.permutation(len(rows))
    rep = np.array([rows[i][0] for i in perm], dtype=np.uint32)
    dig = np.array([rows[i][1] for i in perm], dtype="<u8").view(np.uint8).reshape(-1, 32)
    assert len(rep) == 4092
    want = ref_group(rep, dig)
    a, _, (mismatched, fallbacks) = run(eng, rep, dig, sa.EXACT_AUTO, want)
    assert fallbacks == 1 and mismatched > 0
    w_, _, _ = run(eng, rep, dig, sa.EXACT_WORDS, want)
    assert (a == w_).all()


def test_random_scale(methods):
    """200,003 rows of uniform random digests, 30 % of them copies of an earlier row.  No
    fallback is a condition: the chance of one 64-bit collision is about n^2 / 2^65 ~ 1e-9."""
    import torch
    eng = methods
    n, uniq = 200_003, 140_002
    rng = np.random.default_rng(2024)
    dig = np.empty((n, 32), dtype=np.uint8)
    dig[:uniq] = rng.integers(0, 256, (uniq, 32), dtype=np.uint8)
    rep = np.empty(n, dtype=np.uint32)
    rep[:uniq] = rng.integers(0, 1000, uniq)
    src = rng.integers(0, uniq, n - uniq)
    dig[uniq:], rep[uniq:] = dig[src], rep[src]
    perm = rng.permutation(n)
    dig, rep = dig[perm], rep[perm]
    want = ref_group(rep, dig)
    assert want[1] == uniq
    a, objects, (mismatched, fallbacks) = run(eng, rep, dig, sa.EXACT_AUTO, want)
    assert (mismatched, fallbacks) == (0, 0)
    d_obj = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    assert eng.L.sd_cas_copy_objects_dev(eng.h, d_obj.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert int(d_obj.item()) == objects == uniq
    w, _, _ = run(eng, rep, dig, sa.EXACT_WORDS, want)
    assert eng.L.sd_cas_copy_objects_dev(eng.h, d_obj.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert int(d_obj.item()) == uniq and (a == w).all()


def test_argument_refusals(methods):
    import torch
    eng = methods
    n = 64
    rng = np.random.default_rng(9)
    rep, dig = pooled(rng, n)
    d_rep = DevInput(rep, guard=int(rep[0]))
    d_dig = DevInput(dig.reshape(-1), guard=0, slack=64)
    out = DevFence(np.uint32, n)
    stream = int(torch.cuda.current_stream().cuda_stream)
    obj = ctypes.c_uint64(77)

    def call(rep_ptr, dig_ptr, nn, out_ptr):
        return eng.L.sd_cas_group_exact_dev(eng.h, rep_ptr, dig_ptr, nn, out_ptr, ctypes.byref(obj), stream)
    # rep_exact aliases rep (the same array, and an overlapping one)
    assert call(d_rep.ptr, d_dig.ptr, n, d_rep.ptr) == -1
    assert call(d_rep.ptr, d_dig.ptr, n, d_rep.ptr + 4 * (n - 1)) == -1
    assert call(out.ptr + 8, d_dig.ptr, n - 2, out.ptr) == -1
    # a digest pointer that is not 16-B aligned
    assert call(d_rep.ptr, d_dig.ptr + 8, n, out.ptr) == -1
    with pytest.raises(CasError) as e:
        eng.group_exact(d_rep.t, d_dig.buf[4096 + 8:4096 + 8 + 32 * n], out.t)
    assert e.value.code == -1
    # n >= 2^32
    assert call(d_rep.ptr, d_dig.ptr, 1 << 32, out.ptr) == -1
    assert call(None, d_dig.ptr, (1 << 32) + 5, out.ptr) == -1
    # null digests / output
    assert call(d_rep.ptr, None, n, out.ptr) == -1
    assert call(d_rep.ptr, d_dig.ptr, n, None) == -1
    assert eng.L.sd_cas_set_exact_method(eng.h, 2) == -1 and eng.L.sd_cas_set_exact_method(eng.h, -1) == -1
    torch.cuda.synchronize()
    assert obj.value == 77
    assert (out.host().view(np.uint8) == 0xC3).all()
    check_all(out, d_rep, d_dig)


# ---- files ---------------------------------------------------------------------------------
NAMES = ["f0_A", "f1_B1", "f2_B2", "f3_C", "f4_X", "f5_D", "f6_E"]


@pytest.fixture(scope="module")
def file_set(tmp_path_factory):
    """A 300,000 random bytes; B1 / B2 = A with an UNSAMPLED byte changed (the first and the
    last one: tests/test_exact_dups_cpu.py::test_sampling_gap); C = A; X = A with a SAMPLED byte
    changed; D = E, 50,000 bytes (hashed whole)."""
    d = tmp_path_factory.mktemp("exact_files")
    rng = np.random.default_rng(42)
    a = rng.integers(0, 256, 300_000, dtype=np.uint8)

    def flipped(at):
        b = a.copy()
        b[at] ^= 0xFF
        return b
    small = rng.integers(0, 256, 50_000, dtype=np.uint8)
    blobs = [a, flipped(18_432), flipped(291_807), a, flipped(18_431), small, small]
    for name, blob in zip(NAMES, blobs):
        (d / name).write_bytes(blob.tobytes())
    return d, [str(d / name) for name in NAMES]


def test_files_exact_duplicates(eng, file_set):
    """The sampled cas_id puts A, B1, B2 and C into one Object and calls 900,000 bytes waste;
    only A and C are copies."""
    _, paths = file_set
    rep = eng.exact_duplicates(paths, k=3)
    assert rep.rep.tolist() == [0, 0, 0, 0, 4, 5, 5]
    assert rep.rep_exact.tolist() == [0, 1, 2, 0, 4, 5, 5]
    assert rep.copies_exact.tolist() == [2, 1, 1, 2, 1, 2, 2]
    assert rep.unconfirmed == 0
    assert rep.totals["objects"] == 3 and rep.totals_exact["objects"] == 5
    assert rep.totals["rows"] == rep.totals_exact["rows"] == 7
    assert rep.totals["total_bytes"] == rep.totals_exact["total_bytes"] == 5 * 300_000 + 100_000
    assert rep.totals_exact["unique_bytes"] - rep.totals["unique_bytes"] == 600_000
    assert rep.totals["duplicate_sets"] == 2 and rep.totals_exact["duplicate_sets"] == 2
    assert rep.totals["max_copies"] == 4 and rep.totals_exact["max_copies"] == 2
    assert rep.top_heads.tolist() == [0, 5, NO] and rep.top_waste.tolist() == [300_000, 50_000, 0]
    # the sampled report's top entry, from the same keys
    keys, status, sizes, digests, errnos = eng.identify_validate(paths)
    assert (status == 0).all() and (errnos == 0).all()
    sampled = eng.duplicate_report(keys, sizes, k=1)
    assert sampled.top_waste.tolist() == [900_000] and (sampled.rep == rep.rep).all()
    assert sampled.totals == rep.totals
    assert len({digests[0], digests[1], digests[2], digests[4]}) == 4 and digests[0] == digests[3]


def test_example_exact_flag(file_set):
    d, paths = file_set
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "-s"], check=True)
    exe = os.path.join(ROOT, "examples", "sd_duplicates")
    r = subprocess.run([exe, str(d), "--exact"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    plain = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    base = json.loads(plain.stdout)
    assert "exact" not in base and "unconfirmed" not in base
    assert {k: v for k, v in out.items() if k not in ("exact", "unconfirmed")} == base
    assert out["totals"]["objects"] == 3 and out["top"][0]["waste"] == 900_000
    assert out["unconfirmed"] == 0
    assert out["exact"]["totals"] == {
        "rows": 7, "objects": 5, "total_bytes": 1_600_000, "unique_bytes": 1_250_000,
        "duplicate_sets": 2, "max_copies": 2, "size_mismatch_rows": 0, "bad_rows": 0}
    top = out["exact"]["top"]
    assert [(t["waste"], t["copies"], t["size"], t["paths"]) for t in top] == [
        (300_000, 2, 300_000, [paths[0], paths[3]]), (50_000, 2, 50_000, [paths[5], paths[6]])]
    assert len(top[0]["checksum"]) == 64 and top[0]["cas_id"] == out["top"][0]["cas_id"]


# ---- the host report -----------------------------------------------------------------------
def report_case():
    rng = np.random.default_rng(77)
    n = 3000
    key_pool = rng.integers(1, 2 ** 63, 300, dtype=np.uint64)
    kidx = rng.integers(0, 300, n)
    variant = rng.integers(0, 3, n)  # up to three different contents behind one cas_id
    keys = key_pool[kidx]
    digests = [bytes([int(kidx[i]) & 255, int(kidx[i]) >> 8, int(variant[i])] + [0x5A] * 29).hex() for i in range(n)]
    sizes = (102_401 + 1000 * kidx.astype(np.uint64)).astype(np.uint64)
    state = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2], dtype=np.uint8), n)
    for i in np.flatnonzero(rng.random(n) < 0.1).tolist():
        digests[i] = None
    digests[5] = ""  # the C layout's "no checksum"
    state[5] = 0
    return keys, sizes, digests, state


def report_reference(keys, sizes, digests, state, k):
    n = len(keys)
    elig = [state[i] == 0 and bool(digests[i]) for i in range(n)]
    first, rep = {}, np.full(n, NO, dtype=np.uint32)
    for i in range(n):
        if elig[i]:
            rep[i] = first.setdefault((int(keys[i]), digests[i]), i)
    members = {}
    for i in range(n):
        if elig[i]:
            members.setdefault(int(rep[i]), []).append(i)
    copies = np.array([len(members[int(rep[i])]) if elig[i] else 0 for i in range(n)], dtype=np.uint32)
    heads = sorted(members)
    totals = {"rows": sum(elig), "objects": len(heads),
              "total_bytes": int(sum(int(sizes[i]) for i in range(n) if elig[i])),
              "unique_bytes": int(sum(int(sizes[h]) for h in heads)),
              "duplicate_sets": sum(len(members[h]) >= 2 for h in heads),
              "max_copies": max(len(m) for m in members.values()),
              "size_mismatch_rows": 0, "bad_rows": 0}
    dup = sorted((h for h in heads if len(members[h]) >= 2),
                 key=lambda h: (-(len(members[h]) - 1) * int(sizes[h]), h))[:k]
    top_heads = dup + [NO] * (k - len(dup))
    top_waste = [(len(members[h]) - 1) * int(sizes[h]) for h in dup] + [0] * (k - len(dup))
    unconfirmed = sum(1 for i in range(n) if state[i] == 0 and not digests[i])
    return rep, copies, totals, top_heads, top_waste, unconfirmed


@pytest.mark.parametrize("exact_method", [0, 1], ids=["auto", "words"])  # EXACT_AUTO, EXACT_WORDS
def test_host_report(methods, exact_method):
    eng = methods
    keys, sizes, digests, state = report_case()
    k = 50
    want = report_reference(keys, sizes, digests, state, k)
    plain = eng.duplicate_report(keys, sizes, state, k=0)
    eng.set_exact_method(exact_method)
    runs = [eng.duplicate_report_exact(keys, sizes, digests, state, k=k) for _ in range(2)]
    for r in runs:
        assert (r.rep == plain.rep).all() and r.totals == plain.totals
        assert (r.rep_exact == want[0]).all() and (r.copies_exact == want[1]).all()
        assert r.totals_exact == want[2]
        assert r.top_heads.tolist() == want[3] and r.top_waste.tolist() == want[4]
        assert r.unconfirmed == want[5] and want[5] > 0
        inel = (state != 0) | np.array([not d for d in digests])
        assert (r.rep_exact[inel] == NO).all() and (r.copies_exact[inel] == 0).all()
    assert (runs[0].top_heads == runs[1].top_heads).all() and (runs[0].top_waste == runs[1].top_waste).all()
    # a huge k: (NO_OBJECT, 0) past the sets found; state None = every row hashed
    r = eng.duplicate_report_exact(keys, sizes, digests, None, k=2000)
    w = report_reference(keys, sizes, digests, np.zeros(len(keys), dtype=np.uint8), 2000)
    assert (r.rep_exact == w[0]).all() and r.totals_exact == w[2] and r.unconfirmed == w[5]
    assert r.top_heads.tolist() == w[3] and r.top_waste.tolist() == w[4] and w[3][-1] == NO


def test_host_report_empty_and_none_eligible(eng):
    r = eng.duplicate_report_exact([], [], [], None, k=3)
    assert r.top_heads.tolist() == [NO] * 3 and r.totals_exact["rows"] == 0 and r.unconfirmed == 0
    r = eng.duplicate_report_exact([5, 5, 6], [10, 10, 10], [None, "", None], None, k=2)
    assert r.rep.tolist() == [0, 0, 2] and r.rep_exact.tolist() == [NO] * 3
    assert r.unconfirmed == 3 and r.totals_exact["rows"] == 0 and r.totals["objects"] == 2
    assert r.top_heads.tolist() == [NO, NO]


@pytest.mark.parametrize("bad", ["zz" + "0" * 62, "0" * 63, "0" * 40 + " " + "0" * 23],
                         ids=["nonhex", "short", "space"])
def test_host_report_malformed_hex_touches_nothing(eng, bad):
    n, k = 8, 4
    keys = np.arange(1, n + 1, dtype=np.uint64)
    sizes = np.full(n, 1000, dtype=np.uint64)
    hexes = np.zeros(n, dtype="S65")
    hexes[:] = ("ab" * 32).encode()
    hexes[6] = bad.encode()
    state = np.zeros(n, dtype=np.uint8)
    state[6] = 2  # even on a row that takes no part
    outs = [HostFence(np.uint32, n), HostFence(np.uint32, n), HostFence(np.uint32, n),
            HostFence(np.uint64, 8), HostFence(np.uint64, 8), HostFence(np.uint64, 1),
            HostFence(np.uint32, k), HostFence(np.uint64, k), HostFence(np.uint64, 1)]
    rc = eng.L.sd_cas_duplicate_report_exact(
        eng.h, keys.ctypes.data, sizes.ctypes.data, hexes.ctypes.data, state.ctypes.data, n,
        outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, outs[5].ptr, k,
        outs[6].ptr, outs[7].ptr, outs[8].ptr)
    assert rc == -1 and b"row 6" in eng.L.sd_cas_last_error(eng.h)
    for f in outs:
        f.check()
        assert (f.a.view(np.uint8) == 0xC3).all()
    if len(bad) == 64:  # the wrapper hands a 64-char string to the library as it is
        with pytest.raises(CasError) as e:
            eng.duplicate_report_exact(keys, sizes, [h.decode() for h in hexes], state)
        assert e.value.code == -1
