"""GPU tests of the exact duplicate sets by comparison: sd_cas_group_exact_contents_dev (a
grouping split by comparing whole contents where they lie), its round cap and counters, and
CasEngine.exact_duplicates_compared over real files.  The reference answer is computed from the
bytes in tests/exact_compare_cases.py (a dict keyed by rep value, length and bytes); the
expected rounds and counters come from that module's model of the rounds, which
tests/test_exact_compare_cpu.py holds to the reference.  Every input sits in a DevInput fence
and every output in a DevFence: after each call the inputs equal their snapshots and the
guards are intact.  Boundaries are placed from the library's own constants."""
import ctypes
import os

import numpy as np
import pytest

import spacedrive_amd as sa
from spacedrive_amd import CasError
from tests import exact_compare_cases as cases
from tests.fence import DevFence, DevInput, check_all

pytestmark = pytest.mark.gpu

NO = sa.NO_OBJECT
SLICE, PIECE, RUN_K, DEFAULT_ROUNDS = cases.constants()


@pytest.fixture
def rounds(eng):
    """Leaves the shared engine on its default cap whatever a test set."""
    yield eng
    eng.set_exact_compare_rounds(None)


class Packed:
    """A case on the device, fenced: arena, offs, lens, rep."""

    def __init__(self, rep, blobs, seed=1, tail=0, arena=None):
        self.n = len(blobs)
        if arena is None:
            arena = cases.pack(blobs, seed, tail)
        self.h_arena, self.h_offs, self.h_lens = arena
        self.arena = DevInput(self.h_arena, guard=0xA5)
        # a guard offset / length far outside any arena: a read past the arrays breaks the bounds
        self.offs = DevInput(self.h_offs, guard=1 << 40)
        self.lens = DevInput(self.h_lens, guard=1 << 40)
        self.rep = DevInput(np.ascontiguousarray(rep, dtype=np.uint32), guard=int(rep[0]) if self.n else 0)
        self.arena_bytes = len(self.h_arena)

    def call(self, eng, fill=0xC3):
        out = DevFence(np.uint32, self.n, fill=fill)
        objects = eng.group_exact_contents(self.rep.t, self.arena.t, self.offs.t, self.lens.t, out.t,
                                           arena_bytes=self.arena_bytes)
        check_all(out, self.arena, self.offs, self.lens, self.rep)
        return out.host(), objects, eng.exact_compare_counters()


def agree(got, want):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


def test_lengths_and_positions(rounds):
    """{P, an equal copy, a copy differing in one byte} at every length around a quad, a slice
    and a piece, the byte at both ends and on both sides of every slice and piece boundary; the
    padding of every row holds different garbage, and the equal copy is still equal."""
    eng = rounds
    rep, blobs, cs = cases.lengths_case(SLICE, PIECE)
    want = cases.reference(rep, blobs)
    case = Packed(rep, blobs)
    pad = [int(o + ln) for o, ln in zip(case.h_offs, case.h_lens) if ln % 16]
    assert len({bytes(case.h_arena[a:a + 16]) for a in pad}) == len(pad)  # no two paddings alike
    eng.set_exact_compare_rounds(0)
    got, objects, counters = case.call(eng)
    agree(got, want)
    assert objects == 2 * len(cs) and counters == (1, 2 * len(cs), len(cs), 0)


def test_byte_sweep(rounds):
    eng = rounds
    rep, blobs = cases.sweep_case()
    want = cases.reference(rep, blobs)
    got, objects, counters = Packed(rep, blobs).call(eng)
    agree(got, want)
    assert objects == 2 * 4101 + 1
    assert counters[0] == 1 and counters[2] == 4101 and counters == (1, 4102, 4101, 0)


def test_several_contents_per_class(rounds):
    eng = rounds
    rep, blobs = cases.abc_case()
    eng.set_exact_compare_rounds(0)
    got, objects, counters = Packed(rep, blobs).call(eng)
    assert got.tolist() == [0, 1, 0, 3, 1, 0, 3, 3] and objects == 3
    assert counters[0] in (2, 3) and counters == cases.model_rounds(rep, blobs, 0)[1:]


def test_classes_runs_and_the_cap(rounds):
    """Classes of 1, 2, K - 1, K, K + 1 and 2 K + 1 copies with the unequal copy first, last and
    in the middle, two interleaved classes and 40 pairwise-distinct rows, in one call, under
    every cap: the same answer, the model's counters."""
    eng = rounds
    rep, blobs = cases.classes_case(RUN_K, SLICE)
    want = cases.reference(rep, blobs)
    case = Packed(rep, blobs)
    seen = {}
    for cap in (0, 1, 2, None):
        eng.set_exact_compare_rounds(cap)
        got, objects, counters = case.call(eng)
        agree(got, want)
        assert objects == int((want == np.arange(len(want))).sum())
        assert counters == cases.model_rounds(rep, blobs, DEFAULT_ROUNDS if cap is None else cap)[1:]
        seen[cap] = counters
    assert seen[0][0] == 39 and seen[0][3] == 0 and seen[1][3] > 0 and seen[None][0] == DEFAULT_ROUNDS


def test_rep_is_a_value(rounds):
    eng = rounds
    rng = np.random.default_rng(31)
    pool = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (700, 700, 9000, 9000, 70_000)]
    labels = np.array([0xFFFFFFFF, 0xFFFFFFFE, 1 << 31, 5000, 77, 0], dtype=np.uint32)
    n = 600
    rep = labels[rng.integers(0, len(labels), n)]
    blobs = [pool[j] for j in rng.integers(0, len(pool), n)]
    want = cases.reference(rep, blobs)
    assert (rep >= n).any() and (want != np.arange(n)).any()
    got, objects, _ = Packed(rep, blobs).call(eng)
    agree(got, want)
    # a rep that is not canonical (rows 1.. carry row 3, not row 0) gives the canonical partition
    a, b = pool[0], pool[1]
    got, objects, _ = Packed(np.full(6, 3, dtype=np.uint32), [a, b, a, a, b, b]).call(eng)
    assert got.tolist() == [0, 1, 0, 0, 1, 1] and objects == 2
    # two lengths inside one rep split without a compare
    got, objects, counters = Packed(np.full(4, 8, dtype=np.uint32), [a, pool[2], a[:699], pool[2][:-1]]).call(eng)
    assert got.tolist() == [0, 1, 2, 3] and objects == 4 and counters == (0, 0, 0, 0)
    # length-0 rows of one rep are one Object; their offset lies in the arena's last 16 bytes
    blobs = [a, b"", b"", a, b""]
    arena, offs, lens = cases.pack(blobs, tail=16)
    offs[[1, 2, 4]] = len(arena) - 16
    got, objects, counters = Packed(np.full(5, 2, dtype=np.uint32), blobs, arena=(arena, offs, lens)).call(eng)
    assert got.tolist() == [0, 1, 1, 0, 1] and objects == 2 and counters == (1, 3, 0, 0)


def test_small_n(rounds):
    import torch
    eng = rounds
    e32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    e64 = torch.zeros(0, dtype=torch.int64, device="cuda")
    arena = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert eng.group_exact_contents(e32, arena, e64, e64, e32.clone()) == 0
    assert eng.exact_compare_counters() == (0, 0, 0, 0)
    d_obj = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    assert eng.L.sd_cas_copy_objects_dev(eng.h, d_obj.data_ptr(), int(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert int(d_obj.item()) == 0
    got, objects, counters = Packed(np.array([7], dtype=np.uint32), [b"x" * 33]).call(eng)
    assert got.tolist() == [0] and objects == 1 and counters == (0, 0, 0, 0)
    rng = np.random.default_rng(32)
    blobs = [rng.integers(0, 256, 100, dtype=np.uint8).tobytes()] * 1000
    got, objects, counters = Packed(np.arange(1000, dtype=np.uint32)[::-1].copy(), blobs).call(eng)
    assert (got == np.arange(1000)).all() and objects == 1000 and counters[0] == 0
    assert eng.L.sd_cas_copy_objects_dev(eng.h, d_obj.data_ptr(), int(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert int(d_obj.item()) == 1000


def test_refusals(rounds):
    import torch
    eng = rounds
    rng = np.random.default_rng(33)
    a = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    rep, blobs = np.zeros(4, dtype=np.uint32), [a, a, a[:100], a]
    case = Packed(rep, blobs)
    n = case.n
    out = DevFence(np.uint32, n)
    stream = int(torch.cuda.current_stream().cuda_stream)
    obj = ctypes.c_uint64(77)

    def call(rep_p, arena_p, ab, offs_p, lens_p, nn, out_p):
        return eng.L.sd_cas_group_exact_contents_dev(eng.h, rep_p, arena_p, ab, offs_p, lens_p, nn, out_p,
                                                     ctypes.byref(obj), stream)
    good = (case.rep.ptr, case.arena.ptr, case.arena_bytes, case.offs.ptr, case.lens.ptr, n, out.ptr)
    # a content ending past arena_bytes
    assert call(*good[:2], int(case.h_offs[3] + case.h_lens[3]) - 1, *good[3:]) == -1
    assert b"arena_bytes" in eng.L.sd_cas_last_error(eng.h)
    # an offset that is not 16-B aligned; a length over 64 GiB
    for arr, row, val in ((case.h_offs, 1, int(case.h_offs[1]) + 8), (case.h_lens, 2, (64 << 30) + 1)):
        bad = arr.copy()
        bad[row] = val
        d_bad = DevInput(bad, guard=0)
        args = list(good)
        args[3 if arr is case.h_offs else 4] = d_bad.ptr
        assert call(*args) == -1
        d_bad.unchanged()
    with pytest.raises(CasError) as e:
        eng.group_exact_contents(case.rep.t, case.arena.t, case.offs.t, case.lens.t, out.t, arena_bytes=4096)
    assert e.value.code == -1
    # null arrays, too many rows, an output overlapping rep
    for k in (0, 3, 4, 6):
        args = list(good)
        args[k] = None
        assert call(*args) == -1
    assert call(*good[:5], (1 << 24) + 1, out.ptr) == -1
    assert call(*good[:6], case.rep.ptr) == -1 and call(*good[:6], case.rep.ptr + 4 * (n - 1)) == -1
    assert call(out.ptr + 4, *good[1:5], n - 1, out.ptr) == -1
    torch.cuda.synchronize()
    assert obj.value == 77 and (out.host().view(np.uint8) == 0xC3).all()
    check_all(out, case.arena, case.offs, case.lens, case.rep)
    # a valid call afterwards is correct
    got, objects, _ = case.call(eng)
    assert got.tolist() == [0, 0, 2, 0] and objects == 2


def test_random(rounds):
    """6,000 rows: fresh contents, equal copies and one-byte-changed copies (the conditions on
    the reference are checked without a GPU, tests/test_exact_compare_cpu.py); against the numpy
    reference and against checksums_dev + group_exact over the same arena."""
    import torch
    eng = rounds
    rep, blobs = cases.random_case()
    want = cases.reference(rep, blobs)
    case = Packed(rep, blobs)
    got, objects, counters = case.call(eng)
    agree(got, want)
    assert objects == int((want == np.arange(case.n)).sum())
    assert counters == cases.model_rounds(rep, blobs, DEFAULT_ROUNDS)[1:]
    dig = torch.empty(case.n * 32, dtype=torch.uint8, device="cuda")
    by_digest = torch.empty(case.n, dtype=torch.int32, device="cuda")
    eng.checksums_dev(case.arena.t, case.offs.t, case.lens.t, dig, arena_bytes=case.arena_bytes)
    assert eng.group_exact(case.rep.t, dig, by_digest) == objects
    agree(got, by_digest.cpu().numpy().view(np.uint32))
    eng.set_exact_compare_rounds(1)
    capped, objects1, counters1 = case.call(eng)
    agree(capped, want)
    assert objects1 == objects and counters1 == cases.model_rounds(rep, blobs, 1)[1:] and counters1[3] > 0


# ---- files ---------------------------------------------------------------------------------
NAMES = ["f0_A", "f1_B1", "f2_B2", "f3_C", "f4_X", "f5_D", "f6_E", "f7_U", "f8_missing"]


@pytest.fixture(scope="module")
def file_set(tmp_path_factory):
    """A, 300,000 random bytes; A with the unsampled bytes 18,432 and 291,807 flipped; a copy of A;
    A with the sampled byte 18,431 flipped; two equal 50,000-byte files; one unrelated file; one
    path that does not exist."""
    d = tmp_path_factory.mktemp("compared_files")
    rng = np.random.default_rng(42)
    a = rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    small = rng.integers(0, 256, 50_000, dtype=np.uint8).tobytes()
    other = rng.integers(0, 256, 120_000, dtype=np.uint8).tobytes()
    blobs = [a, cases.flipped(a, 18_432), cases.flipped(a, 291_807), a, cases.flipped(a, 18_431), small, small, other]
    for name, blob in zip(NAMES, blobs):
        (d / name).write_bytes(blob)
    return [str(d / name) for name in NAMES]


def same_report(a, b):
    for f in ("rep", "rep_exact", "copies_exact", "top_heads", "top_waste"):
        assert (getattr(a, f) == getattr(b, f)).all(), f
    assert a.totals == b.totals and a.totals_exact == b.totals_exact and a.unconfirmed == b.unconfirmed


def test_files(eng, file_set):
    paths = file_set
    want = eng.exact_duplicates(paths, k=3)
    assert want.rep_exact.tolist() == [0, 1, 2, 0, 4, 5, 5, 7, NO]
    got = eng.exact_duplicates_compared(paths, k=3)
    same_report(got, want)
    assert (got.candidate_rows, got.candidate_bytes, got.compared_rows, got.checksum_rows) == (6, 1_300_000, 6, 0)
    # the set of A does not fit: its four rows take the checksum route, the report is unchanged
    small = eng.exact_duplicates_compared(paths, k=3, arena_bytes=700_000)
    same_report(small, want)
    assert (small.candidate_rows, small.compared_rows, small.checksum_rows) == (6, 2, 4)
    assert eng.exact_duplicates_compared([], k=2).top_heads.tolist() == [NO, NO]


def test_files_changed_since_the_stat(eng, file_set, tmp_path, monkeypatch):
    """A candidate that can no longer be read is unconfirmed and counted nowhere else."""
    paths = list(file_set[:4])
    real = eng.file_metadata_from_paths

    def stat_then_lose(ps):
        out = real(ps)
        os.rename(paths[3], str(tmp_path / "gone"))
        return out
    monkeypatch.setattr(eng, "file_metadata_from_paths", stat_then_lose)
    try:
        got = eng.exact_duplicates_compared(paths, k=1)
    finally:
        os.rename(str(tmp_path / "gone"), paths[3])
    assert got.rep.tolist() == [0, 0, 0, 0] and got.rep_exact.tolist() == [0, 1, 2, NO]
    assert got.copies_exact.tolist() == [1, 1, 1, 0] and got.unconfirmed == 1
    assert got.totals_exact["rows"] == 3 and got.top_heads.tolist() == [NO]
