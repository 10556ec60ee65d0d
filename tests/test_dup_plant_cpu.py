"""CPU tests of tests/dup_plant.py, the planner and model behind tests/test_dup_sweep_gpu.py: the
numpy port of the probe against csrc/sd_dup_probe.h itself, crafted probe collisions, expect()
against a brute force over real bytes, and the coverage of the sweep plans the GPU tests use."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dup_plant as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
L = dp.L


def _native_row():
    """The row and size of tests/native/dup_probe_test.cpp."""
    x, row = 0x9E3779B97F4A7C15, np.empty(L, dtype=np.uint8)
    for i in range(L):
        x = dp._mix((x + i) & dp.M64)
        row[i] = x & 0xFF
    return 123456789, row


@pytest.fixture(scope="module")
def native_row():
    return _native_row()


def _probe1(size, row):
    return int(dp.probe_np(np.array([size & dp.M64], dtype=np.uint64), row[None, :dp.EDGE], row[None, dp.TAIL:])[0])


def test_port_reproduces_the_headers_probe(tmp_path, native_row):
    size, row = native_row
    exe = str(tmp_path / "dup_probe_test")
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "dup_probe_test.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"dup_probe ok ([0-9a-f]{16})\n", r.stdout)
    assert m, r.stdout
    assert m.group(1) == "ac30bfb075b63e31"  # (the value the header gave when the port was written)
    assert _probe1(size, row) == int(m.group(1), 16)
    assert dp.probe_states(size, row)[8] == int(m.group(1), 16)


def test_header_constants():
    """The constants dup_plant states are the headers'."""
    runs = open(os.path.join(CSRC, "sd_dup_runs.h")).read()
    probe = open(os.path.join(CSRC, "sd_dup_probe.h")).read()
    ctx = open(os.path.join(CSRC, "ctx_internal.h")).read()

    def const(text, name):
        return int(re.search(rf"\b{name}\s*=\s*(\d+)\b", text).group(1))
    assert int(re.search(r"#define SD_DUP_RUN_K (\d+)\n", runs).group(1)) == dp.RUN_K
    assert const(runs, "DUP_ROW_BYTES") == const(probe, "DUP_PROBE_ROW") == L
    assert const(runs, "DUP_WAVE") == dp.WAVE and const(runs, "DUP_SLICE_QUADS") == dp.SLICE_QUADS
    assert "DUP_SLICE_BYTES = DUP_WAVE * DUP_SLICE_QUADS * 16" in runs
    assert "return s * DUP_SLICE_BYTES + (u * DUP_WAVE + lane) * 16u;" in runs
    assert dp.SLICES * dp.SLICE_BYTES == L and dp.SLICES == 7  # the header's static_assert
    assert const(probe, "DUP_PROBE_EDGE") == dp.EDGE
    assert f"size ^ 0x{dp.PROBE_SEED:X}ull" in probe
    assert const(ctx, "DUPV_MIN_CANDIDATE_SHARE") == dp.MIN_CANDIDATE_SHARE


def test_crafted_rows_collide(native_row):
    size, row = native_row
    p = _probe1(size, row)
    for off in (0, 31, dp.TAIL, dp.LAST_WORD - 1):  # a flipped edge byte
        twin = row.copy()
        twin[off] ^= 0x10
        assert _probe1(size, twin) != p
        dp.collide_last_word(size, row, size, twin)
        assert _probe1(size, twin) == p
        assert not np.array_equal(twin[dp.LAST_WORD:], row[dp.LAST_WORD:])
        assert np.array_equal(np.flatnonzero(twin != row)[:1], [off])
    for delta in (1, 1 << 32, 1 << 63):  # another size
        twin = row.copy()
        assert _probe1(size + delta, twin) != p
        dp.collide_last_word(size, row, size + delta, twin)
        assert _probe1(size + delta, twin) == p and _probe1(size, twin) != p
        assert np.array_equal(twin[:dp.LAST_WORD], row[:dp.LAST_WORD])
    # the vectorised form gives the same words
    twin = row.copy()
    twin[5] ^= 1
    e = lambda r: np.concatenate([r[:dp.EDGE], r[dp.TAIL:]])[None]  # noqa: E731
    words = dp.collide_last_words_np(np.array([size], dtype=np.uint64), e(row),
                                     np.array([size + 7], dtype=np.uint64), e(twin))
    dp.collide_last_word(size, row, size + 7, twin)
    assert np.array_equal(words[0], twin[dp.LAST_WORD:])


def _random_plan(n, seed):
    """Groups with exact copies, interior flips, edge flips, flips shared by two members, size
    deltas and crafted collisions, on shuffled indices."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    plan, at = [], 0
    while at + 9 <= n - 40:  # (some files stay untouched)
        k = int(rng.integers(2, 9))
        members = [int(f) for f in perm[at:at + k]]
        at += k
        o = min(members)
        flips, dsize, collide, last = {}, {}, set(), None
        for f in members:
            if f == o:
                continue
            kind = int(rng.integers(0, 7))
            if kind == 1:    # an interior flip
                last = {int(rng.integers(dp.EDGE, dp.TAIL)): 1 << int(rng.integers(0, 8))}
                flips[f] = dict(last)
            elif kind == 2:  # an edge flip: another probe
                off = int(rng.integers(0, 2 * dp.EDGE))
                flips[f] = {off if off < dp.EDGE else dp.TAIL + off - dp.EDGE: 0x20}
            elif kind == 3 and last is not None:  # the last interior flip again
                flips[f] = dict(last)
            elif kind == 4:  # another size
                dsize[f] = int(rng.choice([1, 1 << 32, 1 << 63]))
            elif kind == 5:  # a crafted collision: an edge flip or a size
                if rng.integers(0, 2):
                    off = int(rng.integers(0, 2 * dp.EDGE - 8))
                    flips[f] = {off if off < dp.EDGE else dp.TAIL + off - dp.EDGE: 0x04}
                else:
                    dsize[f] = 1 << int(rng.integers(0, 64))
                collide.add(f)
            elif kind == 6:  # an edge flip shared with the next such member of the group
                flips[f] = {3: 0x80, 40_000: 0x01}
        plan.append(dp.Group(members, flips, dsize, collide))
    return plan


def test_expect_agrees_with_brute_force():
    n = 300
    rng = np.random.default_rng(2)
    content = rng.integers(0, 256, (n, L), dtype=np.uint8)
    sizes = rng.integers(102_401, 1 << 40, n, dtype=np.uint64)
    plan = _random_plan(n, 3)
    assert sum(len(g.collide) for g in plan) >= 10 and sum(len(g.dsize) for g in plan) >= 10
    dp.apply_np(plan, content, sizes)
    want = dp.expect(plan, n)
    probes = dp.probe_np(sizes, content[:, :dp.EDGE], content[:, dp.TAIL:])
    first = {}
    cand = np.array([first.setdefault(int(p), f) for f, p in enumerate(probes)])
    same = lambda a, b: sizes[a] == sizes[b] and np.array_equal(content[a], content[b])  # noqa: E731
    is_cand = cand != np.arange(n)
    verified = np.array([is_cand[f] and same(f, cand[f]) for f in range(n)])
    rep = np.array([next(g for g in range(f + 1) if same(f, g)) for f in range(n)])
    assert np.array_equal(cand, want.cand)
    assert (int(is_cand.sum()), int(verified.sum()), int((is_cand & ~verified).sum())) == want.counters
    assert want.candidates > want.verified > 0 and want.rehashed > 0
    assert np.array_equal(rep, want.rep)
    assert len(np.unique(cand[is_cand])) == want.groups
    assert len(np.unique(rep)) == want.objects
    assert np.array_equal(want.planted, np.unique(np.concatenate([g.members for g in plan])))


def _flips(plan):
    out = []
    for g in plan:
        assert len(g.members) == 2 and list(g.flips) == [max(g.members)]
        (off, mask), = g.flips[max(g.members)].items()
        out.append((off, mask))
    return out


def test_sweep_plans_cover_every_class():
    quantum = 65_536
    assert [q for q, _, _ in dp.SWEEPS.values()] == [1, 1, 2]
    narrow = _flips(dp.sweep_case("narrow-lo", quantum)) + _flips(dp.sweep_case("narrow-hi", quantum))
    wide = _flips(dp.sweep_case("wide", quantum))
    for flips in (narrow, wide):  # each kernel shape sees every offset exactly once
        offs = np.array([o for o, _ in flips])
        assert np.array_equal(np.sort(offs), np.arange(L))
        assert all(m == dp.sweep_bit(o) and bin(m).count("1") == 1 for o, m in flips)
        classes = {dp.locate(o) for o in offs}
        assert classes == {(s, u, lane, w, b) for s in range(dp.SLICES) for u in range(dp.SLICE_QUADS)
                           for lane in range(dp.WAVE) for w in range(4) for b in range(4)}
        # locate() inverts the header's dup_slice_quad_offset
        assert all(o == s * dp.SLICE_BYTES + (u * dp.WAVE + lane) * 16 + 4 * w + b
                   for o, (s, u, lane, w, b) in ((o, dp.locate(o)) for o in offs[::97]))
        bits = {(o % 16, m) for o, m in flips}
        assert bits == {(b, 1 << k) for b in range(16) for k in range(8)}
    # both members of a pair at shuffled indices, no file in two pairs
    plan = dp.sweep_case("narrow-lo", quantum)
    members = np.array([g.members for g in plan])
    assert len(np.unique(members)) == members.size == L
    assert (np.diff(members[:, 0]) < 0).any() and members.max() > quantum - 100
    e = dp.expect(plan, quantum)
    edge = sum(dp.in_probe_edge(o) for o in dp.SWEEPS["narrow-lo"][1])
    assert edge == dp.EDGE and e.counters == (L // 2 - edge, 0, L // 2 - edge)
    assert e.objects == quantum and np.array_equal(e.rep, np.arange(quantum))
