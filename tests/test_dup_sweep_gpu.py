"""GPU tests that sweep the fused chain's duplicate comparison (dup_verify.hip K1V: dup_compare_task,
dup_slices_differ, dup_load_slice, sd_cas_dup_finish_kernel) over every byte of a row and over
the shapes of its compare tasks.  A wrong "same" verdict merges two files into one Object and
nothing faults, so every case plants its near misses with tests/dup_plant.py and asserts what
that module's model says from the plan alone: the (candidates, verified, rehashed) counters, the
whole of rep, which keys are equal, and the oracle's keys on the planted files.  One batch quantum
launches the 256-lane mixed kernel, two quanta the 512-lane one; nothing here is larger."""
import numpy as np
import pytest
import torch

from tests import dup_plant as dp

pytestmark = pytest.mark.gpu

L = dp.L


@pytest.fixture(scope="module")
def base(eng):
    """One quantum of distinct files (never modified: the cases edit clones)."""
    n = eng.batch_quantum
    content = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(0xD0B1E, 0, n, content, sizes, L, dup_permille=0)
    torch.cuda.synchronize()
    return content, sizes


@pytest.fixture(autouse=True)
def _verify_on(eng):
    eng.set_dup_verify(True)
    yield
    eng.set_dup_verify(True)


def _batch(eng, base, quanta, seed, stride=L):
    """(content, sizes) to edit: a clone of base, or fresh distinct files of another shape."""
    if quanta == 1 and stride == L:
        return base[0].clone(), base[1].clone()
    n = quanta * eng.batch_quantum
    if stride == L:
        content = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    else:  # random padding after every row, which no copy below touches
        content = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(seed, 0, n, content, sizes, stride, dup_permille=0)
    return content, sizes


def _probed(eng, c, z):
    eng.set_dup_verify(True)  # this call probes, whatever earlier batches held
    return dp.fused(eng, c, z)


def _assert_oracle(oracle, c, z, got, idx):
    idx = np.unique(np.asarray(idx, dtype=np.int64))
    want = dp.oracle_keys(oracle, c, z, idx)
    bad = idx[got[idx] != want]
    assert bad.size == 0, f"{bad.size} of {idx.size} keys differ from the oracle's, files {bad[:8]}"


def _assert_classes(e, got, rep, objects):
    """rep is expect's, and the keys agree or differ exactly along its classes, over all n."""
    r = rep.cpu().numpy()
    bad = np.flatnonzero(r != e.rep)
    assert bad.size == 0, f"rep differs at {bad.size} files: {[(int(f), int(r[f]), int(e.rep[f])) for f in bad[:8]]}"
    assert (got == got[e.rep]).all()
    assert len(np.unique(got)) == e.objects == objects


@pytest.mark.parametrize("case", list(dp.SWEEPS))
def test_every_byte_offset(eng, oracle, base, case):
    """One pair per byte offset, the copy one bit apart there (tests/test_dup_plant_cpu.py: each
    kernel shape meets every (slice, quad, lane, word, byte) of a compare task's loads once, and
    every bit at every byte of a quad).  An interior pair is a candidate that must be refuted;
    a pair that differs in the probe's bytes [0, 32) or [57,312, 57,344) is no candidate at all."""
    quanta, offsets, seed = dp.SWEEPS[case]
    c, z = _batch(eng, base, quanta, seed)
    try:
        n = int(z.numel())
        plan = dp.sweep_case(case, eng.batch_quantum)
        e = dp.expect(plan, n)
        edge = sum(dp.in_probe_edge(o) for o in offsets)
        assert e.counters == (len(offsets) - edge, 0, len(offsets) - edge) and edge in (32, 64)
        dp.apply(plan, c, z)
        keys, rep, objects, counters = _probed(eng, c, z)
        got = keys.cpu().numpy().view(np.uint64)
        orig = np.array([g.original for g in plan])
        copy = np.array([max(g.members) for g in plan])
        offs = np.array(list(offsets))
        merged = got[copy] == got[orig]
        wrong_rep = rep.cpu().numpy()[copy] != copy
        for off in offs[merged | wrong_rep][:64]:
            print("taken for a copy:", dp.describe(int(off)))
        print(f"{case}: counters {counters}, expected {e.counters}; {int(merged.sum())} pairs share a key")
        assert counters == e.counters
        assert objects == n
        assert torch.equal(rep, torch.arange(n, dtype=torch.int32, device="cuda"))
        assert not merged.any()
        sel = offs % 28 == 0
        free = np.setdiff1d(np.arange(n), e.planted)
        untouched = np.random.default_rng(seed).choice(free, 256, replace=False)
        _assert_oracle(oracle, c, z, got, np.concatenate([orig[sel], copy[sel], untouched]))
    finally:
        del c, z
        torch.cuda.empty_cache()


def test_probe_collisions_are_refuted(eng, oracle, base):
    """True 64-bit probe collisions between different probe inputs (dup_plant.collide_last_word):
    a pair per edge offset that differs in one bit there and in the crafted last word, and 64 pairs
    of equal bytes up to the crafted word whose sizes differ by 1, 2^32 or 2^63; beside 2,048 exact
    copies.  Every crafted pair is a candidate, none is verified, and each file keeps its own key.

    No test can isolate the sizes[f] == sizes[g] term of dup_compare_task: two files of equal
    content and different sizes cannot have equal probes, because every step of the probe's chain
    is a bijection of its state, so the size's difference survives to the end unless a later word
    differs too — and then the bytes refute the pair as well."""
    c, z = _batch(eng, base, 1, 0)
    n = int(z.numel())
    perm = np.random.default_rng(21).permutation(n)
    pairs = iter(perm[:2 * 4096].reshape(-1, 2))
    plan, crafted = [], []
    edge_offs = list(range(0, dp.EDGE)) + list(range(dp.TAIL, dp.LAST_WORD))
    for off in edge_offs:
        a, b = sorted(int(f) for f in next(pairs))
        plan.append(dp.Group([a, b], flips={b: {off: dp.sweep_bit(off)}}, collide={b}))
        crafted.append((a, b))
    for i in range(64):
        a, b = sorted(int(f) for f in next(pairs))
        plan.append(dp.Group([a, b], dsize={b: (1, 1 << 32, 1 << 63)[i % 3]}, collide={b}))
        crafted.append((a, b))
    for _ in range(2048):
        plan.append(dp.Group([int(f) for f in next(pairs)]))
    e = dp.expect(plan, n)
    assert len(crafted) == 56 + 64 and e.counters == (len(crafted) + 2048, 2048, len(crafted))
    dp.apply(plan, c, z)
    keys, rep, objects, counters = _probed(eng, c, z)
    got = keys.cpu().numpy().view(np.uint64)
    for (a, b), off in zip(crafted, edge_offs):
        if got[a] == got[b]:
            print("collision taken for a copy:", dp.describe(off))
    assert counters == e.counters
    assert eng.dup_verify_rows()[0] == e.groups == len(plan)
    _assert_classes(e, got, rep, objects)
    crafted = np.array(crafted)
    assert (got[crafted[:, 0]] != got[crafted[:, 1]]).all()
    exact = np.array([g.members for g in plan[len(crafted):len(crafted) + 128]])
    _assert_oracle(oracle, c, z, got, np.concatenate([crafted.ravel(), exact.ravel()]))


def _matrix_plan(n, seed, groups=3000):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    plan, at = [], 0
    for _ in range(groups):
        k = int(rng.integers(1, 41))
        if at + k + 1 > n:
            break
        members = [int(f) for f in perm[at:at + k + 1]]
        at += k + 1
        o, flips, last = min(members), {}, None
        for f in members:
            if f == o or rng.random() < 0.4:
                continue  # the original, or an exact copy
            if last is None or rng.random() >= 0.1:
                last = {int(rng.integers(dp.EDGE, dp.TAIL)): 1 << int(rng.integers(0, 8))}
            flips[f] = dict(last)  # (with probability 0.1 the group's previous near miss again)
        plan.append(dp.Group(members, flips))
    return plan


@pytest.mark.parametrize("case", ["narrow", "wide", "padded"])
def test_verdict_matrix(eng, oracle, base, case):
    """About 3,000 groups of 1..40 copies at shuffled indices, each copy exact with probability
    0.4 and otherwise one bit apart at a uniform interior offset; one near miss in ten repeats
    its group's previous one, and those two share rep and key though both are rehashed.  The
    compare windows hold several originals and every mix of verdicts."""
    quanta, stride = {"narrow": (1, L), "wide": (2, L), "padded": (1, 57_360)}[case]
    c, z = _batch(eng, base, quanta, 41, stride)
    try:
        n = int(z.numel())
        plan = _matrix_plan(n, {"narrow": 31, "wide": 32, "padded": 33}[case])
        assert len(plan) >= 2_900
        e = dp.expect(plan, n)
        assert e.verified > 10_000 and e.rehashed > 10_000 and e.objects < n - e.verified
        dp.apply(plan, c, z)
        if stride != L:
            g = plan[0]
            m = torch.tensor(g.members, device="cuda")
            assert len(torch.unique(c[m, L:], dim=0)) == len(g.members)  # the padding differs
        keys, rep, objects, counters = _probed(eng, c, z)
        print(f"{case}: {len(plan)} groups, counters {counters}, expected {e.counters}")
        assert counters == e.counters
        assert eng.dup_verify_rows()[0] == e.groups
        got = keys.cpu().numpy().view(np.uint64)
        _assert_classes(e, got, rep, objects)
        picked = np.random.default_rng(5).choice(len(plan), 200, replace=False)
        edited = np.concatenate([plan[i].members for i in picked])
        _assert_oracle(oracle, c, z, got, edited)
        dp.check(eng, oracle, c, z, keys, rep, objects)
    finally:
        del c, z
        torch.cuda.empty_cache()


def test_windows_of_singles(eng, oracle, base):
    """4,097 groups of one copy.  List C's order is then known: first[] is the scan of cnt over
    the file index and every rank is 0, so C[p] is the copy of the p-th smallest original, task w
    compares C[16 w, 16 w + 16) and wave v of the finish kernel finishes C[64 v, 64 v + 64).
    Near misses at chosen p: run heads refuted early (slice 0, odd p) and late (slice 6, even p),
    windows refuted whole (100, 101, 104..107), the hand-over to the next entry after a
    refutation and a reference reload at every entry (200..210, alternating), finish waves where
    only lane 0 (p = 64, 256) or only lane 63 (p = 255) failed, a wave that failed whole (104..107
    are wave 26; 100 and 101 alone are half of wave 25), and a last finish block whose single
    live lane (p = 4,096) is rehashed."""
    c, z = _batch(eng, base, 1, 0)
    n = int(z.numel())
    k = 4_097
    rng = np.random.default_rng(61)
    origs = np.sort(rng.choice(n // 2, k, replace=False))
    copies = n // 2 + rng.choice(n // 2, k, replace=False)  # (shuffled: C's order is the originals')
    K = dp.RUN_K
    near = {0, 15, 16, 17, 31, 32, 63, 64, 255, 256, 4096}
    near |= set(range(100 * K, 102 * K)) | set(range(104 * K, 108 * K)) | set(range(200 * K, 211 * K, 2))
    assert K == 16 and 104 * K % 64 == 0 and max(near) == k - 1
    plan = []
    for p in range(k):
        flips = {}
        if p in near:
            off = (6 * dp.SLICE_BYTES if p % 2 == 0 else dp.EDGE) + p * 37 % (dp.SLICE_BYTES - dp.EDGE)
            assert dp.EDGE <= off < dp.TAIL and dp.locate(off)[0] == (6 if p % 2 == 0 else 0)
            flips = {int(copies[p]): {off: dp.sweep_bit(off)}}
        plan.append(dp.Group([int(origs[p]), int(copies[p])], flips))
    e = dp.expect(plan, n)
    assert e.counters == (k, k - len(near), len(near)) and e.groups == k
    dp.apply(plan, c, z)
    keys, rep, objects, counters = _probed(eng, c, z)
    got = keys.cpu().numpy().view(np.uint64)
    wrong = [p for p in range(k) if (got[copies[p]] == got[origs[p]]) != (p not in near)]
    print(f"windows: counters {counters}, expected {e.counters}; wrong verdicts at C positions {wrong[:32]}")
    assert counters == e.counters
    groups, tasks, refs = eng.dup_verify_rows()
    assert groups == k and tasks == (k + K - 1) // K
    assert not wrong
    _assert_classes(e, got, rep, objects)
    _assert_oracle(oracle, c, z, got, e.planted)


def test_pause_threshold_boundary(eng, base):
    """A probed batch with n / 32 candidates leaves the next call probing; one candidate fewer
    pauses it (ctx_internal.h DUPV_MIN_CANDIDATE_SHARE), with the same keys, rep and objects."""
    n = eng.batch_quantum
    k = n // dp.MIN_CANDIDATE_SHARE
    pairs = np.random.default_rng(71).permutation(n)[:2 * k].reshape(-1, 2)
    for cands, pauses in ((k, False), (k - 1, True)):
        c, z = _batch(eng, base, 1, 0)
        plan = [dp.Group([int(a), int(b)]) for a, b in pairs[:cands]]
        e = dp.expect(plan, n)
        assert e.counters == (cands, cands, 0) and cands * dp.MIN_CANDIDATE_SHARE - n in (0, -dp.MIN_CANDIDATE_SHARE)
        dp.apply(plan, c, z)
        first = _probed(eng, c, z)
        assert first[3] == e.counters and first[2] == n - cands
        assert np.array_equal(first[1].cpu().numpy(), e.rep)
        keys, rep, objects, counters = dp.fused(eng, c, z)  # (no setter: the last batch's note decides)
        assert counters == ((0, 0, 0) if pauses else e.counters)
        assert torch.equal(keys, first[0]) and torch.equal(rep, first[1]) and objects == first[2]
        del c, z
