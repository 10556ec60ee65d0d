"""GPU tests of the fused chain's grouped duplicate verification (dup_verify.hip K1V: candidates
ordered by their original, compare tasks that read an original once per run of its copies).
Every case checks the keys against the oracle on a sample that holds every edited file, rep and
the Object count against the standalone grouping, and the exact (candidates, verified, rehashed)
counters.  Every case is one batch quantum unless its name says otherwise."""
import time

import numpy as np
import pytest
import torch

from oracle.pyoracle import SAMPLED_CONTENT_LEN

pytestmark = pytest.mark.gpu

L = SAMPLED_CONTENT_LEN
SAMPLE = 2048
SLICE = 8192


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


def _fused(eng, content, sizes):
    n = int(sizes.numel())
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    rep = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    objects = eng.hash_group_sampled(content, sizes, keys, rep, ovf)
    return keys, rep, objects, eng.dup_verify_counters()


def _check(eng, oracle, content, sizes, keys, rep, objects, edited=()):
    n = int(sizes.numel())
    rng = np.random.default_rng(n + len(edited))
    idx = np.unique(np.concatenate([np.asarray(edited, dtype=np.int64), rng.integers(0, n, SAMPLE + 256)]))
    assert len(idx) >= SAMPLE
    host = content[torch.from_numpy(idx).cuda()][:, :L].contiguous().cpu().numpy()
    hs = sizes.cpu().numpy().view(np.uint64)[idx]
    want = oracle.cas_keys_strided(host.reshape(-1), L, L, hs)
    got = keys.cpu().numpy().view(np.uint64)
    assert (got[idx] == want).all()
    rep2 = torch.empty(n, dtype=torch.int32, device="cuda")
    assert eng.group(keys, rep2) == objects
    assert torch.equal(rep, rep2)
    return got


def _copy(c, z, dst, src):
    c[dst] = c[src]
    z[dst] = z[src]


def test_one_group_mixed_verdicts_every_slice(eng, oracle, base):
    """One original with 21 copies scattered over the batch: 7 exact, and 14 that differ in one
    byte, at the first and at the last byte of each 8-KiB slice (inside [32, 57,312), so the
    probes stay equal), exact ones and near misses interleaved in index order."""
    content, sizes = base
    c, z = content.clone(), sizes.clone()
    offs = []
    for s in range(7):
        offs += [max(s * SLICE, 32), min((s + 1) * SLICE - 1, 57_311)]
    assert offs[:4] == [32, 8_191, 8_192, 16_383] and offs[-2:] == [49_152, 57_311]
    o = 1_234
    spots = [3_001 + 2_903 * i for i in range(21)]
    assert spots[-1] < int(z.numel())
    exact, near = [], []
    for i, f in enumerate(spots):
        _copy(c, z, f, o)
        if i % 3 == 1:
            exact.append(f)
        else:
            c[f, offs[len(near)]] ^= 0x01
            near.append(f)
    assert len(exact) == 7 and len(near) == 14
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (21, 7, 14)
    got = _check(eng, oracle, c, z, keys, rep, objects, edited=[o] + spots)
    assert all(got[f] == got[o] for f in exact)
    assert all(got[f] != got[o] for f in near)
    assert objects == int(z.numel()) - 7


@pytest.fixture(scope="module")
def run_lengths(base):
    """Groups of 1, 2, ..., 70 copies (2,485 candidates), originals and copies at shuffled
    indices: every task boundary for any task width up to 64."""
    content, sizes = base
    n = int(sizes.numel())
    c, z = content.clone(), sizes.clone()
    perm = np.random.default_rng(70).permutation(n)
    src, dst, at = [], [], 0
    for k in range(1, 71):  # k + 1 identical files: the smallest is hashed, k are candidates
        src += [perm[at]] * k
        dst += list(perm[at + 1:at + 1 + k])
        at += k + 1
    assert len(dst) == 2_485
    c[torch.from_numpy(np.asarray(dst)).cuda()] = c[torch.from_numpy(np.asarray(src)).cuda()]
    z[torch.from_numpy(np.asarray(dst)).cuda()] = z[torch.from_numpy(np.asarray(src)).cuda()]
    torch.cuda.synchronize()
    return c, z, perm[:at].copy(), len(dst)


def test_every_run_length(eng, oracle, run_lengths):
    c, z, members, cands = run_lengths
    assert cands == 2_485 and len(members) == 2_555
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (cands, cands, 0)
    assert objects == int(z.numel()) - cands
    groups, tasks, refs = eng.dup_verify_rows()
    assert groups == 70 and tasks >= 1 and groups <= refs < groups + tasks
    _check(eng, oracle, c, z, keys, rep, objects, edited=members)


@pytest.mark.parametrize("order", ["o<f1<f2<f3", "o<f3<f1<f2"])
def test_refuted_copy_is_never_a_reference(eng, oracle, base, order):
    """f1 is a near miss of o, f2 is byte-identical to f1, f3 is byte-identical to o."""
    content, sizes = base
    c, z = content.clone(), sizes.clone()
    o = 500
    f1, f2, f3 = (9_000, 31_000, 60_000) if order == "o<f1<f2<f3" else (31_000, 60_000, 9_000)
    for f in (f1, f2, f3):
        _copy(c, z, f, o)
    c[f1, 20_000] ^= 0x80
    c[f2] = c[f1]
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (3, 1, 2)
    got = _check(eng, oracle, c, z, keys, rep, objects, edited=[o, f1, f2, f3])
    assert got[f1] == got[f2] != got[o] and got[f3] == got[o]
    r = rep.cpu().numpy()
    assert r[f2] == f1 and r[f1] == f1 and r[f3] == o
    assert objects == int(z.numel()) - 2


def test_hot_group_beside_ordinary_ones(eng, oracle):
    """The synthetic 30 % batch with 20,000 further rows overwritten by copies of one file; it
    finishes within the time of an all-identical batch (a serialised group takes about a second)."""
    n = eng.batch_quantum
    c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    roots = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(78, 0, n, c, z, L, dup_permille=300)
    eng.synth_roots(78, 0, n, roots, dup_permille=300)
    hot = int(roots[17].item())
    extra = torch.from_numpy(np.random.default_rng(5).permutation(n)[:20_000]).cuda()
    c[extra] = c[hot].clone()
    z[extra] = z[hot].clone()
    roots[extra] = hot  # files of one root hold the same bytes, files of two roots do not
    planted = n - int(torch.unique(roots).numel())
    assert planted > 20_000
    allsame = c[5:6].repeat(n, 1)
    zsame = z[5:6].repeat(n)
    _fused(eng, allsame, zsame)  # (buffers sized, code loaded)
    torch.cuda.synchronize()
    _fused(eng, c, z)

    def timed(cc, zz):  # the best of three
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = _fused(eng, cc, zz)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return out, best
    ref, t_same = timed(allsame, zsame)
    assert ref[3] == (n - 1, n - 1, 0)
    (keys, rep, objects, counters), t_hot = timed(c, z)
    print(f"hot group {t_hot * 1e3:.2f} ms, all identical {t_same * 1e3:.2f} ms")
    assert counters == (planted, planted, 0)
    assert objects == n - planted
    assert t_hot <= t_same
    edited = np.concatenate([extra.cpu().numpy()[:300], [hot, 17, n - 1]])
    assert eng.dup_verify_rows()[0] == int(torch.unique(roots).numel()) - int((torch.bincount(roots, minlength=n) == 1).sum().item())
    _check(eng, oracle, c, z, keys, rep, objects, edited=edited)


def test_last_row_is_a_copy_and_ends_the_tensor(eng, oracle, base):
    """stride == the row length: the content tensor ends at the last copy's 57,344th byte."""
    content, sizes = base
    c, z = content.clone(), sizes.clone()
    n = int(z.numel())
    assert c.stride(0) == L and c.numel() == n * L
    for f, o in ((n - 1, 77), (n - 2, 77), (n - 3, n - 4)):
        _copy(c, z, f, o)
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (3, 3, 0)
    assert objects == n - 3
    _check(eng, oracle, c, z, keys, rep, objects, edited=[77, n - 4, n - 3, n - 2, n - 1])


def test_padded_stride_padding_differs_inside_groups_of_three(eng, oracle):
    n = eng.batch_quantum
    stride = 57_360
    c = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(32, 0, n, c, z, stride, dup_permille=0)
    k = 900
    src = torch.arange(k, device="cuda") * 5
    dst = [20_000 + torch.arange(k, device="cuda") * 11 + j for j in (0, 3, 7)]
    for d in dst:
        c[d, :L] = c[src, :L]
        z[d] = z[src]
        assert not torch.equal(c[d, L:], c[src, L:])
    assert not torch.equal(c[dst[0], L:], c[dst[1], L:])
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (3 * k, 3 * k, 0)
    assert objects == n - 3 * k
    assert eng.dup_verify_rows()[0] == k
    edited = np.concatenate([src.cpu().numpy()[:200]] + [d.cpu().numpy()[:200] for d in dst])
    _check(eng, oracle, c, z, keys, rep, objects, edited=edited)


@pytest.mark.parametrize("quanta", [1, 2])
def test_both_grid_shapes(eng, oracle, quanta):
    """The synthetic 30 % batch at one quantum (256-lane workgroups) and at two (512-lane)."""
    n = quanta * eng.batch_quantum
    c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    roots = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(79, 0, n, c, z, L, dup_permille=300)
    eng.synth_roots(79, 0, n, roots, dup_permille=300)
    iota = torch.arange(n, device="cuda")
    planted = int((roots != iota).sum().item())
    assert 0.25 * n < planted < 0.35 * n
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (planted, planted, 0)
    assert objects == n - planted
    groups, tasks, refs = eng.dup_verify_rows()
    assert groups == int(torch.unique(roots[roots != iota]).numel())
    assert groups <= refs < groups + tasks
    dups = torch.nonzero(roots != iota).flatten()[:512].cpu().numpy()
    _check(eng, oracle, c, z, keys, rep, objects, edited=dups)


def test_setter_off_after_on_is_bit_identical(eng, oracle, run_lengths):
    c, z, members, cands = run_lengths
    keys_on, rep_on, obj_on, counters_on = _fused(eng, c, z)
    assert counters_on == (cands, cands, 0)
    eng.set_dup_verify(False)
    keys_off, rep_off, obj_off, counters_off = _fused(eng, c, z)
    assert counters_off == (0, 0, 0) and eng.dup_verify_rows() == (0, 0, 0)
    assert torch.equal(keys_on, keys_off) and torch.equal(rep_on, rep_off) and obj_on == obj_off
