"""GPU tests of the fused chain's duplicate verification (dup_verify.hip K1V: probe, candidate
lists, the mixed hash / compare kernel, the finish kernel; sd_cas_set_dup_verify and
sd_cas_dup_verify_counters).  Every case is one batch quantum, the smallest batch the fused chain
accepts.  For every case the keys equal the oracle's on a sample of at least 2,048 files that
holds every edited file, rep and the Object count equal the standalone grouping's, and the
counters (candidates, verified, rehashed) are what the case planted."""
import numpy as np
import pytest
import torch

from oracle.pyoracle import SAMPLED_CONTENT_LEN

pytestmark = pytest.mark.gpu

L = SAMPLED_CONTENT_LEN
SAMPLE = 2048


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


def test_distinct_files(eng, oracle, base):
    content, sizes = base
    keys, rep, objects, (cand, verified, rehashed) = _fused(eng, content, sizes)
    assert verified == 0 and rehashed == cand == 0
    assert objects == int(sizes.numel())
    _check(eng, oracle, content, sizes, keys, rep, objects)


def test_synthetic_duplicates(eng, oracle):
    n = eng.batch_quantum
    content = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    roots = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(77, 0, n, content, sizes, L, dup_permille=300)
    eng.synth_roots(77, 0, n, roots, dup_permille=300)
    planted = int((roots != torch.arange(n, device="cuda")).sum().item())
    assert 0.25 * n < planted < 0.35 * n
    keys, rep, objects, counters = _fused(eng, content, sizes)
    assert counters == (planted, planted, 0)
    assert objects == n - planted
    dups = torch.nonzero(roots != torch.arange(n, device="cuda")).flatten()[:512].cpu().numpy()
    _check(eng, oracle, content, sizes, keys, rep, objects, edited=dups)


def test_all_identical_spills_regions(eng, oracle, base):
    content, sizes = base
    n = int(sizes.numel())
    c = content[5:6].repeat(n, 1)
    z = sizes[5:6].repeat(n)
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (n - 1, n - 1, 0)
    assert objects == 1 and int(rep.max().item()) == 0
    _check(eng, oracle, c, z, keys, rep, objects, edited=[0, 1, n - 1])


def test_near_misses_are_rehashed(eng, oracle, base):
    """Equal size, equal first and last 32 B (so equal probes), one byte apart elsewhere."""
    content, sizes = base
    c, z = content.clone(), sizes.clone()
    offs = [32, 28_671, 28_672, 57_311]
    a = [100 + 3 * i for i in range(4)]
    b = [40_000 + 517 * i for i in range(4)]
    for ai, bi, off in zip(a, b, offs):
        c[bi] = c[ai]
        z[bi] = z[ai]
        c[bi, off] ^= 0x40
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (4, 0, 4)
    got = _check(eng, oracle, c, z, keys, rep, objects, edited=a + b)
    assert all(got[ai] != got[bi] for ai, bi in zip(a, b))
    assert objects == int(z.numel())


def test_equal_content_different_size(eng, oracle, base):
    content, sizes = base
    c, z = content.clone(), sizes.clone()
    a, b = [7, 300], [9_000, 65_000]
    for ai, bi in zip(a, b):
        c[bi] = c[ai]
        z[bi] = z[ai] + 1
    keys, rep, objects, (cand, verified, rehashed) = _fused(eng, c, z)
    assert verified == 0 and rehashed == cand
    got = _check(eng, oracle, c, z, keys, rep, objects, edited=a + b)
    assert all(got[ai] != got[bi] for ai, bi in zip(a, b))


def test_candidate_of_a_file_in_a_later_tile(eng, oracle, base):
    """20,000 duplicates at the end of the batch, of files just before them: the first compare
    tiles of the grid hold pairs whose earlier file is hashed by one of the last hash tiles."""
    content, sizes = base
    n = int(sizes.numel())
    c, z = content.clone(), sizes.clone()
    k = 20_000
    dst = torch.arange(n - k, n, device="cuda")
    src = 40_000 + (torch.arange(k, device="cuda") % 5_000)
    c[dst] = c[src]
    z[dst] = z[src]
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (k, k, 0)
    assert objects == n - k
    assert torch.equal(rep[dst].long(), src)
    edited = np.concatenate([np.arange(n - k, n - k + 300), np.arange(40_000, 40_300), [n - 1]])
    _check(eng, oracle, c, z, keys, rep, objects, edited=edited)


def test_padded_stride_with_different_padding(eng, oracle):
    n = eng.batch_quantum
    stride = 57_360
    c = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(31, 0, n, c, z, stride, dup_permille=0)
    k = 1_000
    src = torch.arange(k, device="cuda") * 3
    dst = 30_000 + torch.arange(k, device="cuda") * 7
    c[dst, :L] = c[src, :L]
    z[dst] = z[src]
    assert not torch.equal(c[dst, L:], c[src, L:])
    keys, rep, objects, counters = _fused(eng, c, z)
    assert counters == (k, k, 0)
    assert objects == n - k
    _check(eng, oracle, c, z, keys, rep, objects,
           edited=np.concatenate([src.cpu().numpy(), dst.cpu().numpy()]))


def test_alternating_region_sets_then_group_regions(eng, oracle):
    n = eng.batch_quantum
    batches = []
    for seed in (91, 92):
        c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
        z = torch.empty(n, dtype=torch.int64, device="cuda")
        r = torch.empty(n, dtype=torch.int64, device="cuda")
        eng.synth_sampled(seed, 0, n, c, z, L, dup_permille=300)
        eng.synth_roots(seed, 0, n, r, dup_permille=300)
        batches.append((c, z, int((r != torch.arange(n, device="cuda")).sum().item())))
    keys = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2)]
    reps = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()  # the inputs are ready; from here on the library orders the streams
    # set A, then set B on another stream (A is dropped ungrouped), B's tables, then A again
    eng.hash_regions_sampled(batches[0][0], batches[0][1], keys[0], reps[0], ovf)
    eng.hash_regions_sampled(batches[1][0], batches[1][1], keys[1], reps[1], ovf, stream=side.cuda_stream)
    assert eng.dup_verify_counters() == (batches[1][2], batches[1][2], 0)
    obj1 = eng.group_regions(n, reps[1], stream=side.cuda_stream)
    eng.hash_regions_sampled(batches[0][0], batches[0][1], keys[0], reps[0], ovf)
    assert eng.dup_verify_counters() == (batches[0][2], batches[0][2], 0)
    obj0 = eng.group_regions(n, reps[0])
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    for j, obj in ((0, obj0), (1, obj1)):
        assert obj == n - batches[j][2]
        _check(eng, oracle, batches[j][0], batches[j][1], keys[j], reps[j], obj)


def test_few_candidates_pause_the_probing(eng, oracle, base):
    """A probed batch with fewer than 1 candidate in 32 files: the next 16 calls run the plain
    K1G (no counters, the same results), the call after them probes again, and so does the
    first call after the setter."""
    content, sizes = base
    c, z = content.clone(), sizes.clone()
    c[50_000] = c[3]
    z[50_000] = z[3]
    c[50_000, 1_000] ^= 1  # one near miss: a candidate that is rehashed
    first = _fused(eng, c, z)
    assert first[3] == (1, 0, 1)
    _check(eng, oracle, c, z, *first[:3], edited=[3, 50_000])
    for _ in range(16):
        keys, rep, objects, counters = _fused(eng, c, z)
        assert counters == (0, 0, 0)
        assert torch.equal(keys, first[0]) and torch.equal(rep, first[1]) and objects == first[2]
    assert _fused(eng, c, z)[3] == (1, 0, 1)
    assert _fused(eng, c, z)[3] == (0, 0, 0)
    eng.set_dup_verify(True)
    assert _fused(eng, c, z)[3] == (1, 0, 1)


def test_setter_off_is_bit_identical(eng, oracle):
    n = eng.batch_quantum
    c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(55, 0, n, c, z, L, dup_permille=300)
    keys_on, rep_on, obj_on, counters_on = _fused(eng, c, z)
    assert counters_on[1] > 0
    eng.set_dup_verify(False)
    keys_off, rep_off, obj_off, counters_off = _fused(eng, c, z)
    assert counters_off == (0, 0, 0)
    assert torch.equal(keys_on, keys_off) and torch.equal(rep_on, rep_off) and obj_on == obj_off
    _check(eng, oracle, c, z, keys_off, rep_off, obj_off)
    with pytest.raises(Exception):
        eng._check(eng.L.sd_cas_set_dup_verify(eng.h, 2), "set_dup_verify")
