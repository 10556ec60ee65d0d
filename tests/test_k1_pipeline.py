"""K1 / K1G line pipeline (csrc/cas_sampled.hpp, cas_lane_sampled): every key of a batch against
the oracle, at the batch sizes where the dispatch changes the grid.

The lane program walks a file's 448 lines as one sequence and refills each of its two line
buffers in place while the other is being compressed.  A line fetched from the wrong place,
or landing in a buffer that is still being read, changes that lane's key, so the tests
compare EVERY key (not a sample) of 30 %-duplicate batches of

  * one quantum (the 256-lane grid),
  * two quanta (the 512-lane grid),
  * two quanta + 77 files (K1 over the quanta, K1L on the remainder beside it),

for K1 (hash_sampled) and for K1G (hash_regions_sampled + group_regions; a batch that is not a
whole number of quanta is not eligible for the region chain, so the + 77 batch takes
hash_group_sampled, which then runs K1 and the standalone grouping).  The last line of a row
is the last thing a lane reads: a padded stride filled with a non-zero pattern must not reach
a key, and a batch whose last row ends exactly at the end of its allocation must hash like
any other (the loop requests no line past the 448th).

The reference keys are computed once per module and shared.
"""
import numpy as np
import pytest

from oracle.pyoracle import SAMPLED_CONTENT_LEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

L = SAMPLED_CONTENT_LEN
EXTRA = 77


def host64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def batch(eng, oracle):
    """2 quanta + 77 sampled files, 30 % duplicates, resident on the device, and the oracle's
    key of every one of them (read-only for the tests)."""
    q = eng.batch_quantum
    n = 2 * q + EXTRA
    content = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(0x4B31, 0, n, content, sizes, L, dup_permille=300)
    torch.cuda.synchronize()
    host = content.cpu().numpy()
    want = oracle.fast_cas_keys_strided(host.reshape(-1), L, L, host64(sizes), 16)
    del host
    want.setflags(write=False)
    assert len(np.unique(want)) < n - n // 5  # the duplicates are there
    yield content, sizes, want
    del content
    torch.cuda.empty_cache()


def sizes_of(eng):
    q = eng.batch_quantum
    return {"quantum": q, "two_quanta": 2 * q, "two_quanta_plus": 2 * q + EXTRA}


@pytest.mark.parametrize("shape", ["quantum", "two_quanta", "two_quanta_plus"])
def test_k1_every_key_vs_oracle(eng, batch, shape):
    content, sizes, want = batch
    n = sizes_of(eng)[shape]
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    eng.hash_sampled(content, sizes, keys, n=n)
    got = host64(keys)
    bad = np.flatnonzero(got != want[:n])
    assert bad.size == 0, f"{bad.size} of {n} keys differ, first at file {bad[:5]}"


@pytest.mark.parametrize("shape", ["quantum", "two_quanta", "two_quanta_plus"])
def test_k1g_every_key_and_rep(eng, batch, shape):
    """K1G: keys == the oracle's, rep == the standalone grouping's, the overflow flag stays 0,
    and a second launch on the same context gives the same result (its cursors are left
    zero)."""
    content, sizes, want = batch
    q = eng.batch_quantum
    n = sizes_of(eng)[shape]
    c, z = content[:n], sizes[:n]
    ref_keys = torch.from_numpy(want[:n].view(np.int64).copy()).cuda()
    ref_rep = torch.empty(n, dtype=torch.int32, device="cuda")
    ref_objects = eng.group(ref_keys, ref_rep)
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    for launch in range(2):
        keys = torch.zeros(n, dtype=torch.int64, device="cuda")
        rep = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        if n % q == 0:
            eng.hash_regions_sampled(c, z, keys, rep, ovf)
            objects = eng.group_regions(n, rep)
        else:
            with pytest.raises(Exception):  # the region chain takes whole quanta only
                eng.hash_regions_sampled(c, z, keys, rep, ovf)
            objects = eng.hash_group_sampled(c, z, keys, rep, ovf)
        torch.cuda.synchronize()
        bad = np.flatnonzero(host64(keys) != want[:n])
        assert bad.size == 0, f"launch {launch}: {bad.size} of {n} keys differ, first at {bad[:5]}"
        assert int(ovf.item()) == 0, launch
        assert objects == ref_objects, launch
        assert torch.equal(rep, ref_rep), launch


def test_padded_stride_does_not_reach_a_key(eng, batch):
    """Rows at stride 57,344 + 4,096 with the padding filled with a non-zero pattern: the keys
    of the stride-57,344 rows, K1 and K1G."""
    content, sizes, want = batch
    n = eng.batch_quantum
    stride = L + 4096
    padded = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
    padded[:, :L] = content[:n]
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    eng.hash_sampled(padded, sizes, keys, n=n)
    assert (host64(keys) == want[:n]).all()
    keys.zero_()
    rep = torch.empty(n, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.hash_regions_sampled(padded, sizes[:n], keys, rep, ovf)
    eng.group_regions(n, rep, want_objects=False)
    torch.cuda.synchronize()
    assert (host64(keys) == want[:n]).all() and int(ovf.item()) == 0
    del padded
    torch.cuda.empty_cache()


def test_last_row_ends_with_its_allocation(eng, batch):
    """A batch in a tensor of exactly n * 57,344 bytes: the last lane's last line is the last
    128 bytes of the allocation.  (The guard: cas_lane_sampled leaves its loop before it
    would request line 448.)"""
    content, sizes, want = batch
    n = eng.batch_quantum
    torch.cuda.empty_cache()
    flat = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    assert flat.numel() * flat.element_size() == n * L
    flat.view(n, L).copy_(content[:n])
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    eng.hash_sampled(flat, sizes, keys, stride=L, n=n)
    assert (host64(keys) == want[:n]).all()
    keys.zero_()
    rep = torch.empty(n, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.hash_regions_sampled(flat.view(n, L), sizes[:n], keys, rep, ovf)
    eng.group_regions(n, rep, want_objects=False)
    torch.cuda.synchronize()
    assert (host64(keys) == want[:n]).all() and int(ovf.item()) == 0
    del flat
    torch.cuda.empty_cache()
