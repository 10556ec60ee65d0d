"""GPU tests of the two placements of the fused chain's duplicate compares (dup_verify.hip K1V;
SD_CAS_DUP_PLACEMENT, read at context creation): `static`, the tile map fixed before launch, and
`cu`, roles taken at run time by each workgroup (sd_dup_runs.h); `auto`, the default, chooses
between them by the batch's size.  Every case runs through one context of each placement.  The static context's keys are checked against the oracle on a sample
that holds the edited files, its rep and Object count against the standalone grouping, and its
counters against the construction (tests/dup_plant.py's model where a plan is used); the cu
context's keys, rep, Object count, dup_verify_counters and dup_verify_rows must equal the static
context's.  Batches are one batch quantum unless a name says otherwise.  Run against the debug
library, the finish kernel's conservation check (hash tiles run, tasks run, every per-CU counter back
at zero) fails the test through conftest's violation counter."""
import os

import numpy as np
import pytest
import torch

from tests import dup_plant as dp

pytestmark = pytest.mark.gpu

L = dp.L
PLACEMENTS = ("static", "cu", "auto")


@pytest.fixture(scope="module")
def engines(eng):
    """A context per placement (eng: the session's context has initialised the device)."""
    from spacedrive_amd import CasEngine
    old = os.environ.get("SD_CAS_DUP_PLACEMENT")
    made = {}
    try:
        for p in PLACEMENTS:
            os.environ["SD_CAS_DUP_PLACEMENT"] = p
            made[p] = CasEngine(0)
    finally:
        if old is None:
            os.environ.pop("SD_CAS_DUP_PLACEMENT", None)
        else:
            os.environ["SD_CAS_DUP_PLACEMENT"] = old
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def base(eng):
    """One quantum of distinct files (never modified: the cases edit clones)."""
    n = eng.batch_quantum
    content = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(0xD0B1E5, 0, n, content, sizes, L, dup_permille=0)
    torch.cuda.synchronize()
    return content, sizes


def _probed(e, content, sizes):
    """One fused call that probes whatever the context saw before (the setter re-arms it)."""
    e.set_dup_verify(True)
    keys, rep, objects, counters = dp.fused(e, content, sizes)
    return keys, rep, objects, counters, e.dup_verify_rows()


def _both(engines, oracle, content, sizes, edited=(), other="cu"):
    """Both placements on one batch: static checked against the oracle and the standalone
    grouping, cu against static.  Returns static's (keys, rep, objects, counters, rows)."""
    ref = _probed(engines["static"], content, sizes)
    dp.check(engines["static"], oracle, content, sizes, ref[0], ref[1], ref[2], edited=edited)
    got = _probed(engines[other], content, sizes)
    assert torch.equal(got[0], ref[0]), "keys differ between the placements"
    assert torch.equal(got[1], ref[1]), "rep differs between the placements"
    assert got[2:] == ref[2:], f"objects, counters, rows: {other} {got[2:]} static {ref[2:]}"
    n_cand = ref[3][0]
    assert ref[4][1] == (n_cand + dp.RUN_K - 1) // dp.RUN_K  # every task ran, once
    return ref


def test_unknown_placement_is_refused(eng, monkeypatch):
    from spacedrive_amd import CasEngine
    monkeypatch.setenv("SD_CAS_DUP_PLACEMENT", "both")
    with pytest.raises(Exception):
        CasEngine(0)


def test_every_file_identical(engines, oracle, base):
    """n_hash = 1: the hash queue is empty after one workgroup and almost every other one takes
    the drain path."""
    content, sizes = base
    n = int(sizes.numel())
    c = content[5:6].repeat(n, 1)
    z = sizes[5:6].repeat(n)
    keys, rep, objects, counters, rows = _both(engines, oracle, c, z, edited=[0, 1, n - 1])
    assert counters == (n - 1, n - 1, 0) and objects == 1
    assert rows[0] == 1 and rows[2] == rows[1]  # one group: a reference row per task
    assert int(rep.max().item()) == 0


def test_no_two_files_alike(engines, oracle, base):
    """No task: every workgroup hashes.  That the calls probed (and did not run the paused path)
    shows in the call after them, which is not re-armed: the note of zero candidates pauses it."""
    content, sizes = base
    n = int(sizes.numel())
    keys, rep, objects, counters, rows = _both(engines, oracle, content, sizes)
    assert counters == (0, 0, 0) and rows == (0, 0, 0) and objects == n
    c, z = content.clone(), sizes.clone()
    c[n - 1] = c[0]
    z[n - 1] = z[0]
    for p in ("static", "cu"):
        torch.cuda.synchronize()
        k2, r2, o2, paused = dp.fused(engines[p], c, z)
        assert paused == (0, 0, 0) and o2 == n - 1 and int(r2[n - 1].item()) == 0
        assert _probed(engines[p], c, z)[3] == (1, 1, 0)


@pytest.mark.parametrize("quanta", [1, 2, 3, 4])
def test_synthetic_thirty_percent(engines, oracle, eng, quanta):
    """1 and 3 quanta are the static placement's 256-lane grid, 2 and 4 its 512-lane one; the
    third shape's list H is no whole number of 256-file tiles.  Up to 3 quanta the chip holds the
    run-time roles' whole grid at once and a compare workgroup has no quota; 4 quanta (4 x CUs + 1
    workgroups) is the smallest batch whose compare workgroups leave after their quota and whose
    last workgroup waits for a place."""
    n = quanta * eng.batch_quantum
    c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    roots = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(81, 0, n, c, z, L, dup_permille=300)
    eng.synth_roots(81, 0, n, roots, dup_permille=300)
    iota = torch.arange(n, device="cuda")
    planted = int((roots != iota).sum().item())
    assert 0.25 * n < planted < 0.35 * n
    if quanta == 3:
        assert (n - planted) % 256 != 0
    dups = torch.nonzero(roots != iota).flatten()[:512].cpu().numpy()
    keys, rep, objects, counters, rows = _both(engines, oracle, c, z, edited=dups)
    assert counters == (planted, planted, 0) and objects == n - planted
    assert rows[0] == int(torch.unique(roots[roots != iota]).numel())
    assert rows[0] <= rows[2] < rows[0] + rows[1]


def test_default_placement_from_twelve_quanta(engines, oracle, eng):
    """auto takes the run-time roles from three rounds of the chip's workgroup slots on (12 quanta:
    sd_dup_runs.h dup_roles_pay) and the static map below: the first batch on the roles' side."""
    n = 12 * eng.batch_quantum
    c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(83, 0, n, c, z, L, dup_permille=300)
    keys, rep, objects, counters, rows = _both(engines, oracle, c, z, other="auto")
    assert 0.25 * n < counters[0] < 0.35 * n and counters[1] == counters[0] and counters[2] == 0
    assert objects == n - counters[0]


def test_fewer_tasks_than_cus(engines, oracle, base):
    """Five groups of two spread over the batch: five candidates, one task."""
    content, sizes = base
    n = int(sizes.numel())
    c, z = content.clone(), sizes.clone()
    plan = [dp.Group([11 + 9_001 * i, n - 7 - 5_003 * i]) for i in range(5)]
    dp.apply(plan, c, z)
    want = dp.expect(plan, n)
    keys, rep, objects, counters, rows = _both(engines, oracle, c, z, edited=want.planted)
    assert counters == want.counters == (5, 5, 0)
    assert objects == want.objects and rows == (5, 1, 5)
    assert (rep.cpu().numpy() == want.rep).all()


def test_hot_group_beside_ordinary_ones(engines, oracle, eng):
    """The synthetic 30 % batch with 20,000 further rows overwritten by copies of one file."""
    n = eng.batch_quantum
    c = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    z = torch.empty(n, dtype=torch.int64, device="cuda")
    roots = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(82, 0, n, c, z, L, dup_permille=300)
    eng.synth_roots(82, 0, n, roots, dup_permille=300)
    hot = int(roots[17].item())
    extra = torch.from_numpy(np.random.default_rng(6).permutation(n)[:20_000]).cuda()
    c[extra] = c[hot].clone()
    z[extra] = z[hot].clone()
    roots[extra] = hot  # files of one root hold the same bytes, files of two roots do not
    classes = torch.unique(roots)
    planted = n - int(classes.numel())
    assert planted > 20_000
    edited = np.concatenate([extra.cpu().numpy()[:300], [hot, 17, n - 1]])
    keys, rep, objects, counters, rows = _both(engines, oracle, c, z, edited=edited)
    assert counters == (planted, planted, 0) and objects == n - planted
    assert rows[0] == int(classes.numel()) - int((torch.bincount(roots, minlength=n) == 1).sum().item())
