"""GPU tests of the hash grouping (sd_cas_group_dev / sd_cas_group_min_dev,
spacedrive_amd/csrc/group_hash.hip) at the exact edges of its three chains: a region at its
capacity and one row past it, a reservation that starts at g == cap, a bucket of exactly one trip
and one row more, exactly FILL distinct keys and one more, an LDS table without a free slot, a
failed READ_FIRST claim, two global tables carved in one call, own tables side by side, probe
chains that wrap in LDS and in global memory, and the persistent counters after calls that leave
something behind.  The cases and the exit each one reaches are in tests/group_cases.py, held to a
CPU model by tests/test_group_cases_cpu.py; here every row's representative / minimum and the
Object count are compared exactly with numpy (first row per key; minimum.at), the outputs written
over a poison value, every call made twice in a row."""
import numpy as np
import pytest

from tests import group_cases as gc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B


def explain(case_id, what, got, want, keys, target):
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    m = gc.model(keys, target)
    i = int(bad[0])
    b = gc.bucket_of_row(keys, i, m["bits"])
    return (f"{case_id} {what}: {len(bad)} wrong rows, first row {i} got {int(got[i])} want {int(want[i])}, "
            f"chain {m['chain']} bucket {b} ({int(m['rows'][b])} rows, {int(m['distinct'][b])} distinct), "
            f"predicted exit {m['exit'][b]}")


def run_case(eng, case_id, repeats=2):
    c = gc.build(case_id)
    keys, target, n = c["keys"], c["target"], len(c["keys"])
    dk = torch.from_numpy(np.array(keys).view(np.int64)).cuda()          # a copy: the case is read-only
    dv = torch.from_numpy(np.array(c["vals"]).view(np.int32)).cuda()
    if target:
        eng.set_group_method(eng.GROUP_HASH, target)
    try:
        for call in range(repeats):
            rep = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
            objects = eng.group(dk, rep)
            msg = explain(case_id, f"group call {call}", rep.cpu().numpy().view(np.uint32), c["rep"], keys, target)
            assert msg is None, msg
            assert objects == c["objects"], (case_id, "group call", call, objects, c["objects"])
        for call in range(repeats):
            out = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
            objects = eng.group_min(dk, dv, out)
            msg = explain(case_id, f"group_min call {call}", out.cpu().numpy().view(np.uint32), c["mins"], keys, target)
            assert msg is None, msg
            assert objects == c["objects"], (case_id, "group_min call", call, objects, c["objects"])
    finally:
        if target:
            eng.set_group_method()


@pytest.mark.parametrize("case_id", [c for c in gc.CASES if "-seq-" not in c])
def test_group_edges(eng, case_id):
    run_case(eng, case_id)


@pytest.mark.parametrize("seq", list(gc.SEQUENCES))
def test_group_sequences(eng, seq):
    """Calls on one engine in an order in which a counter left behind by one call (the spill
    count, the full-region and done counts, the bucket totals, the region cursors) changes the
    answer of a later one; every call is checked."""
    for case_id in gc.SEQUENCES[seq]:
        run_case(eng, case_id, repeats=1)
