"""GPU tests of the link emission (sd_cas_identifier_links_ex_dev, spacedrive_amd/csrc/links.hip)
at the size edges of its path for rows that already own an Object: the compaction's 16,384-row
blocks and the 256-block rounds of their offset scan, the segmented-min scan's 2,048-event tiles
and the 256-tile rounds of its tile prefix, and the key filter's "passes, but no such key"
answers of the binary search.  The cases and what each one reaches are in tests/links_cases.py,
held to the reference on the CPU by tests/test_links_cases_cpu.py; here every row's step, Object
and action and every step's counts are compared exactly with the literal job replay (the closed
form for the 4.2 M-row case), the outputs written over a poison value."""
import numpy as np
import pytest

from tests import links_cases as lc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON32, POISON8 = -7, 0xEE


def dev64(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()   # a copy: the case is read-only


def dev32(a):
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def assert_answer(got, want, case_id):
    step, obj, act, counts = got
    wstep, wobj, wact, wcounts = want
    assert [tuple(c) for c in counts.tolist()] == wcounts, case_id
    for name, g, w in (("step", step, wstep), ("object", obj, wobj), ("action", act, wact)):
        bad = np.flatnonzero(g.astype(np.int64) != w)
        assert len(bad) == 0, (case_id, name, len(bad), bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


@pytest.mark.parametrize("case_id", list(lc.CASES))
def test_links_edges(eng, case_id):
    (keys, states, pre, seeds, chunk, _), want = lc.build(case_id)
    n = len(keys)
    step = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
    obj = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
    act = torch.full((n,), POISON8, dtype=torch.uint8, device="cuda")
    sk = np.array([k for k, _ in seeds], np.uint64)
    so = np.array([o for _, o in seeds], np.uint32)
    s2, o2, a2, counts = eng.identifier_links(
        dev64(keys), torch.from_numpy(states.copy()).cuda(), chunk, existing=(dev64(sk), dev32(so)),
        pre_objects=dev32(pre), out=(step, obj, act))
    assert s2 is step and o2 is obj and a2 is act
    assert_answer((step.cpu().numpy().view(np.uint32), obj.cpu().numpy().view(np.uint32),
                   act.cpu().numpy(), counts), want, case_id)


@pytest.mark.parametrize("case_id", lc.HOST_CASES)
def test_links_edges_host(eng, case_id):
    """The same through sd_cas_identifier_links_ex (host arrays, the library's own staging)."""
    (keys, states, pre, seeds, chunk, _), want = lc.build(case_id)
    sk = np.array([k for k, _ in seeds], np.uint64)
    so = np.array([o for _, o in seeds], np.uint32)
    got = eng.identifier_links_host(keys, states, chunk, existing=(sk, so), pre_objects=pre)
    assert_answer(got, want, case_id)
