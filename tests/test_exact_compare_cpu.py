"""CPU tests of the whole-content compare (sd_cas_group_exact_contents_dev): its task arithmetic
(spacedrive_amd/csrc/sd_content_tasks.h) as a stand-alone host program, plain and under
ASan + UBSan; the constants the library exports; and a numpy model of the rounds (pivot
election, the cap's hand-over to the digest route) held to a dict-based reference over the
content patterns the GPU tests use, which also fixes the round counts those tests expect and
the random case's seed.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import exact_compare_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_task_arithmetic(tmp_path, flags):
    """Its own main, nothing preloaded: piece counts at 0, 1, PIECE +- 1, 2^32 +- 1 and 64 GiB,
    task -> (entry, piece) over lists of 1, K - 1, K, K + 1 and 2 K + 1 entries of mixed lengths,
    run starts, the last-quad mask for all 16 residues."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "content_tasks_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC,
          os.path.join(NATIVE, "content_tasks_test.cpp"), "-o", exe]
    subprocess.run(cc + flags, check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    s, p, k, _ = cases.constants()
    assert r.stdout.strip() == f"content_tasks ok slice={s} piece={p} run_k={k}"


def test_constants_are_the_headers():
    s, p, k, rounds = cases.constants()
    assert s == 8192 and p % s == 0 and 1 <= k <= 32 and rounds >= 1
    text = open(os.path.join(ROOT, "include", "sd_hip_cas.h")).read()
    assert f"#define SD_CAS_EXACT_COMPARE_ROUNDS_DEFAULT {rounds}\n" in text
    import spacedrive_amd as sa
    assert sa.EXACT_COMPARE_ROUNDS_DEFAULT == rounds


def check_model(rep, blobs, caps=(0, 1, 2, 4)):
    want = cases.reference(rep, blobs)
    out = {}
    for cap in caps:
        got, rounds, compares, unequal, digest_rows = cases.model_rounds(rep, blobs, cap)
        assert (got == want).all(), (cap, np.flatnonzero(got != want)[:8])
        assert (cap == 0 and digest_rows == 0) or rounds <= cap
        assert unequal <= compares
        out[cap] = (rounds, compares, unequal, digest_rows)
    return want, out


def test_model_abc():
    rep, blobs = cases.abc_case()
    want, out = check_model(rep, blobs)
    assert want.tolist() == [0, 1, 0, 3, 1, 0, 3, 3]
    assert out[0] == (3, 7 + 4 + 2, 5 + 3, 0)
    assert out[1][0] == 1 and out[1][3] == 4  # rows 3, 4, 6, 7 go on with pivot 1
    assert out[2][3] == 2


def test_model_sweep_and_lengths():
    rep, blobs = cases.sweep_case()
    want, out = check_model(rep, blobs, caps=(0, 1))
    assert len(blobs) == 2 * 4102 and out[0] == out[1] == (1, 4102, 4101, 0)
    assert (want[1::2][:-1] == np.arange(1, 2 * 4101, 2)).all() and want[-1] == 2 * 4101
    s, p, _, _ = cases.constants()
    rep, blobs, cs = cases.lengths_case(s, p)
    want, out = check_model(rep, blobs, caps=(0, 1))
    assert out[0] == out[1] == (1, 2 * len(cs), len(cs), 0)
    assert (want.reshape(-1, 3) == (3 * np.arange(len(cs)))[:, None] + np.array([0, 0, 2])).all()
    # every slice and piece boundary below L, both sides, and both ends
    L = 2 * p + 17
    at = {b for ln, b in cs if ln == L}
    assert {0, L - 1, s - 1, s, p - 1, p, 2 * p - 1, 2 * p, 2 * p - s, 2 * p + 16} <= at
    assert {ln for ln, _ in cs} >= {1, 15, 16, 17, s - 1, s, s + 1, p - 1, p, p + 1, L}


def test_model_classes_and_the_cap():
    _, _, k, _ = cases.constants()
    rep, blobs = cases.classes_case(k, 8192)
    want, out = check_model(rep, blobs)
    assert out[0][0] == 39 and out[0][3] == 0  # 40 pairwise-distinct rows: 39 rounds without a cap
    assert out[1][3] > 0 and out[2][3] > 0 and out[4][3] > 0
    # rows the cap hands over whose content equals their current pivot's: the pivot must go along
    a, b = b"a" * 100, b"b" * 100
    for cap in (1, 2):
        got = cases.model_rounds(np.zeros(5, np.uint32), [a, b, b, a, b], cap)
        assert got[0].tolist() == [0, 1, 1, 0, 1]


def test_random_case_meets_its_conditions():
    rep, blobs = cases.random_case()
    want, out = check_model(rep, blobs, caps=(0, 1, 4))
    below, split, rich = cases.random_case_facts(rep, want)
    assert len(blobs) == 6000 and below >= 1000 and split >= 500 and rich >= 50, (below, split, rich)
    assert max(len(b) for b in blobs) <= 40 * 1024
    assert out[0][3] == 0 and out[0][0] >= 2
