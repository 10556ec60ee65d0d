"""CPU tests of the pair-and-promote tree reduction (spacedrive_amd/csrc/blake3_tree.hpp): the
level rule, the in-LDS phases and the stride form, compiled for the host and driven over
simulated lanes by a stand-alone program (tests/native/tree_reduce_test.cpp, its own main,
nothing preloaded) — once plain, once under the address and undefined-behaviour sanitizers —
against the recursive left-balanced definition and the oracle.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# family -> cases: 256 lanes x 1 and x 2 parents, a 64-lane wave, four 16-lane slices side by
# side (16 rounds x 4 slices), each with and without ROOT on the top; the stride form
FAMILIES = {"lds256x1": 256, "lds256x2": 1024, "lds64": 64, "slices16": 64}
FAMILIES.update({k + "_root": v for k, v in list(FAMILIES.items())})
FAMILIES.update({"stride16": 16, "stride64": 64})
ORACLE_COUNTS = list(range(1, 65)) + [255, 256, 257, 1023, 1024]


def content(length):
    """content_byte() of tree_reduce_test.cpp"""
    i = np.arange(1, length + 1, dtype=np.uint64)
    v = (i * np.uint64(2654435761) + np.uint64(length * 0x9E3779B1 & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    return ((v >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8).tobytes()


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                ids=["plain", "asan_ubsan"])
def rows(request, tmp_path_factory):
    """The output lines of one run of the stand-alone program, split into words."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("tree_reduce") / "tree_reduce_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-x", "c++", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "tree_reduce_test.cpp"), "-o", exe]
    subprocess.run(cc + request.param, check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert not r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stdout[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_every_form_vs_the_recursive_definition(rows):
    got = {r[0]: (int(r[1]), int(r[2])) for r in rows if r[0] != "o"}
    assert got == {name: (cases, 0) for name, cases in FAMILIES.items()}


def test_roots_of_true_chunk_cvs_vs_oracle(rows, oracle):
    got = [r for r in rows if r[0] == "o"]
    assert [int(r[1]) for r in got] == ORACLE_COUNTS and all(len(r) == 3 for r in got)
    bad = [int(n) for _, n, h in got if bytes.fromhex(h) != oracle.blake3(content((int(n) - 1) * 1024 + 1))]
    assert not bad, bad[:10]
