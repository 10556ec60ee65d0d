"""CPU test of the run-time roles of csrc/sd_dup_runs.h (which workgroup of the fused chain's main
kernel hashes, compares or drains the task queue: the progress rule, the CU slot, the compare
budget): a stand-alone host program (its own main, nothing preloaded), built here as
tests/test_dup_groups_cpu.py builds its own, plain and under -fsanitize=address,undefined, for
every per-CU limit and quota the kernel was swept at."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("limit,quota", [(None, None), (1, 1), (2, 1), (0, 1), (1, 2), (2, 2), (0, 2)],
                         ids=["default", "l1q1", "l2q1", "nolimit-q1", "l1q2", "l2q2", "nolimit-q2"])
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_progress_rule_cu_slot_and_arrival_orders(tmp_path, san, limit, quota):
    exe = str(tmp_path / "dup_roles_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "dup_roles_test.cpp"), "-o", exe]
    defs = [] if limit is None else [f"-DSD_DUP_CU_LIMIT={limit}", f"-DSD_DUP_QUOTA_MUL={quota}"]
    subprocess.run(cc + san + defs, check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("dup_roles ok LIMIT=")
    if limit is not None:
        assert r.stdout.strip().startswith(f"dup_roles ok LIMIT={limit} QUOTA={quota} ")
