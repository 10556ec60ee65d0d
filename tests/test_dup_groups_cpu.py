"""CPU test of csrc/sd_dup_runs.h, the index arithmetic of the fused chain's compare tasks (task
window -> entries, workgroup -> hash or compare tile, slice -> quads): a stand-alone host program
(its own main, nothing preloaded), built here as tests/test_dup_probe_cpu.py builds its own, plain
and under -fsanitize=address,undefined, for every task width the kernel was swept at."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("k", [None, 8, 16, 32], ids=["default", "k8", "k16", "k32"])
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_task_windows_tiles_and_slices(tmp_path, san, k):
    exe = str(tmp_path / "dup_runs_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "dup_runs_test.cpp"), "-o", exe]
    subprocess.run(cc + san + ([f"-DSD_DUP_RUN_K={k}"] if k else []), check=True, capture_output=True,
                   timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("dup_runs ok K=")
    if k:
        assert r.stdout.strip() == f"dup_runs ok K={k}"
