"""CPU test of csrc/sd_dup_probe.h, the probe that nominates duplicate candidates for the fused
chain: a stand-alone host program (its own main, nothing preloaded), plain and under
-fsanitize=address,undefined — bounds at row offsets 0 and 57,312, determinism, every edge byte
counted."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_probe_bounds_and_determinism(tmp_path, flags):
    exe = str(tmp_path / "dup_probe_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "dup_probe_test.cpp"), "-o", exe]
    subprocess.run(cc + flags, check=True, capture_output=True, timeout=600)
    runs = [subprocess.run([exe], capture_output=True, text=True, timeout=120) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("dup_probe ok ")
    assert runs[0].stdout == runs[1].stdout  # the same probe in another process
