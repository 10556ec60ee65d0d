"""CPU test of the fused chain's region-set decisions (spacedrive_amd/csrc/sd_region_sets.h): which
set a hash_regions call refills and what it waits for first, when group_regions is refused, and
where the context's last Object count lies.  tests/native/region_sets_test.cpp replays the call
sequences of the GPU tests test_hash_regions_split_pipelined,
test_hash_regions_streams_and_ungrouped and test_alternating_region_sets_then_group_regions as
pure transitions.  No GPU and no library: the header includes no HIP header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_region_set_decisions(tmp_path, flags):
    """A stand-alone host program (its own main, nothing preloaded), run directly."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "region_sets_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-x", "c++", "-I", CSRC,
          os.path.join(NATIVE, "region_sets_test.cpp"), "-o", exe]
    subprocess.run(cc + flags, check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "region_sets ok"


def test_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "sd_region_sets.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert includes == ["<stdint.h>"]
