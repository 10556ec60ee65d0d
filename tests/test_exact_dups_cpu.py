"""CPU tests of the exact duplicate grouping (include/sd_hip_cas.h: sd_cas_group_exact_dev,
sd_cas_duplicate_report_exact): the checksum hex helpers, the two workspace layouts (each one
function that measures and carves), and the sampling gap the GPU file test rests on — bytes of a
file beyond 100 KiB that no cas_id sees.  No GPU: only host functions of libsd_hip_cas.so."""
import ctypes
import os
import subprocess

import pytest

import spacedrive_amd as sa
from oracle.pyoracle import py_sample_plan
from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = "/opt/rocm/bin/hipcc"

HEX = "0123456789abcdef" * 4


def test_hex_round_trip_either_case():
    raw = bytes(range(7, 39))
    assert sa.digest_from_hex(raw.hex()) == raw
    assert sa.digest_to_hex(raw) == raw.hex()  # lowercase, as Hash::to_hex
    assert sa.digest_from_hex(raw.hex().upper()) == raw
    mixed = "".join(c.upper() if i % 3 else c for i, c in enumerate(HEX))
    assert sa.digest_to_hex(sa.digest_from_hex(mixed)) == HEX
    assert sa.digest_to_hex(b"\xff" * 32) == "f" * 64 and sa.digest_to_hex(bytes(32)) == "0" * 64


@pytest.mark.parametrize("bad", [HEX[:63], HEX + "0", "g" + HEX[1:], HEX[:40] + " " + HEX[41:], "",
                                 HEX[:62] + "0x"], ids=["63", "65", "nonhex", "space", "empty", "0x"])
def test_hex_refused(bad):
    with pytest.raises(ValueError):
        sa.digest_from_hex(bad)
    # the raw ABI: SD_CAS_EINVAL and `out` left as it was
    out = ctypes.create_string_buffer(b"\xa5" * 32, 32)
    assert _native.lib().sd_cas_digest_from_hex(bad.encode(), ctypes.addressof(out)) == -1
    assert out.raw == b"\xa5" * 32


def test_hex_null_pointers_are_refused():
    out = ctypes.create_string_buffer(32)
    assert _native.lib().sd_cas_digest_from_hex(None, ctypes.addressof(out)) == -1
    assert _native.lib().sd_cas_digest_from_hex(HEX.encode(), None) == -1


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    _native.lib()  # the library must have been built
    libdir = os.path.dirname(_native.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("exact_layout") / "exact_layout_test")
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC,
                    os.path.join(NATIVE, "exact_layout_test.cpp"), "-o", exe, "-D__HIP_PLATFORM_AMD__",
                    "-I", "/opt/rocm/include", "-L", libdir, "-l:" + os.path.basename(_native.LIB_PATH),
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread"],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        assert f[0] == "L"
        out[f[1]] = (int(f[2]), int(f[3]), [(m.split(":")[0], int(m.split(":")[1]), int(m.split(":")[2]))
                                            for m in f[4:]])
    return out


def test_layouts_measure_what_they_carve(layouts):
    """Members ascend in declaration order on 256-B boundaries, each past the previous member's
    use, and the last one's use fits the total; the null-base total is the carved total."""
    for n in (0, 1, 65537, 1441792):
        assert f"exact({n})" in layouts
        for m in (0, n // 2, n):
            for k in (0, 1024):
                assert f"exact_report({n},{m},{k})" in layouts
    for key, (total, measured, members) in layouts.items():
        assert total == measured, key
        end = 0
        for name, off, need in members:
            assert off % 256 == 0 and off >= end, (key, name)
            end = off + need
        assert end <= total, key
    # the counter is a block of its own even at n = 0; digests are 32 B per eligible row
    assert layouts["exact(0)"][0] == 256
    assert dict((a, c) for a, _, c in layouts["exact_report(65537,65537,0)"][2])["cdigests"] == 32 * 65537


@pytest.mark.parametrize("size", [300_000, 1_048_576])
def test_sampling_gap(size):
    """cas.rs:31-58 reads the header, four samples and the footer: offset 18,432 (the byte after
    the first sample) and size - 8,193 (the byte before the footer) are in no window, their
    neighbours 18,431 and size - 8,192 are."""
    plan = py_sample_plan(size)

    def sampled(off):
        return any(o <= off < o + ln for o, ln in plan)
    assert not sampled(18_432) and not sampled(size - 8_193)
    assert sampled(18_431) and sampled(size - 8_192)
    covered = set()
    for o, ln in plan:
        covered.update(range(o, o + ln))
    assert len(covered) == 57_344
    assert size - len(covered) == {300_000: 242_656, 1_048_576: 991_232}[size]
    unsampled = sorted(set(range(size)) - covered)
    assert unsampled[0] == 18_432
    if size == 300_000:
        assert unsampled[-1] == 291_807
