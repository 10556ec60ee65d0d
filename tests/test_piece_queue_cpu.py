"""The validator's piece queue (spacedrive_amd/csrc/sd_piece_queue.h) on the CPU: the cutter,
the reader on real files and the engine on a real HostPool over a fake device
(tests/native/piece_queue_test.cpp lists what is asserted).  The program is built twice, plain
and with the thread sanitizer, and each build is run directly under a time limit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def build(exe, *flags):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    cc = [HIPCC, "-O2", "-g", "-std=c++17", "-pthread", *flags, "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "piece_queue_test.cpp"), "-o", exe]
    return subprocess.run(cc, capture_output=True, text=True, timeout=300)


def run(exe, tmp_path, **env):
    scratch = tmp_path / "files"
    scratch.mkdir(exist_ok=True)
    r = subprocess.run([exe, str(scratch)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, **env})
    assert r.returncode == 0 and "piece queue ok" in r.stdout, r.stdout + r.stderr
    return r


def test_piece_queue(tmp_path):
    exe = str(tmp_path / "piece_queue_test")
    b = build(exe)
    assert b.returncode == 0, b.stderr
    run(exe, tmp_path)


def test_piece_queue_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "piece_queue_test_tsan")
    b = build(exe, "-fsanitize=thread")
    if b.returncode != 0 and ("libclang_rt.tsan" in b.stderr or "tsan" in b.stderr.lower()):
        pytest.skip("the thread sanitizer build failed for lack of its runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr
    r = run(exe, tmp_path, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    assert "ThreadSanitizer" not in r.stderr, r.stderr
