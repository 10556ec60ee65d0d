"""CPU tests of the lane-side BLAKE3 message walker (spacedrive_amd/csrc/blake3_lane.hpp): the
lane program of K2 (message = le64(size) || content) and of the validator's lane kernel
(message = content), compiled for the host and run by a stand-alone program
(tests/native/lane_walker_test.cpp, its own main, nothing preloaded) — once plain, once under
the address and undefined-behaviour sanitizers — against the oracle.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from spacedrive_amd.cas import MAX_PACKED_CONTENT_LEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# every stack depth and fold the lane class can reach (<= 128 chunks, and one past)
PLAIN_LENS = list(range(0, 1101)) + [k * 1024 + d for k in range(1, 129) for d in (-1, 0, 1)]
PREFIXED_SMALL = list(range(0, 1101))
# every chunk count of the whole-file path: the message ends one byte before, at, and one
# byte past a chunk boundary (tests/test_gpu_parity.py runs the same list on the device)
PREFIXED_SWEEP = [min(max(k * 1024 - 8 + d, 0), MAX_PACKED_CONTENT_LEN)
                  for k in range(1, 105) for d in (-1, 0, 1)]


def size_of(length):
    return length if length % 3 else length * 3 + (1 << 33) + 200_000  # both words of the prefix


def content(length):
    """content_byte() of lane_walker_test.cpp"""
    i = np.arange(1, length + 1, dtype=np.uint64)
    v = (i * np.uint64(2654435761) + np.uint64(length * 0x9E3779B1 & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    return ((v >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8).tobytes()


def requests():
    return ([("p", n, 0) for n in PLAIN_LENS] + [("x", n, size_of(n)) for n in PREFIXED_SMALL + PREFIXED_SWEEP]
            + [("i", n, size_of(n)) for n in PREFIXED_SWEEP])


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                ids=["plain", "asan_ubsan"])
def digests(request, tmp_path_factory):
    """{(mode, len): digest} from one run of the stand-alone program."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("lane_walker") / "lane_walker_test")
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-x", "c++", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "lane_walker_test.cpp"), "-o", exe]
    subprocess.run(cc + request.param, check=True, capture_output=True, timeout=600)
    reqs = requests()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="".join(f"{m} {n} {s}\n" for m, n, s in reqs), capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert [(m, int(n)) for m, n, _ in rows] == [(m, n) for m, n, _ in reqs]
    return {(m, int(n)): bytes.fromhex(h) for m, n, h in rows}


def test_plain_walk_vs_oracle(digests, oracle):
    bad = [n for n in PLAIN_LENS if digests[("p", n)] != oracle.blake3(content(n))]
    assert not bad, bad[:10]


def test_prefixed_walk_vs_oracle(digests, oracle):
    lens = PREFIXED_SMALL + PREFIXED_SWEEP
    bad = [n for n in lens if digests[("x", n)] != oracle.blake3(struct.pack("<Q", size_of(n)) + content(n))]
    assert not bad, bad[:10]
    # ... and as cas keys, from an arena padded with 0xFF like the program's buffers
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += (n + 15) // 16 * 16
    arena = np.full(o + 16, 0xFF, dtype=np.uint8)
    for n, off in zip(lens, offs):
        arena[off:off + n] = np.frombuffer(content(n), np.uint8)
    want = oracle.cas_keys(arena, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64),
                           np.array([size_of(n) for n in lens], dtype=np.uint64))
    got = np.array([int.from_bytes(digests[("x", n)][:8], "big") for n in lens], dtype=np.uint64)
    assert (got == want).all(), [lens[i] for i in np.flatnonzero(got != want)[:10]]


def test_prefixed_walk_is_the_plain_walk_of_the_prefixed_bytes(digests):
    bad = [n for n in PREFIXED_SWEEP if digests[("x", n)] != digests[("i", n)]]
    assert not bad, bad[:10]
