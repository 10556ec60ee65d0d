"""The C host example examples/sd_duplicates.c: a directory's duplicate report through the C
ABI from a compiled program (walk, sd_cas_file_metadata_from_paths, sd_cas_duplicate_report).
CPU: it builds, links and loads, and without a gfx950 device it refuses to run.  GPU: its one
JSON object equals what the oracle's cas_ids and a dictionary pass over the files give."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "sd_duplicates")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "-s"], check=True)
    return EXE


def test_example_builds_and_needs_a_device(exe, tmp_path):
    import torch
    (tmp_path / "a").write_bytes(b"x" * 10)
    (tmp_path / "b").write_bytes(b"x" * 10)
    r = subprocess.run([exe, str(tmp_path), "3"], capture_output=True, text=True, timeout=120)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
        out = json.loads(r.stdout)
        assert out["totals"]["objects"] == 1 and out["top"][0]["waste"] == 10
    else:
        assert r.returncode == 1
        assert "sd_cas_ctx_create: -5" in r.stderr
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage


@pytest.mark.gpu
def test_example_report_vs_oracle(exe, oracle, tmp_path):
    rng = np.random.default_rng(23)
    d = tmp_path / "lib"
    (d / "sub").mkdir(parents=True)
    blobs = [rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in [5, 4096, 102_400, 250_000, 1_000_000]]
    for i in range(160):
        p = d / ("sub" if i % 3 == 0 else ".") / f"f{i:04d}"
        if i % 31 == 4:
            p.write_bytes(b"")  # no cas_id: one more Object of 0 bytes
        elif rng.random() < 0.45:
            p.write_bytes(blobs[int(rng.integers(0, len(blobs)))])
        else:
            p.write_bytes(rng.integers(0, 256, int(rng.integers(1, 300_000)), dtype=np.uint8).tobytes())
    k = 4
    r = subprocess.run([exe, str(d), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    paths = sorted(str(p) for p in d.rglob("*") if p.is_file())
    sets, no_cas, total = {}, 0, 0
    for p in paths:
        size = os.path.getsize(p)
        if size == 0:
            no_cas += 1
            continue
        total += size
        sets.setdefault(oracle.generate_cas_id(p, size), []).append(p)
    size_of = {c: os.path.getsize(m[0]) for c, m in sets.items()}
    dups = {c: m for c, m in sets.items() if len(m) >= 2}
    assert out["files"] == len(paths) and out["no_cas"] == no_cas and out["errors"] == 0
    assert out["total_object_count"] == len(sets) + no_cas
    assert out["total_unique_bytes"] == str(sum(size_of.values()))
    assert out["totals"] == {
        "rows": len(paths) - no_cas, "objects": len(sets), "total_bytes": total,
        "unique_bytes": sum(size_of.values()), "duplicate_sets": len(dups),
        "max_copies": max(len(m) for m in sets.values()), "size_mismatch_rows": 0, "bad_rows": 0}
    # waste descending, ties by the head's row = its first path in sorted order
    want = sorted(dups, key=lambda c: (-(len(dups[c]) - 1) * size_of[c], paths.index(dups[c][0])))[:k]
    assert len(dups) >= k and [t["cas_id"] for t in out["top"]] == want
    for t in out["top"]:
        m = dups[t["cas_id"]]
        assert t["paths"] == m and t["copies"] == len(m) and t["size"] == size_of[t["cas_id"]]
        assert t["waste"] == (len(m) - 1) * t["size"]
