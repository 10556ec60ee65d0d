"""A plain `bench.py` run on the GPU: the headline line alone, --steps honoured, and the
--dump-outputs arrays equal to the oracle's keys and canonical grouping of the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.pyoracle import SAMPLED_CONTENT_LEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "sustained", "e2e", "group", "cpu_baseline", "vs_baseline")


@pytest.mark.gpu
def test_plain_run_headline_and_dump(eng, oracle, tmp_path):
    n, steps = eng.batch_quantum, 3   # one quantum: the fused chain, as the default run
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SD_BENCH_ONE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "1", "--files-per-gpu", str(n),
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["n_gpus"] == 1 and line["config"]["grouping"] == "fused"
    assert line["unit"] == "cas_ids/s" and line["dtype"] == "u32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(tmp_path)) == ["keys.npy", "rep.npy"]
    dk, dr = np.load(tmp_path / "keys.npy"), np.load(tmp_path / "rep.npy")
    assert dk.dtype == dr.dtype == np.float64 and dk.shape == (n, 2) and dr.shape == (n,)
    keys = (dk[:, 0].astype(np.uint64) << np.uint64(32)) | dk[:, 1].astype(np.uint64)
    # the same files again (bench.py's default seed and duplicate rate), hashed by the oracle
    content = torch.empty((n, SAMPLED_CONTENT_LEN), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    eng.synth_sampled(0x5DCA50004, 0, n, content, sizes, SAMPLED_CONTENT_LEN, dup_permille=300)
    idx = np.sort(np.random.default_rng(4).choice(n, 1024, replace=False))
    sub = content[torch.from_numpy(idx).cuda()].cpu().numpy()
    want = oracle.fast_cas_keys_strided(sub.reshape(-1), SAMPLED_CONTENT_LEN, SAMPLED_CONTENT_LEN,
                                        sizes.cpu().numpy().view(np.uint64)[idx], 8)
    assert (keys[idx] == want).all()
    orep, oobj = oracle.group_canonical(keys)
    assert oobj < n and (dr == orep).all()
