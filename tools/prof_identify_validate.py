#!/usr/bin/env python3
"""cas_id + file_checksum from one read per file (sd_cas_identify_validate_paths) and K1P
alone (sd_cas_hash_contents_dev), measured against what the same library — or another build
of it given in SD_HIP_CAS_LIB, e.g. the parent commit's — does without them.

--paths N   N tmpfs files, half U(1, 100) KiB and half U(100 KiB, 4 MiB) (--root), one cold
            pass and --runs warm ones of each of
              fused     identify_validate(paths)                     (skipped if the library lacks it)
              checksums file_checksums(paths)                        (a)
              two_reads file_metadata_from_paths + file_checksums    (b)
            interleaved run by run; prints the warm medians and, with the fused leg, its
            ratios to (a) and (b) and an element-for-element comparison of the outputs.
--k1p       n = 100 and 1,280 sampled files of U(1, 4) MiB resident in HBM: hash_contents
            (classify + the bounds verdict's round trip + K1P) against K1L with a wave per file
            on the same files pre-gathered into 57,344-B rows, by HIP events; the kernels' own
            times come from a kernel trace of this run (rocprofv3 --kernel-trace --stats).
Run one process per library: SD_HIP_CAS_LIB is read when the package is imported."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def make_files(orc, n, root):
    import numpy as np
    rng = np.random.default_rng(16)
    os.makedirs(root, exist_ok=True)
    sizes = np.where(rng.random(n) < 0.5, rng.integers(1 << 10, 100 << 10, n),
                     rng.integers((100 << 10) + 1, 4 << 20, n))
    paths = []
    for i, ln in enumerate(sizes):
        p = os.path.join(root, f"iv{i}")
        with open(p, "wb") as fh:
            fh.write(orc.fill_content_range(89, i, 0, (int(ln) + 7) // 8 * 8).tobytes()[:int(ln)])
        paths.append(p)
    return paths, [int(x) for x in sizes]


def paths_run(eng, orc, n, root, runs):
    import numpy as np
    paths, sizes = make_files(orc, n, root)
    total = sum(sizes)
    fused_ok = hasattr(eng.L, "sd_cas_identify_validate_paths")
    legs = {"checksums": lambda: eng.file_checksums(paths),
            "two_reads": lambda: (eng.file_metadata_from_paths(paths), eng.file_checksums(paths))}
    if fused_ok:
        legs["fused"] = lambda: eng.identify_validate(paths)
    eng.file_checksums(paths[:8])
    times = {k: [] for k in legs}
    last = {}
    for _ in range(runs + 1):  # pass 0: cold (just-written files, first-use allocations)
        for k, fn in legs.items():
            t = time.perf_counter()
            last[k] = fn()
            times[k].append(time.perf_counter() - t)
    out = {"lib": os.environ.get("SD_HIP_CAS_LIB") or "in-tree", "files": n, "bytes": total,
           "sampled_files": int(sum(s > (100 << 10) for s in sizes)), "runs": runs}
    for k in legs:
        warm = times[k][1:]
        out[k] = {"cold_s": times[k][0], "warm_s": warm, "warm_median_s": median(warm),
                  "warm_median_gb_per_s": total / median(warm) / 1e9,
                  "warm_median_files_per_s": n / median(warm)}
    if fused_ok:
        keys, cst, szs, dig, errs = last["fused"]
        (k2, s2, z2), (d2, e2) = last["two_reads"]
        out["same_outputs"] = bool((keys == k2).all() and (cst == s2).all() and (szs == z2).all()
                                   and dig == d2 and (errs == e2).all())
        idx = sorted(set(np.random.default_rng(1).integers(0, n, 48).tolist()))
        out["oracle_sample"] = bool(all(
            f"{int(keys[i]):016x}" == orc.generate_cas_id(paths[i], sizes[i])
            and dig[i] == orc.file_checksum(paths[i]) for i in idx))
        out["fused_over_checksums"] = out["fused"]["warm_median_s"] / out["checksums"]["warm_median_s"]
        out["fused_over_two_reads"] = out["fused"]["warm_median_s"] / out["two_reads"]["warm_median_s"]
    for p in paths:
        os.unlink(p)
    return out


def k1p_run(eng, orc, n, iters):
    import numpy as np
    import torch
    rng = np.random.default_rng(17)
    lens = rng.integers(1 << 20, 4 << 20, n).astype(np.uint64)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum((lens[:-1] + 15) // 16 * 16)
    ab = int(offs[-1] + lens[-1]) // 16 * 16 + 32
    arena = torch.empty(ab, dtype=torch.uint8, device="cuda")
    eng.synth_stream(90, 0, 0, ab // 8 * 8, arena)
    # the same files gathered into rows for K1L (on the device: the plan's six ranges)
    rows = torch.empty((n, 57344), dtype=torch.uint8, device="cuda")
    for i in range(n):
        g = 0
        for o, ln in orc.sample_plan(int(lens[i])):
            rows[i, g:g + ln] = arena[int(offs[i]) + o:int(offs[i]) + o + ln]
            g += ln
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int64)).cuda()
    k_in = torch.zeros(n, dtype=torch.int64, device="cuda")
    k_row = torch.zeros(n, dtype=torch.int64, device="cuda")
    eng.set_latency_threshold(1 << 40, 1 << 40)  # K1L ...
    eng.set_chunkpar_split(1 << 40, 1 << 40)     # ... a wave per file
    s = torch.cuda.current_stream()

    def timed(fn):
        fn()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return median(ts)
    t_in = timed(lambda: eng.hash_contents(arena, d_offs, d_lens, k_in, stream=s.cuda_stream))
    t_row = timed(lambda: eng.hash_sampled(rows, d_lens, k_row, stream=s.cuda_stream))
    torch.cuda.synchronize()
    same = bool((k_in == k_row).all())
    del arena, rows
    torch.cuda.empty_cache()
    return {"files": n, "hash_contents_ms": t_in, "k1l_rows_ms": t_row, "same_keys": same,
            "note": "hash_contents_ms includes classify and the host round trip of the bounds "
                    "verdict; kernel times: the kernel trace of this run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--root", default="/dev/shm/sdcas_identify_validate")
    ap.add_argument("--k1p", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from oracle.pyoracle import Oracle
    from spacedrive_amd import CasEngine
    eng, orc = CasEngine(0), Oracle()
    if a.paths:
        print(json.dumps(paths_run(eng, orc, a.paths, a.root, a.runs)), flush=True)
    if a.k1p:
        for n in (100, 1280):
            print(json.dumps(k1p_run(eng, orc, n, a.iters)), flush=True)


if __name__ == "__main__":
    main()
