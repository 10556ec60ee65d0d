#!/usr/bin/env python3
"""What the exact duplicate grouping costs on one GPU: sd_cas_group_dev on the cas keys against
sd_cas_group_exact_dev on the same rows (prior rep = that grouping, one 32-byte digest per
content) under EXACT_AUTO and EXACT_WORDS, at the bench's per-GPU batch (1,310,720 rows) and
config 4's rank share (12,500,000), 30 % copies.  The three are timed alternately in one
process, each figure the median of 20 calls after a warm-up, host clock around a call that ends
in a device synchronise (group_exact blocks by itself).  One JSON line per size.

The HBM model counts the bytes per row beyond the inner grouping — key build 36 B read + 8 B
written, verify 4 B plus 68 B per non-head row — at 8 TB/s.

--group-only: time sd_cas_group_dev alone (with SD_HIP_CAS_LIB = another build of the library,
e.g. the parent commit's, for the same-session comparison)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacedrive_amd import CasEngine  # noqa: E402

REPS, WARM = 20, 3
HBM_BYTES_PER_S = 8e12


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    args = sys.argv[1:]
    group_only = "--group-only" in args
    args = [a for a in args if a != "--group-only"]
    eng = CasEngine(0)
    rng = np.random.default_rng(1)
    for n in [int(x) for x in (args or ["1310720", "12500000"])]:
        uniq = int(n * 0.7)
        content = np.concatenate([np.arange(uniq), rng.integers(0, uniq, n - uniq)])
        rng.shuffle(content)
        keys = torch.from_numpy(rng.integers(0, 2 ** 63, uniq, dtype=np.int64)[content]).cuda()
        rep = torch.empty(n, dtype=torch.int32, device="cuda")
        fns = {"group": lambda: eng.group(keys, rep, want_objects=False)}
        objects = eng.group(keys, rep)
        if not group_only:
            dig = torch.from_numpy(rng.integers(0, 256, (uniq, 32), dtype=np.uint8)).cuda()[
                torch.from_numpy(content).cuda()].contiguous().view(-1)
            out = {m: torch.empty(n, dtype=torch.int32, device="cuda") for m in ("auto", "words")}
            got = {}

            def exact(name, method):
                eng.set_exact_method(method)
                got[name] = eng.group_exact(rep, dig, out[name])
            fns["auto"] = lambda: exact("auto", eng.EXACT_AUTO)
            fns["words"] = lambda: exact("words", eng.EXACT_WORDS)
        ts = {k: [] for k in fns}
        for it in range(WARM + REPS):  # alternating: drift and other tenants hit all three alike
            for k, fn in fns.items():
                t = once(fn)
                if it >= WARM:
                    ts[k].append(t)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res = {"rows": n, "objects": objects, "reps": REPS, "group_ms": med["group"],
               "group_ms_min_max": [min(ts["group"]), max(ts["group"])]}
        if not group_only:
            eng.set_exact_method(eng.EXACT_AUTO)
            mism, fallbacks = 0, 0
            exact("auto", eng.EXACT_AUTO)
            mism, fallbacks = eng.group_exact_counters()
            extra_bytes = n * (36 + 8 + 4) + 68 * (n - objects)
            model_ms = extra_bytes / HBM_BYTES_PER_S * 1e3
            over = med["auto"] - med["group"]
            res.update({
                "exact_auto_ms": med["auto"], "exact_words_ms": med["words"],
                "exact_auto_ms_min_max": [min(ts["auto"]), max(ts["auto"])],
                "auto_over_group": med["auto"] / med["group"], "words_over_group": med["words"] / med["group"],
                "auto_overhead_ms": over, "hbm_model_extra_bytes": extra_bytes, "hbm_model_ms": model_ms,
                "overhead_fraction_of_hbm_model": model_ms / over if over > 0 else None,
                "overhead_exceeds_inner_grouping": over > med["group"],
                "fallbacks": fallbacks, "mismatched_rows": mism,
                "identical": bool(torch.equal(out["auto"], out["words"])) and bool(torch.equal(out["auto"], rep))
                and got["auto"] == got["words"] == objects})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
