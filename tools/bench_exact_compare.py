#!/usr/bin/env python3
"""What splitting candidate sets by comparison costs on one GPU, against the digest route.

Leg A is what the library offered before: checksums_dev (whole-content BLAKE3 of every row) +
group_exact on the same arena and rep.  Leg B is group_exact_contents.  The outputs are compared
for equality before anything is timed; then the legs alternate in one process, each figure the
median of 20 calls after a warm-up, host clock around a call that ends in a device synchronise
(both legs block by themselves).  One JSON line per shape:

  small   1 M files of U(0, 16) KiB, 30 % of them copies of an earlier file (the validator's
          small-file shape)
  pairs   64 files of 1 GiB as 32 pairs, all equal
  tails   the same with a difference in the last byte of each copy

Leg B's bytes are the ones the algorithm needs: each entry once plus each pivot once per run of
its window; bytes / time is set against the 6.0-6.3 TB/s a streaming kernel reaches on this
part.  --scale F shrinks every shape by F (a smoke run).

--sweep: the round cap.  Classes of d = 2, 3, 4, 8, 16 distinct contents, four rows each, at
1 MiB and 64 MiB per file, the differences in the first piece or in the last; each input under
max_rounds = 0 (no cap), 1, 2, 3, 4, 8: median of 5.  Where finishing by digest beats one more
round, the capped call is the faster one."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacedrive_amd import CasEngine  # noqa: E402

REPS, WARM = 20, 3
STREAM_BYTES_PER_S = (6.0e12, 6.3e12)
RUN_K = 16


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def needed_bytes(rep, lens):
    """entries once + pivots once per run: rows ordered by (pivot, row), windows of RUN_K"""
    first = {}
    piv = np.array([first.setdefault((int(r), int(ln)), i) for i, (r, ln) in enumerate(zip(rep, lens))])
    ent = np.flatnonzero(piv != np.arange(len(rep)))
    ent = ent[np.argsort(piv[ent], kind="stable")]
    p = piv[ent]
    starts = np.ones(len(ent), dtype=bool)
    starts[1:] = (p[1:] != p[:-1]) | (np.arange(1, len(ent)) % RUN_K == 0)
    return int(lens[ent].sum() + lens[p[starts]].sum()), len(ent)


class Shape:
    def __init__(self, name, lens, src, flip_last=False, seed=1):
        """lens[i] bytes per row; src[i] = the row whose content row i copies (itself: fresh)"""
        self.name, n = name, len(lens)
        room = (lens.astype(np.int64) + 15) & ~15
        offs = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64)
        total = int(room.sum())
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.arena = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")
        step = 1 << 30
        for at in range(0, total, step):  # fresh bytes everywhere (the padding too), then the copies
            m = min(step, total - at)
            self.arena[at:at + m] = torch.randint(0, 256, (m,), dtype=torch.uint8, device="cuda", generator=g)
        for i in np.flatnonzero(src != np.arange(n)).tolist():
            s, ln = int(src[i]), int(lens[i])
            self.arena[offs[i]:offs[i] + ln] = self.arena[offs[s]:offs[s] + ln]
            if flip_last and ln:
                self.arena[offs[i] + ln - 1] ^= 0xFF
        self.total, self.n = total, n
        self.rep_h, self.lens_h = src.astype(np.uint32), lens.astype(np.int64)
        self.rep = torch.from_numpy(self.rep_h.view(np.int32)).cuda()
        self.offs = torch.from_numpy(offs).cuda()
        self.lens = torch.from_numpy(self.lens_h).cuda()
        self.dig = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        self.out = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in "AB"}
        self.objects = {}

    def leg_a(self, eng):
        eng.checksums_dev(self.arena, self.offs, self.lens, self.dig, arena_bytes=self.total)
        self.objects["A"] = eng.group_exact(self.rep, self.dig, self.out["A"])

    def leg_b(self, eng):
        self.objects["B"] = eng.group_exact_contents(self.rep, self.arena, self.offs, self.lens, self.out["B"],
                                                      arena_bytes=self.total)


def measure(eng, sh, reps=REPS):
    sh.leg_a(eng)
    sh.leg_b(eng)
    identical = bool(torch.equal(sh.out["A"], sh.out["B"])) and sh.objects["A"] == sh.objects["B"]
    counters = eng.exact_compare_counters()
    ts = {"A": [], "B": []}
    for it in range(WARM + reps):
        for k, fn in (("A", sh.leg_a), ("B", sh.leg_b)):
            t = once(lambda: fn(eng))
            if it >= WARM:
                ts[k].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    need, entries = needed_bytes(sh.rep_h, sh.lens_h)
    rate = need / (med["B"] * 1e-3)
    return {"shape": sh.name, "rows": sh.n, "arena_bytes": sh.total, "objects": sh.objects["B"],
            "identical": identical, "reps": reps, "digest_ms": med["A"], "compare_ms": med["B"],
            "digest_ms_min_max": [min(ts["A"]), max(ts["A"])], "compare_ms_min_max": [min(ts["B"]), max(ts["B"])],
            "compare_over_digest": med["B"] / med["A"], "entries": entries, "compare_needed_bytes": need,
            "compare_bytes_per_s": rate, "of_streaming_rate": [rate / STREAM_BYTES_PER_S[1], rate / STREAM_BYTES_PER_S[0]],
            "rounds_compares_unequal_digest_rows": counters}


def shapes(scale):
    rng = np.random.default_rng(1)
    n = max(1000, int(1_000_000 / scale))
    lens = rng.integers(0, 16 * 1024 + 1, n)
    src = np.arange(n)
    copies = np.flatnonzero(rng.random(n) < 0.30)
    copies = copies[copies > 0]
    src[copies] = (rng.random(len(copies)) * copies).astype(np.int64)
    while True:  # a copy of a copy names the fresh row at the end of its chain
        nxt = src[src]
        if (nxt == src).all():
            break
        src = nxt
    lens = lens[src]
    yield lambda: Shape("small", lens, src)
    pairs, size = max(2, int(32 / scale)), (1 << 30) // max(1, int(scale))
    big = np.full(2 * pairs, size)
    bsrc = np.arange(2 * pairs) & ~1
    yield lambda: Shape("pairs", big, bsrc)
    yield lambda: Shape("tails", big, bsrc, flip_last=True)


def sweep_input(d, size, where, budget):
    """classes of d distinct contents x 4 rows, `budget` bytes in all; differences in the first or
    the last piece"""
    classes = max(1, budget // (4 * d * size))
    n = classes * 4 * d
    lens = np.full(n, size)
    src = (np.arange(n) // (4 * d)) * (4 * d)  # every row a copy of its class's first ...
    sh = Shape(f"sweep d={d} size={size} {where}", lens, src)
    offs = sh.offs.cpu().numpy()
    for i in range(n):  # ... then content j of d marked at one byte
        j = (i % (4 * d)) % d
        at = j if where == "first" else size - 1 - j
        if j:
            sh.arena[offs[i] + at] ^= 0x5A
    return sh


def sweep(eng, scale):
    for size in (1 << 20, 64 << 20):
        for d in (2, 3, 4, 8, 16):
            for where in ("first", "last"):
                sh = sweep_input(d, size, where, int((4 << 30) / scale))
                sh.leg_a(eng)
                res = {"input": sh.name, "rows": sh.n, "digest_route_ms": float(np.median([once(lambda: sh.leg_a(eng)) for _ in range(5)]))}
                for cap in (0, 1, 2, 3, 4, 8):
                    eng.set_exact_compare_rounds(cap)
                    sh.leg_b(eng)
                    ok = bool(torch.equal(sh.out["A"], sh.out["B"]))
                    ts = [once(lambda: sh.leg_b(eng)) for _ in range(5)]
                    res[f"cap{cap}_ms"] = float(np.median(ts))
                    res[f"cap{cap}_min_max"] = [min(ts), max(ts)]
                    res[f"cap{cap}_counters"] = eng.exact_compare_counters()
                    res["identical"] = res.get("identical", True) and ok
                print(json.dumps(res), flush=True)
                del sh
    eng.set_exact_compare_rounds(None)


def main():
    args = sys.argv[1:]
    scale = float(args[args.index("--scale") + 1]) if "--scale" in args else 1.0
    eng = CasEngine(0)
    if "--sweep" in args:
        sweep(eng, scale)
        return
    for make in shapes(scale):
        sh = make()
        print(json.dumps(measure(eng, sh)), flush=True)
        del sh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
