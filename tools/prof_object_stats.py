#!/usr/bin/env python3
"""Object statistics (sd_cas_object_stats_dev) and the top list (sd_cas_top_duplicates_dev,
k = 100) beside the grouping (sd_cas_group_dev) that produced their input, on device-resident
rows: 1,310,720 and 12,500,000 rows x three inputs — 30 % duplicates (synth_roots,
dup_permille=300, sizes from the roots), all distinct, one hot key covering every row.

Method: every shape is warmed up first; then ROUNDS interleaved rounds, each timing the three
calls one after the other, so drift of the clock or of the shared host hits all three alike.
group and object_stats are asynchronous: INNER back-to-back calls between two device events,
divided by INNER.  top_duplicates blocks (one read-back inside): host clock around the call
after a device synchronise.  Reported: median and min..max over the rounds, and for
object_stats the algorithmic rate at 30 B/row.  Writes one text table (--out)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from spacedrive_amd import CasEngine  # noqa: E402

ROUNDS, INNER, K = 15, 10, 100
STATS_BYTES_PER_ROW = 30  # rep 4 x 3 passes, copies 4 w + 4 r + 4 r, sizes 8, ~2 of gathers

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "object_stats", "measurements.txt"))
ap.add_argument("--commit", default="unknown")
ap.add_argument("--rows", type=int, nargs="*", default=[1_310_720, 12_500_000])
args = ap.parse_args()

assert torch.cuda.is_available(), "this profile needs the GPU"
eng = CasEngine(0)
props = torch.cuda.get_device_properties(0)


def clocks() -> str:
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30)
        lines = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(lines) or "not reported"
    except Exception as e:  # noqa: BLE001
        return f"not reported ({type(e).__name__})"


def inputs(kind: str, n: int):
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    if kind == "dup30":
        eng.synth_roots(0x0B57A7, 0, n, keys, dup_permille=300)
        sizes = ((keys * 2654435761) & 0xFFFFFFFFFF) + 1
    elif kind == "distinct":
        keys = torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * -7046029254386353131
        sizes = ((keys >> 7) & 0xFFFFFFFFFF) + 1
    else:  # hot: one key covers every row
        keys.fill_(0x1234567)
        sizes = torch.full((n,), 1 << 20, dtype=torch.int64, device="cuda")
    return keys, sizes


def ev_time(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


def host_time(fn) -> float:
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def fmt(ts) -> str:
    return f"{statistics.median(ts):9.4f} ms  ({min(ts):.4f} .. {max(ts):.4f})"


lines = [
    "object statistics beside the grouping: ms per call, median (min .. max) over "
    f"{ROUNDS} interleaved rounds",
    f"card: {props.name}, {props.multi_processor_count} CUs; clocks: {clocks()}",
    f"commit: {args.commit}; torch {torch.__version__}; group / object_stats: {INNER} calls between "
    "device events; top_duplicates (k = 100): host clock, blocking",
    "",
]
for n in args.rows:
    for kind in ("dup30", "distinct", "hot"):
        keys, sizes = inputs(kind, n)
        rep = torch.empty(n, dtype=torch.int32, device="cuda")
        copies = torch.empty(n, dtype=torch.int32, device="cuda")
        totals = torch.empty(8, dtype=torch.int64, device="cuda")
        heads = torch.empty(K, dtype=torch.int32, device="cuda")
        waste = torch.empty(K, dtype=torch.int64, device="cuda")

        def f_group():
            eng.group(keys, rep, want_objects=False)

        def f_stats():
            eng.object_stats(rep, sizes, copies, totals=totals, want_totals=False)

        def f_top():
            eng.top_duplicates(rep, sizes, copies, K, heads, waste)

        for _ in range(3):  # warm-up: code objects, workspace growth
            f_group(); f_stats(); f_top()
        t = eng.object_stats(rep, sizes, copies)
        found = eng.top_duplicates(rep, sizes, copies, K, heads, waste)
        tg, ts, tt = [], [], []
        for _ in range(ROUNDS):
            tg.append(ev_time(f_group))
            ts.append(ev_time(f_stats))
            tt.append(host_time(f_top))
        ms = statistics.median(ts)
        lines += [
            f"rows {n:>10,}  input {kind:8}  objects {t['objects']:>10,}  duplicate_sets "
            f"{t['duplicate_sets']:>9,}  max_copies {t['max_copies']:>10,}  top found {found}",
            f"  group          {fmt(tg)}",
            f"  object_stats   {fmt(ts)}   {n * STATS_BYTES_PER_ROW / ms / 1e6:7.1f} GB/s at "
            f"{STATS_BYTES_PER_ROW} B/row   {ms / statistics.median(tg):.2f} x group",
            f"  top_duplicates {fmt(tt)}",
            "",
        ]
        print("\n".join(lines[-5:]), flush=True)
        del keys, sizes, rep, copies
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines))
print("wrote", args.out)
