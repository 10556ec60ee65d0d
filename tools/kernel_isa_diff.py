#!/usr/bin/env python3
"""Compare the kernels of two builds by their device assembly text.

    hipcc --offload-arch=gfx950 <FLAGS of csrc/Makefile> --cuda-device-only -S x.hip -o x.s
    kernel_isa_diff.py --a old/x.s --b new/x.s new/y.s

Each side is one or more assembly files.  They are split at function symbols, the numbers of the
basic-block labels (.LBB<k>_<j>: k counts the functions of a file) and the `;` comments are
normalised away, and every function of either side is reported as SAME, or DIFFERS with the first
differing lines, or as present on one side only.  Under each function stand the resource figures
that the assembler printed for it (registers, LDS and scratch bytes, occupancy, code length).
Text is compared and nothing else: no instruction is looked for.  Exit status 0: every function
is on both sides, SAME, with equal resource figures.
"""
import argparse
import re
import sys

TYPE_FUNCTION = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
BLOCK_LABEL = re.compile(r"\.LBB\d+_")
RESOURCE = re.compile(r"^;\s*([A-Za-z_0-9:]+)\s*[:=]\s*(\d+)")
RESOURCE_KEYS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy",
                 "codeLenInByte")


def normalise(line):
    """One line without its comment, with block labels renumbered; '' for a line that was only
    a comment or blank."""
    line = line.split(";", 1)[0].rstrip()
    return BLOCK_LABEL.sub(".LBB_", line)


def split_functions(text):
    """{symbol: (normalised body lines, {resource key: value})} of one assembly file.  A body runs
    from the symbol's label to its .Lfunc_end label; the resource figures are the `; key: value`
    comment lines between that and the next function."""
    out = {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = TYPE_FUNCTION.match(lines[i])
        i += 1
        if not m:
            continue
        sym = m.group(1)
        while i < len(lines) and not lines[i].startswith(sym + ":"):
            i += 1
        body = []
        i += 1
        while i < len(lines) and not FUNC_END.match(lines[i]):
            ln = normalise(lines[i])
            if ln:
                body.append(ln)
            i += 1
        res = {}
        while i < len(lines) and not TYPE_FUNCTION.match(lines[i]):
            r = RESOURCE.match(lines[i])
            if r and r.group(1) in RESOURCE_KEYS:
                res[r.group(1)] = int(r.group(2))
            i += 1
        out[sym] = (body, res)
    return out


def first_difference(a, b, context=3):
    """(index, lines of a, lines of b) at the first index where the bodies differ, or None."""
    n = min(len(a), len(b))
    k = next((j for j in range(n) if a[j] != b[j]), n)
    if k == n and len(a) == len(b):
        return None
    return k, a[k:k + context], b[k:k + context]


def load(paths):
    funcs = {}
    for p in paths:
        with open(p) as f:
            for sym, v in split_functions(f.read()).items():
                if sym in funcs:
                    sys.exit(f"{sym} is defined twice among {paths}")
                funcs[sym] = v
    return funcs


def res_text(res):
    return " ".join(f"{k}={res[k]}" for k in RESOURCE_KEYS if k in res)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--a", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--b", nargs="+", required=True, metavar="FILE.s")
    args = ap.parse_args()
    A, B = load(args.a), load(args.b)
    bad = 0
    for sym in list(A) + [s for s in B if s not in A]:
        if sym not in A or sym not in B:
            print(f"ONLY IN {'A' if sym in A else 'B'}  {sym}")
            bad += 1
            continue
        (ba, ra), (bb, rb) = A[sym], B[sym]
        d = first_difference(ba, bb)
        print(f"{'SAME    ' if d is None else 'DIFFERS '} {sym}  ({len(ba)} / {len(bb)} lines)")
        if d is not None:
            bad += 1
            if len(ba) == len(bb):
                print(f"    {sum(x != y for x, y in zip(ba, bb))} lines differ")
            print(f"    first difference at line {d[0]} of the normalised text:")
            for ln in d[1]:
                print(f"    a| {ln}")
            for ln in d[2]:
                print(f"    b| {ln}")
        if ra == rb:
            print(f"    resources equal: {res_text(ra)}")
        else:
            bad += 1
            print(f"    resources a: {res_text(ra)}\n    resources b: {res_text(rb)}")
    print(f"{len(A)} functions in a, {len(B)} in b, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
