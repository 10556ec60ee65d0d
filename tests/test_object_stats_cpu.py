"""Object statistics (sd_cas_object_stats_dev / sd_cas_top_duplicates_dev /
sd_cas_duplicate_report), the part that needs no GPU: the ABI header declares the three entry
points and the SD_CAS_STAT_* indices, CasEngine mirrors them, and the numpy restatement the GPU
tests compare against (np_group / np_stats / np_top, below) agrees with an 8-row example
worked by hand."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_NAMES = ("rows", "objects", "total_bytes", "unique_bytes", "duplicate_sets", "max_copies",
              "size_mismatch_rows", "bad_rows")
NO_OBJECT = 0xFFFFFFFF
M64 = (1 << 64) - 1


# ---- the numpy restatement of the definitions ----------------------------------------------
def np_group(keys):
    """rep[i] = the first row with row i's key, copies[i] = the rows with it."""
    _, first, inv, counts = np.unique(np.asarray(keys, dtype=np.uint64), return_index=True,
                                      return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    return first[inv].astype(np.uint32), counts[inv].astype(np.uint32)


def np_stats(rep, sizes, hashed=None):
    """(copies, totals dict) of any rep array, bad rows included: a row is valid iff
    rep[i] <= i and rep[rep[i]] == rep[i]; rows with hashed[i] False take no part."""
    rep = np.asarray(rep, dtype=np.uint32).astype(np.int64)
    sizes = np.asarray(sizes, dtype=np.uint64)
    n = len(rep)
    i = np.arange(n, dtype=np.int64)
    part = np.ones(n, dtype=bool) if hashed is None else np.asarray(hashed, dtype=bool)
    inb = part & (rep <= i)
    safe = np.where(inb, rep, 0)
    valid = inb & (rep[safe] == rep) if n else inb
    per_head = np.bincount(rep[valid], minlength=max(n, 1))
    copies = np.where(valid, per_head[safe], 0).astype(np.uint32)
    head = valid & (rep == i)
    nonhead = valid & ~head
    t = {
        "rows": int(valid.sum()),
        "objects": int(head.sum()),
        "total_bytes": sum(sizes[valid].tolist()) & M64,
        "unique_bytes": sum(sizes[head].tolist()) & M64,
        "duplicate_sets": int((head & (copies >= 2)).sum()),
        "max_copies": int(copies.max()) if valid.any() else 0,
        "size_mismatch_rows": int((sizes[nonhead] != sizes[safe[nonhead]]).sum()),
        "bad_rows": int((part & ~valid).sum()),
    }
    return copies, t


def np_top(rep, sizes, copies, k):
    """The top list: (heads, waste) of length k, sentinels past the sets found, and found."""
    rep = np.asarray(rep, dtype=np.uint32)
    heads = np.nonzero((rep == np.arange(len(rep), dtype=np.uint32)) & (np.asarray(copies) >= 2))[0]
    sets = [(((int(copies[h]) - 1) * int(sizes[h])) & M64, int(h)) for h in heads]
    sets = sorted(sets, key=lambda s: (-s[0], s[1]))[:k]
    found = len(sets)
    th = np.array([h for _, h in sets] + [NO_OBJECT] * (k - found), dtype=np.uint32)
    tw = np.array([w for w, _ in sets] + [0] * (k - found), dtype=np.uint64)
    return th, tw, found


# ---- tests ----------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "sd_hip_cas.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_three_functions():
    text, code = _header()
    for name in ("sd_cas_object_stats_dev", "sd_cas_top_duplicates_dev", "sd_cas_duplicate_report"):
        assert re.search(r"\bint\s+%s\s*\(\s*sd_cas_ctx\s*\*" % name, code), name
    # each entry's comment cites the slot the reference leaves empty
    sect = text[text.index("Object statistics"):text.index("sd_cas_sort_pairs_dev")]
    assert sect.count("statistics.rs:42,46") >= 3 and sect.count("schema.prisma:83,87") >= 3


def test_stat_defines():
    _, code = _header()
    d = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SD_CAS_\w+)\s+(\d+)\s*$", code, flags=re.M)}
    for idx, name in enumerate(STAT_NAMES):
        assert d["SD_CAS_STAT_" + name.upper()] == idx
    assert d["SD_CAS_STAT_COUNT"] == 8
    assert d["SD_CAS_TOP_MAX"] == 65536


def test_python_mirror():
    from spacedrive_amd import _native, cas
    for m in ("object_stats", "top_duplicates", "duplicate_report"):
        assert callable(getattr(cas.CasEngine, m))
    assert cas.STAT_NAMES == STAT_NAMES and cas.TOP_MAX == 65536
    # the compaction tile documented next to the kernel
    hdr = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "sd_object_stats.h")).read()
    th, ti = (int(re.search(r"%s = (\d+)" % q, hdr).group(1)) for q in ("TOP_THREADS", "TOP_ITEMS"))
    assert cas.TOP_TILE == th * ti
    table = {n for n, _, _ in _native.SIGNATURES}
    assert {"sd_cas_object_stats_dev", "sd_cas_top_duplicates_dev", "sd_cas_duplicate_report"} <= table


def test_numpy_restatement_on_a_hand_worked_example():
    # row:    0   1   2   3   4   5   6   7
    keys = [7, 3, 7, 9, 3, 7, 5, 9]
    sizes = [10, 20, 10, 30, 20, 10, 40, 30]
    # key 7 -> rows 0,2,5 (head 0); key 3 -> rows 1,4 (head 1); key 9 -> rows 3,7 (head 3);
    # key 5 -> row 6 alone
    rep, copies = np_group(keys)
    assert rep.tolist() == [0, 1, 0, 3, 1, 0, 6, 3]
    assert copies.tolist() == [3, 2, 3, 2, 2, 3, 1, 2]
    c2, t = np_stats(rep, sizes)
    assert c2.tolist() == copies.tolist()
    assert t == {"rows": 8, "objects": 4, "total_bytes": 170, "unique_bytes": 10 + 20 + 30 + 40,
                 "duplicate_sets": 3, "max_copies": 3, "size_mismatch_rows": 0, "bad_rows": 0}
    # waste: head 0 -> 2 x 10 = 20, head 1 -> 1 x 20 = 20, head 3 -> 1 x 30 = 30
    th, tw, found = np_top(rep, sizes, copies, 2)
    assert (th.tolist(), tw.tolist(), found) == ([3, 0], [30, 20], 2)
    th, tw, found = np_top(rep, sizes, copies, 5)
    assert (th.tolist(), tw.tolist(), found) == ([3, 0, 1, NO_OBJECT, NO_OBJECT], [30, 20, 20, 0, 0], 3)
    # a stale size on row 4, and three bad rows: 2 points forward, 7 points at a non-head,
    # 5 points past the end — each counted in bad_rows only, copies 0
    bad = rep.copy()
    bad[2], bad[7], bad[5] = 3, 2, 200
    sz = list(sizes)
    sz[4] = 21
    c3, t3 = np_stats(bad, sz)
    assert c3.tolist() == [1, 2, 0, 1, 2, 0, 1, 0]
    assert t3 == {"rows": 5, "objects": 4, "total_bytes": 10 + 20 + 30 + 21 + 40, "unique_bytes": 100,
                  "duplicate_sets": 1, "max_copies": 2, "size_mismatch_rows": 1, "bad_rows": 3}
    # rows that are not hashed take no part
    c4, t4 = np_stats(rep, sizes, hashed=[True, True, False, True, True, True, True, True])
    assert c4.tolist() == [2, 2, 0, 2, 2, 2, 1, 2] and t4["rows"] == 7 and t4["bad_rows"] == 0
