"""CPU tests of the workspace carver (spacedrive_amd/csrc/sd_ws.h) and of every layout built on
it.  Each device chain's workspace layout is one function that both measures (null base) and
carves; tests/native/ws_layout_test.cpp prints every layout at the shapes where a plan switches,
and the totals are held to those of the last commit that spelled the layouts out by hand
(tests/golden/ws_sizes.json, made once by tests/golden/make_ws_sizes.py).  No GPU: only the pure
size / layout functions of libsd_hip_cas.so are called."""
import json
import os
import subprocess

import pytest

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = "/opt/rocm/bin/hipcc"
# the fused chain's region set: the parent's caller added 256 B for the Object counters to
# region_group_workspace_bytes(n); the layout now owns them (its `objects` member)
REGION_OBJECTS_RESERVE = 256


def _build(tmp, name, src, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp / name)
    cc = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-I", CSRC, os.path.join(NATIVE, src), "-o", exe]
    subprocess.run(cc + extra, check=True, capture_output=True, timeout=600)
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_carver_measures_what_it_carves(tmp_path, flags):
    """A stand-alone host program (its own main, nothing preloaded): null-base measuring equals
    carving from a malloc'ed base, takes are 256-aligned, disjoint and gap-free, a take of 0
    advances by 0, take<u64>(2^32 + 1) does not wrap."""
    exe = _build(tmp_path, "ws_carve_test", "ws_carve_test.cpp", flags)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ws_carve ok"


@pytest.fixture(scope="module")
def layout_lines(tmp_path_factory):
    _native.lib()  # the library must have been built
    libdir = os.path.dirname(_native.LIB_PATH)
    exe = _build(tmp_path_factory.mktemp("ws_layout"), "ws_layout_test", "ws_layout_test.cpp",
                 ["-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-L", libdir,
                  "-l:" + os.path.basename(_native.LIB_PATH), "-Wl,-rpath," + libdir,
                  "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sizes, layouts = {}, {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "S":
            sizes[f[1]] = int(f[2])
        else:
            assert f[0] == "L"
            members = []
            for m in f[4:]:
                name, off, need = m.split(":")
                members.append((name, None if off == "-" else int(off), int(need)))
            layouts[f[1]] = (int(f[2]), None if f[3] == "-" else int(f[3]), members)
    return sizes, layouts


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "ws_sizes.json")) as f:
        return json.load(f)


def test_every_shape_is_printed(layout_lines):
    sizes, layouts = layout_lines
    ns = [1, 255, 256, 257, 4095, 4096, 4097, 65536, 1441792, 1441793, 12500000, 40000001, 2 ** 32 - 1]
    for n in ns:
        for name in ("sort", "group", "group_min_sorted", "region_group", "small_regions", "big_regions",
                     "inplace", "dup_verify", "packed", "reduce_cvs"):
            assert f"{name}({n})" in layouts
        for t in (0, 1, 16):
            assert f"hash_chain({n},{t})" in layouts
        for pre in (0, 1):
            for n_seed in (0, 5):
                assert f"link_io({n},{n_seed},{pre})" in layouts
                assert f"link_staging({n},{n_seed},{(n + 99) // 100},{pre})" in layouts
    for n in (1, 65535, 65536):
        for arena in (0, 1 << 20, 64 << 30):
            assert f"checksum_batch({n},{arena})" in layouts
    for parts in (1, 1023, 1024, 16384):
        assert f"partition({parts})" in layouts
    for ns_, np_ in ((0, 1), (1, 0), (100, 0), (37, 63)):
        for plen in (0, 1, 127, 128, 102400):
            assert f"staged({ns_},{np_},{plen})" in layouts
    # the batch checksum's lane section exists from 65,536 buffers
    assert (sizes["checksum_batch_lane(65535)"], sizes["checksum_batch_lane(65536)"]) == (0, 1)


def test_members_ascend_cover_their_use_and_fit_the_total(layout_lines):
    _, layouts = layout_lines
    for key, (total, wrapper, members) in layouts.items():
        if wrapper is not None:  # (a layout without one: its total is pinned by the golden file)
            assert total == wrapper, key  # the *_bytes wrapper is the same walk
        end = 0
        for name, off, need in members:
            if off is None:  # an absent section takes no room and nobody indexes it
                continue
            assert need >= 0, (key, name)  # every member states what its launcher indexes
            assert off % 256 == 0 or key.startswith("staged("), (key, name)
            assert off >= end, (key, name)  # declaration order, past the previous member's use
            end = off + need
        assert end <= total, key
        if key.startswith(("link_staging(", "checksum_batch(")):
            absent = [name for name, off, _ in members if off is None]
            pre = key.endswith(",1)")
            if key.startswith("link_staging(") and not pre:
                # zero-element sections: the three pointers coincide with the counters
                offs = {name: off for name, off, _ in members}
                assert offs["boff"] == offs["tiles"] == offs["filter"] == offs["counters"], key
            if key.startswith("checksum_batch("):
                n = int(key[len("checksum_batch("):].split(",")[0])
                assert absent == ([] if n >= 65536 else ["lane_info", "lkeys", "skeys", "order"]), key


def test_wrapper_of_the_hash_grouping_is_the_largest_chain(layout_lines):
    sizes, _ = layout_lines
    flags = {k: v for k, v in sizes.items() if k.startswith(("hash_group_is_max(", "staged_h2d("))}
    assert len(flags) == 13 * 3 + 20 and all(v == 1 for v in flags.values()), flags


def test_totals_equal_the_parents(layout_lines, golden):
    """The library hands out the same bytes as the last commit with hand-written layouts: every
    exported total, and every total that commit computed in static code (by its formulas)."""
    sizes, layouts = layout_lines
    assert len(golden["parent_commit"]) == 40
    assert (len(golden["exported"]), len(golden["by_formula"])) == (201, 281)
    for key, want in golden["exported"].items():
        if key.startswith("region_group_workspace_bytes("):
            want += REGION_OBJECTS_RESERVE
        assert sizes[key] == want, key
    for key, want in golden["by_formula"].items():
        assert layouts[key][0] == want, key
