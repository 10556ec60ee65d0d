"""Host-side checks of the round-6 measurement tools (no GPU): the rehearsal checker pulls the
bench line out of a committed one-GPU N-rank rehearsal log (gloo chatter around it) and
passes it, and fails a line whose exchange overflowed; and of tools/kernel_isa_diff.py, the
per-kernel comparison of two builds' device assembly, on made-up text."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "rehearsal_check.py")


def run(log, n):
    return subprocess.run([sys.executable, TOOL, log, str(n)], capture_output=True, text=True)


def test_rehearsal_check_on_committed_logs(tmp_path):
    for n in (2, 4, 8):
        src = os.path.join(ROOT, "profiles", "r06", "final", f"bench_n{n}_rehearsal.log")
        log = tmp_path / f"n{n}.log"
        log.write_text(open(src, errors="replace").read())
        r = run(str(log), n)
        assert r.returncode == 0, r.stdout + r.stderr
        d = json.loads(r.stdout)
        assert d["ok"] and d["n_gpus"] == n and d["capacity_per_peer"] > 0
        assert json.load(open(tmp_path / f"n{n}.json"))["n_gpus"] == n


def test_rehearsal_check_rejects_overflow_and_wrong_n(tmp_path):
    src = os.path.join(ROOT, "profiles", "r06", "final", "bench_n2_rehearsal.json")
    line = json.load(open(src))
    assert run_line(tmp_path, line, 4).returncode == 1  # n_gpus mismatch
    bad = json.loads(json.dumps(line).replace('"timed_steps_overflowed": 0', '"timed_steps_overflowed": 3'))
    r = run_line(tmp_path, bad, 2)
    assert r.returncode == 1 and not json.loads(r.stdout)["checks"]["timed_steps_overflowed_0"]


def run_line(tmp_path, line, n):
    log = tmp_path / "x.log"
    log.write_text("[Gloo] Rank 0 is connected to 1 peer ranks.\n" + json.dumps(line) + "\n")
    return run(str(log), n)


def _isa_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ASM = """\t.text
\t.type\tkern_a,@function
kern_a:                                 ; @kern_a
; %bb.0:
\top_one v0, v1                          ; a comment
\tbranch_if .LBB{k}_2
.LBB{k}_2:                                ; =>This Inner Loop Header
\top_two v0, {imm}
.Lfunc_end{k}:
\t.size\tkern_a, .Lfunc_end{k}-kern_a
; Kernel info:
; codeLenInByte = 12
; NumVgprs: {vgprs}
; ScratchSize: 0
; LDSByteSize: 512 bytes/workgroup (compile time only)
; Occupancy: 8
\t.type\tkern_b,@function
kern_b:
\top_three
.Lfunc_end{k1}:
; NumVgprs: 3
"""


def test_kernel_isa_diff_splits_and_normalises():
    """tools/kernel_isa_diff.py on made-up text: functions are split at their symbols, comments and
    block-label numbers do not count, an operand and a resource figure do."""
    tool = _isa_tool()
    assert tool.normalise("\tbranch .LBB12_34 ; why") == "\tbranch .LBB_34"
    assert tool.normalise("; only a comment") == "" and tool.normalise("   ") == ""
    a = tool.split_functions(ASM.format(k=0, k1=1, imm=7, vgprs=24))
    b = tool.split_functions(ASM.format(k=9, k1=10, imm=7, vgprs=24))
    assert list(a) == ["kern_a", "kern_b"]
    assert a["kern_a"][0] == ["\top_one v0, v1", "\tbranch_if .LBB_2", ".LBB_2:", "\top_two v0, 7"]
    assert a["kern_a"][1] == {"codeLenInByte": 12, "NumVgprs": 24, "ScratchSize": 0, "LDSByteSize": 512,
                              "Occupancy": 8}
    assert a["kern_b"] == (["\top_three"], {"NumVgprs": 3})
    assert a == b  # another function index: the same kernels
    assert tool.first_difference(a["kern_a"][0], b["kern_a"][0]) is None
    c = tool.split_functions(ASM.format(k=0, k1=1, imm=8, vgprs=25))
    assert tool.first_difference(a["kern_a"][0], c["kern_a"][0]) == (3, ["\top_two v0, 7"], ["\top_two v0, 8"])
    assert a["kern_a"][1] != c["kern_a"][1] and a["kern_b"] == c["kern_b"]
    assert tool.first_difference(["x"], ["x", "y"]) == (1, [], ["y"])


def test_kernel_isa_diff_exit_status(tmp_path):
    same, other = tmp_path / "a.s", tmp_path / "b.s"
    same.write_text(ASM.format(k=0, k1=1, imm=7, vgprs=24))
    other.write_text(ASM.format(k=4, k1=5, imm=8, vgprs=24))
    tool = os.path.join(ROOT, "tools", "kernel_isa_diff.py")
    r = subprocess.run([sys.executable, tool, "--a", str(same), "--b", str(same)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("SAME") == 2, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool, "--a", str(same), "--b", str(other)], capture_output=True, text=True)
    assert r.returncode == 1 and "DIFFERS  kern_a" in r.stdout and "SAME     kern_b" in r.stdout, r.stdout
