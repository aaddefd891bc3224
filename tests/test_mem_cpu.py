"""The owning buffers of csrc/gicp_mem.h (DevBuf, PinnedBuf, alloc_init), checked on the CPU.

tests/native/mem_check.cpp includes the header as the library does and defines the four functions it reaches
the runtime through on malloc / free, with counters and an injected allocation failure.  It is built here with
the address and undefined-behaviour sanitizers (LeakSanitizer included) and run as a child process: growth
policy, failure injection, moves and swaps, allocate-initialise-publish, and no leak at exit.  No GPU and
nothing loaded into Python."""
import os
import subprocess

from native_build import ROOT, build

SRC = os.path.join(ROOT, "tests", "native", "mem_check.cpp")
CASES = ("growth_policy_device", "growth_policy_pinned", "failure_injection", "moves_and_swaps", "publish_after_init")


def test_owning_buffers_under_sanitizers(tmp_path):
    exe = build([SRC], str(tmp_path / "mem_check"), "address,undefined", ["-fno-sanitize-recover=all"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    for case in CASES:
        assert f"ok {case}" in lines, (case, run.stdout)
    assert "FAIL" not in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    assert lines[-1] == "PASS"
    counts = next(ln for ln in lines if ln.startswith("allocations")).split()
    assert counts[1] == counts[3] and int(counts[1]) > 0 and counts[6] == "0" and counts[9] == "0", counts
