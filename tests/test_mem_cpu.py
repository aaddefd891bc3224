"""The owning buffers of csrc/gicp_mem.h (DevBuf, PinnedBuf, alloc_init), checked on the CPU.

tests/native/mem_check.cpp includes the header as the library does and defines the four functions it reaches
the runtime through on malloc / free, with counters and an injected allocation failure.  It is built here with
the address and undefined-behaviour sanitizers (LeakSanitizer included) and run as a child process: growth
policy, failure injection, moves and swaps, allocate-initialise-publish, and no leak at exit.  No GPU and
nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mem_check.cpp")
CASES = ("growth_policy_device", "growth_policy_pinned", "failure_injection", "moves_and_swaps", "publish_after_init")


def host_compiler():
    """The host compiler of the ROCm tree the library is built with (the Makefile's ROCM), or g++."""
    clang = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = clang if os.access(clang, os.X_OK) else shutil.which("g++")
    assert cxx, "no host C++ compiler: neither the ROCm tree's clang++ nor g++"
    return cxx


def test_owning_buffers_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mem_check")
    cxx = host_compiler()
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           SRC, "-o", exe]
    if os.path.basename(cxx) == "g++":   # clang links the sanitizer runtimes statically by default; g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
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
