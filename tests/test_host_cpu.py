"""The host-only unit of the library (csrc/gicp_hostmath.cpp: the tiling and its thread pool, the shard split, the
accept threshold, the host scans), checked on the CPU.

tests/native/host_check.cpp is linked with gicp_hostmath.cpp by the host compiler alone (no HIP runtime), once
under the address and undefined-behaviour sanitizers and once under the thread sanitizer, and run as a child
process.  The tile table decides every result of the library; here it must be a partition within its caps, and
the same table whatever the warm-start hint and the number of pool threads.  No GPU and nothing loaded into
Python."""
import os
import subprocess

import pytest

from native_build import ROCM, ROOT, build

CSRC = os.path.join(ROOT, "generalized-icp_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "host_check.cpp"), os.path.join(CSRC, "gicp_hostmath.cpp")]
# gicp_internal.h takes its vector types from the HIP headers; as host code they need no HIP compiler
FLAGS = ["-O1", "-pthread", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include")]
CASES = ("tiling_partition", "tiling_independent_of_hint_and_threads", "worker_pool", "shard_tile_count",
         "accept_d2_max", "scan_bounds")


@pytest.mark.parametrize("sanitize,extra", [("address,undefined", ["-fno-sanitize-recover=all"]), ("thread", [])],
                         ids=["asan_ubsan", "tsan"])
def test_host_unit_under_sanitizers(tmp_path, sanitize, extra):
    exe = build(SOURCES, str(tmp_path / "host_check"), sanitize, extra + FLAGS)
    env = {k: v for k, v in os.environ.items() if k != "GICP_TILE_BUDGET"}   # the default tile budget
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    for case in CASES:
        assert f"ok {case}" in lines, (case, run.stdout)
    assert "FAIL" not in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    assert lines[-1] == "PASS"
