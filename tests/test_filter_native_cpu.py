"""The host yardstick of the input filters (csrc/gicp_hostmath.cpp gicp_filter_points_host) under the
address and undefined-behaviour sanitizers.

tests/native/filter_check.cpp is linked with gicp_hostmath.cpp by the host compiler alone (no HIP runtime) and run as
a child process: a few of the CPU cases, each against a brute-force count over all pairs, with exactly-sized output
buffers.  No GPU and nothing sanitized loaded into Python."""
import os
import subprocess

from native_build import ROCM, ROOT, build

CSRC = os.path.join(ROOT, "generalized-icp_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "filter_check.cpp"), os.path.join(CSRC, "gicp_hostmath.cpp")]
# gicp_internal.h takes its vector types from the HIP headers; as host code they need no HIP compiler
FLAGS = ["-O1", "-pthread", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include")]
CASES = ("shell_and_radius", "lattice_on_the_bound", "lattice_crop", "two_coincident", "one_row", "widest_grid",
         "refused_grid")


def test_host_filter_under_sanitizers(tmp_path):
    exe = build(SOURCES, str(tmp_path / "filter_check"), "address,undefined", FLAGS)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    for case in CASES:
        for dim in (2, 3):
            assert any(line.startswith(f"ok {case}_{dim}d") for line in lines), (case, dim, run.stdout)
    assert "FAIL" not in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    assert lines[-1] == "PASS"
