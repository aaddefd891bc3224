"""The host yardstick of statistical outlier removal (csrc/gicp_hostmath.cpp gicp_sor_points_host) under
the address and undefined-behaviour sanitizers.

tests/native/sor_check.cpp is linked with gicp_hostmath.cpp by the host compiler alone (no HIP runtime) and run as a
child process: a few of the CPU cases, each against a full sort of every row's distances and the definition written out
with the shared functions, with exactly-sized output buffers.  No GPU and nothing sanitized loaded into Python."""
import os
import subprocess

from native_build import ROCM, ROOT, build

CSRC = os.path.join(ROOT, "generalized-icp_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "sor_check.cpp"), os.path.join(CSRC, "gicp_hostmath.cpp")]
# gicp_internal.h takes its vector types from the HIP headers; as host code they need no HIP compiler
FLAGS = ["-O1", "-pthread", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include")]
CASES = ("random_k8", "random_k1", "random_k31_ratio0", "two_rows_k8", "five_rows_k31", "nine_rows_k8", "lattice_k6",
         "coincident_k31", "refused")


def test_host_sor_under_sanitizers(tmp_path):
    exe = build(SOURCES, str(tmp_path / "sor_check"), "address,undefined", FLAGS)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    for case in CASES:
        for dim in (2, 3):
            assert any(line.startswith(f"ok {case}_{dim}d") for line in lines), (case, dim, run.stdout)
    assert "FAIL" not in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    assert lines[-1] == "PASS"
