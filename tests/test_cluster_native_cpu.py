"""The host yardstick of Euclidean cluster extraction (csrc/gicp_hostmath.cpp gicp_cluster_points_host)
under the address and undefined-behaviour sanitizers.

tests/native/cluster_check.cpp is linked with gicp_hostmath.cpp by the host compiler alone (no HIP runtime) and run as a
child process: a few of the CPU cases, each against a union-find over all pairs written out with the shared predicate
and decision, with exactly-sized output buffers.  No GPU and nothing sanitized loaded into Python."""
import os
import subprocess

from native_build import ROCM, ROOT, build

CSRC = os.path.join(ROOT, "generalized-icp_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "cluster_check.cpp"), os.path.join(CSRC, "gicp_hostmath.cpp")]
# gicp_internal.h takes its vector types from the HIP headers; as host code they need no HIP compiler
FLAGS = ["-O1", "-pthread", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include")]
CASES = ("random", "random_min2", "random_2_to_5", "one_row", "two_rows", "chain", "chain_below", "lattice", "coincident",
         "refused")


def test_host_cluster_under_sanitizers(tmp_path):
    exe = build(SOURCES, str(tmp_path / "cluster_check"), "address,undefined", FLAGS)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    for case in CASES:
        for dim in (2, 3):
            assert any(line.startswith(f"ok {case}_{dim}d") for line in lines), (case, dim, run.stdout)
    assert "FAIL" not in run.stdout and run.stderr == "", (run.stdout, run.stderr)
    assert lines[-1] == "PASS"
