"""Building the stand-alone programs under tests/native (test_mem_cpu.py, test_host_cpu.py): host code only, with a
sanitizer linked in statically, run as child processes.  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")


def host_compiler():
    """The host compiler of the ROCm tree the library is built with (the Makefile's ROCM), or g++."""
    clang = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    cxx = clang if os.access(clang, os.X_OK) else shutil.which("g++")
    assert cxx, "no host C++ compiler: neither the ROCm tree's clang++ nor g++"
    return cxx


def build(sources, exe, sanitize, flags=()):
    """Compile `sources` into `exe` under -fsanitize=`sanitize`; the build must succeed without a warning."""
    cxx = host_compiler()
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", "-g", f"-fsanitize={sanitize}", *flags, *sources, "-o", exe]
    if os.path.basename(cxx) == "g++":   # clang links the sanitizer runtimes statically by default; g++ on request
        static = {"address": "-static-libasan", "undefined": "-static-libubsan", "thread": "-static-libtsan"}
        cmd[1:1] = [static[s] for s in sanitize.split(",")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe
