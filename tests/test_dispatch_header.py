"""csrc/nb_dispatch.h, the value -> template-argument helper every host launcher goes through, tested on its own: a host-only
C++ program (tests/dispatch/dispatch_test.cpp) built with the host compiler, address and undefined-behaviour sanitizers on.
No GPU and no HIP runtime library: the header only needs hipError_t."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

ROCM_INCLUDE = "/opt/rocm/include"


def test_dispatch_header_host_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dispatch_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
           "-I" + os.path.join(ROOT, "nbody_cosmological_simulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "dispatch", "dispatch_test.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    # the program allocates nothing; the leak checker needs ptrace, which a sandboxed runner may not grant
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
