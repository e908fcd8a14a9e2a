"""tests/cpp/test_aggregate.cpp: spsamd_aggregate through the plain C ABI on the device against the loop of the header compiled
by g++, on three dozen random patterns.  The g++ line of the other C++ tests plus the HIP runtime, whose hipMalloc gives the
device buffers."""
import os
import subprocess

import pytest

from tests.gpu_util import ROOT


def _build(tmp_path):
    from spsparse_amd import build
    libdir = os.path.dirname(build.build())
    exe = os.path.join(str(tmp_path), "test_aggregate")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_aggregate.cpp"), "-o", exe, "-L" + libdir,
                           "-lspsparse_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_aggregate_compiles(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe, "--abi-only"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")


@pytest.mark.gpu
def test_cpp_aggregate(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
