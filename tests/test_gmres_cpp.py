"""tests/cpp/test_gmres.cpp: spsamd_solve_gmres through the plain C ABI on the device against the loop of the header
compiled by g++ with -ffp-contract=off, on an upwind 1-D convection-diffusion operator of order 2500 (two levels of the fold)
under the three preconditioners with restart 7, and on a 6 x 6 operand with a NaN.  The g++ line of the other C++ tests plus the contraction
flag."""
import os
import subprocess

import pytest

from tests.gpu_util import ROOT


def _build(tmp_path):
    from spsparse_amd import build
    libdir = os.path.dirname(build.build())
    exe = os.path.join(str(tmp_path), "test_gmres")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_gmres.cpp"), "-o", exe, "-L" + libdir,
                           "-lspsparse_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_gmres_compiles(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe, "--abi-only"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")


@pytest.mark.gpu
def test_cpp_gmres(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
