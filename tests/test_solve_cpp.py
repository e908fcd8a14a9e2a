"""tests/cpp/test_solve.cpp: spsamd_solve_tri through the plain C ABI on the device against the substitution loop compiled by
g++ (real subsd / divsd NaN rules), with a Gauss-Seidel sweep chained from spsamd_multiply_dense; built with the same g++
line as the shim test in test_abi.py."""
import os
import subprocess

import pytest

from tests.gpu_util import build_cpp_test


def test_cpp_solve_compiles(tmp_path):
    assert os.path.exists(build_cpp_test("solve", tmp_path))


@pytest.mark.gpu
def test_cpp_solve(tmp_path):
    out = subprocess.run([build_cpp_test("solve", tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
