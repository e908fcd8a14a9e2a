"""tests/cpp/test_emult.cpp: spsamd_emult through the plain C ABI on the device, built with the same g++ line as the shim
test in test_abi.py."""
import os
import subprocess

import pytest

from tests.gpu_util import build_cpp_test


def test_cpp_emult_compiles(tmp_path):
    assert os.path.exists(build_cpp_test("emult", tmp_path))


@pytest.mark.gpu
def test_cpp_emult(tmp_path):
    out = subprocess.run([build_cpp_test("emult", tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
