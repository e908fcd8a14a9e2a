"""tests/cpp/test_extract.cpp: spsparse_amd::extract (the C++ mirror of spsamd_extract) on the device,
built with the same g++ line as the shim test in test_abi.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from spsparse_amd import build
    libdir = os.path.dirname(build.build())
    exe = os.path.join(str(tmp_path), "test_extract")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_extract.cpp"), "-o", exe, "-L" + libdir, "-lspsparse_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_extract_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_extract(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
