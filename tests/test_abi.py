"""The drop-in boundary without a GPU: the C ABI library loads, exports every
symbol include/spsparse_amd.h declares, the C++ shim (same parameter list as
spsparse::multiply, multiply_sparse.hpp:138-164) compiles and links, and
every way into the product path fails loudly when no device is present
(there is no CPU fallback).  The GPU half runs the C++ restatement of the
reference's own tests through the shim."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.gpu_util import build_cpp_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spsparse_amd.h")


def _lib():
    from spsparse_amd import build
    return build.build()


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(spsamd_[a-z0-9_]+)\s*\(", text))
    return sorted(n for n in names if n != "spsamd_chunk_fn")


def test_library_exports_every_declared_symbol():
    from spsparse_amd import capi
    lib = ctypes.CDLL(_lib())
    declared = _declared()
    assert len(declared) >= 13
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(capi.SYMBOLS) == declared
    assert b"gfx950" in ctypes.cast(ctypes.CFUNCTYPE(ctypes.c_char_p)(("spsamd_version", lib))(), ctypes.c_char_p).value


def test_product_path_has_no_oracle_or_cpu_fallback():
    """Nothing under spsparse_amd/ or include/ may touch oracle/."""
    for top in ("spsparse_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".h", ".hpp", ".hip", ".cpp")):
                    src = open(os.path.join(dp, f), errors="ignore").read()
                    assert "oracle" not in src.replace("test oracle", "").replace("the oracle's", ""), os.path.join(dp, f)
    # ... and the developer scripts may not import it either (checkers that need it live under tests/)
    for f in os.listdir(os.path.join(ROOT, "scripts")):
        if f.endswith((".py", ".sh")):
            src = open(os.path.join(ROOT, "scripts", f), errors="ignore").read()
            assert "import orc" not in src and "from oracle" not in src and "oracle/" not in src, f


def _gpu_present():
    try:
        out = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        return "gfx950" in out
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="CPU-container check")
def test_fails_loudly_without_gpu(tmp_path):
    from spsparse_amd import capi
    with pytest.raises(capi.SpsamdError) as e:
        capi.Context()
    assert e.value.code == -6
    exe = build_cpp_test("shim", tmp_path)
    out = subprocess.run([exe, "--abi-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "fails loudly" in out.stdout


@pytest.mark.gpu
def test_cpp_shim_restates_reference_tests(tmp_path):
    """tests/test_multiply_sparse.cpp:45-78,84-136; tests/test_array.cpp:50-56,135-168 through
    spsparse_amd::multiply / VectorCooArray on the device."""
    exe = build_cpp_test("shim", tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
