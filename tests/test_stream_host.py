"""spsamd_multiply_stream without a GPU: the numpy model of its row-block partition on hand-made cases, the C++ template
with stream_block_tuples set compiles and links, and the streamed path fails loudly where there is no device."""
import os
import subprocess

import numpy as np
import pytest

from tests import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _op(idx0, idx1, t):
    """(rows, inner) of op(X) for stored indices."""
    return (idx1, idx0) if t == "T" else (idx0, idx1)


def test_bounds_count_products_and_cap_at_columns():
    # op(A) 4 x 3: row 0 -> k 0, 2; row 1 empty; row 2 -> k 1; row 3 -> k 0, 1, 2
    ar, ak = np.array([0, 0, 2, 3, 3, 3]), np.array([0, 2, 1, 0, 1, 2])
    blen = np.array([2, 5, 1])                        # op(B) rows of 2, 5 and 1 tuples
    assert list(sr.row_bounds(ar, ak, 4, blen, 100)) == [3, 0, 5, 8]
    assert list(sr.row_bounds(ar, ak, 4, blen, 4)) == [3, 0, 4, 4]     # min(P_r, cols(op(B)))


def test_empty_rows_join_the_block_before_them():
    bound = [3, 0, 0, 4, 0, 2, 0]
    assert sr.blocks(bound, 7) == [0, 5, 7]          # 3+0+0+4+0 = 7, then 2+0
    assert sr.blocks([0, 0, 0], 1) == [0, 3]         # one block of empty rows
    assert sr.blocks(bound, 100) == [0, 7]


def test_a_row_exactly_at_the_budget():
    assert sr.blocks([5, 1, 5, 5], 5) == [0, 1, 2, 3, 4]
    assert sr.blocks([4, 1, 5, 0, 1], 5) == [0, 2, 4, 5]


def test_a_row_over_the_budget_names_the_smallest_budget():
    with pytest.raises(sr.Capacity) as e:
        sr.blocks([1, 9, 2], 8)
    assert e.value.smallest == 9
    assert sr.blocks([1, 9, 2], 9) == [0, 1, 2, 3]  # 1 + 9 > 9 and 9 + 2 > 9: one row per block
    assert sr.blocks([1, 9, 2], 10) == [0, 2, 3]


def test_transposes_take_rows_of_op():
    # stored A 3 x 2 with 'T': op(A) is 2 x 3, its rows are the stored columns
    a0, a1 = np.array([0, 1, 2, 2]), np.array([0, 0, 1, 0])
    rows, inner = _op(a0, a1, "T")
    # stored B 4 x 3 with 'T': op(B) is 3 x 4, its rows are the stored columns (k = idx1)
    b0, b1 = np.array([0, 1, 2, 3, 3]), np.array([0, 0, 2, 1, 2])
    brows, _ = _op(b0, b1, "T")
    blen = np.bincount(brows, minlength=3)           # [2, 1, 2]
    bound = sr.row_bounds(rows, inner, 2, blen, 4)
    assert list(bound) == [4, 2]                     # op(A) row 0 -> k 0, 1, 2 (2+1+2 = 5, capped at 4); row 1 -> k 2
    assert sr.block_count(rows, inner, 2, blen, 4, 4) == 2
    assert sr.block_count(rows, inner, 2, blen, 4, 6) == 1
    assert sr.block_count([], [], 2, blen, 4, 6) == 0


def _build(tmp_path):
    from spsparse_amd import build
    libdir = os.path.dirname(build.build())
    exe = os.path.join(str(tmp_path), "test_stream")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_stream.cpp"), "-o", exe, "-L" + libdir, "-lspsparse_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_template_with_stream_block_tuples_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _gpu_present():
    try:
        out = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        return "gfx950" in out
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="CPU-container check")
def test_streamed_path_fails_loudly_without_gpu(tmp_path):
    out = subprocess.run([_build(tmp_path), "--abi-only"], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "fails loudly" in out.stdout


@pytest.mark.gpu
def test_cpp_streamed_multiply_equals_plain(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
