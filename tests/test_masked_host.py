"""spsamd_multiply_masked without a GPU: the reference helper (tests/masked_ref.py, the row-wise checker filtered by M's
keys) is pinned to the oracle's inner-product loop filtered the same way, and the library and the Python binding carry
the new entry point."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import binding as orc
from tests import add_ref as ar
from tests import masked_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = (1.0, -0.75, np.inf)


def _case(seed):
    rng = np.random.default_rng(seed)
    nrow, ninner, ncol = (int(x) for x in rng.integers(1, 8, 3))
    tA, tB = str(rng.choice(['.', 'T'])), str(rng.choice(['.', 'T']))
    ash = (ninner, nrow) if tA == 'T' else (nrow, ninner)
    bsh = (ncol, ninner) if tB == 'T' else (ninner, ncol)
    junk = bool(rng.integers(2))
    A = ar.random_operand(rng, ash, int(rng.integers(0, 40)), lead_junk=junk)
    B = ar.random_operand(rng, bsh, int(rng.integers(0, 40)), lead_junk=junk)
    sc = [mr.random_scale(rng, d, rng.random() < 0.4) for d in (nrow, ninner, ncol)]
    sc = [None if s is None else orc.Vec(s[0], s[1], d) for s, d in zip(sc, (nrow, ninner, ncol))]
    M = mr.random_mask(rng, (nrow, ncol), int(rng.integers(0, 30)))
    kw = dict(C_=CS[seed % 3], scalei=sc[0], tA=tA, scalej=sc[1], tB=tB, scalek=sc[2],
              duplicate_policy=int(rng.integers(0, 3)), zero_nan=junk or bool(rng.integers(2)))
    return orc.Mat(*A, ash), orc.Mat(*B, bsh), M, kw


@pytest.mark.parametrize("block", range(4))
def test_helper_matches_inner_product_oracle(block):
    """masked_ref (row-wise checker + filter) == orc_multiply_mm + the same filter over 400 seeded cases with NaN
    payloads, +-Inf, +-0, duplicates, scales with missing and zero entries, every policy and zero_nan: indices equal,
    values bit for bit, NaNs as NaNs (mr.same_tuples)."""
    for seed in range(block * 100, block * 100 + 100):
        A, B, M, kw = _case(seed)
        got = mr.masked_ref(A, B, M, **kw)
        want = mr.masked_ref(A, B, M, rowwise=False, **kw)
        assert mr.same_tuples(got, want), "seed %d" % seed


def test_helper_known_answers():
    # (L L) o L on a triangle plus a pendant edge: one triangle, found at its (max, min) key
    L = orc.Mat([1, 2, 2, 3], [0, 0, 1, 2], np.ones(4), (4, 4))
    i, j, v = mr.masked_ref(L, L, ([1, 2, 2, 3, 2], [0, 0, 1, 2, 0]))
    assert list(zip(i.tolist(), j.tolist(), v.tolist())) == [(2, 0, 1.0)]
    # a pre-scale sum that the scale turns into 0.0 is still emitted; a key outside the product's pattern is not
    A = orc.Mat([0, 1], [0, 0], [2.0, 3.0], (2, 1))
    B = orc.Mat([0], [0], [1.0], (1, 1))
    i, j, v = mr.masked_ref(A, B, ([0, 1], [0, 0]), scalei=orc.Vec([0, 1], [0.5, 0.0], 2))
    assert i.tolist() == [0] and v.tolist() == [1.0]
    i, j, v = mr.masked_ref(A, B, ([0, 1], [0, 0]), C_=0.0)
    assert i.size == 0
    # sanitize_duplicates keeps specials only on keys that occur once
    X = mr.sanitize_duplicates((np.array([0, 0, 1]), np.array([1, 1, 0]), np.array([np.nan, 1.0, np.inf])))
    assert np.isfinite(X[2][:2]).all() and np.isinf(X[2][2])


def test_entry_point_is_exported_and_bound():
    """Fails without the feature: the header declares spsamd_multiply_masked, the built library exports it, capi binds it
    and knows the masked_path knob's entry point."""
    from spsparse_amd import build, capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spsparse_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+spsamd_multiply_masked\s*\(", text)
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_multiply_masked")
    assert "spsamd_multiply_masked" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "multiply_masked", None))
    assert "masked_path" in open(os.path.join(ROOT, "include", "spsparse_amd.h")).read()
