"""spsamd_add without a GPU: the host restatement (tests/add_ref.py) is pinned to the test oracle's consolidate() of the
concatenated, pre-scaled tuples, and the library, header and Python binding carry the new entry point."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import binding as orc
from tests import add_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1.0, -0.75, 0.0, np.inf)


def _case(seed):
    rng = np.random.default_rng(seed)
    shape = (int(rng.integers(1, 7)), int(rng.integers(1, 7)))
    tA, tB = rng.choice(['.', 'T']), rng.choice(['.', 'T'])
    bshape = shape[::-1] if (tA == 'T') != (tB == 'T') else shape
    junk = bool(rng.integers(2))
    A = ar.random_operand(rng, shape, int(rng.integers(0, 40)), lead_junk=junk)
    B = ar.random_operand(rng, bshape, int(rng.integers(0, 40)), lead_junk=junk)
    alpha, beta = SCALES[int(rng.integers(4))] if rng.random() < 0.5 else 1.0, SCALES[int(rng.integers(4))]
    return A, B, float(alpha), float(beta), str(tA), str(tB), int(rng.integers(0, 3)), junk or bool(rng.integers(2))


@pytest.mark.parametrize("block", range(6))
def test_restatement_matches_oracle_consolidate(block):
    """add_ref == orc.consolidate(scaled_cat(...)) bit for bit, over 300 seeded cases."""
    for seed in range(block * 50, block * 50 + 50):
        A, B, alpha, beta, tA, tB, pol, zn = _case(seed)
        got = ar.add_ref(A, B, alpha, beta, tA, tB, pol, zn)
        r, c, v = ar.scaled_cat(A, B, alpha, beta, tA, tB)
        want = orc.consolidate(r, c, v, 0, pol, zn)
        assert ar.same_tuples(got, want), "seed %d" % seed


def test_cases_cover_the_quirks():
    """The seeded cases hold what they are meant to: duplicates across operands, +-0, NaN payloads, +-Inf, a leading run
    of NaNs spread over both operands under zero_nan, and cancellations to 0.0 that are emitted."""
    seen = dict(cross_dup=0, neg_zero=0, nan_payloads=set(), inf=0, lead_both=0)
    for seed in range(300):
        A, B, alpha, beta, tA, tB, pol, zn = _case(seed)
        ra, ca = ar.op(A[0], A[1], tA)
        rb, cb = ar.op(B[0], B[1], tB)
        ka, kb = set(zip(ra.tolist(), ca.tolist())), set(zip(rb.tolist(), cb.tolist()))
        seen["cross_dup"] += bool(ka & kb)
        for v in (A[2], B[2]):
            seen["neg_zero"] += int(np.sum((v == 0) & np.signbit(v)))
            seen["inf"] += int(np.sum(np.isinf(v)))
            seen["nan_payloads"] |= set(v[np.isnan(v)].view(np.uint64).tolist())
        if zn and len(A[2]) and len(B[2]):
            a_low = np.isnan(A[2][np.lexsort((ca, ra))][:1]).any()
            b_low = np.isnan(B[2][np.lexsort((cb, rb))][:1]).any()
            seen["lead_both"] += bool(a_low and b_low)
    assert seen["cross_dup"] > 200 and seen["neg_zero"] > 50 and seen["inf"] > 50 and seen["lead_both"] > 10
    assert len(seen["nan_payloads"]) >= 4


def test_quirks_known_answers():
    nan = np.nan
    # a sum that cancels to 0.0 is emitted; a zero after the first kept entry is dropped
    A = (np.array([0, 0]), np.array([0, 1]), np.array([1.0, 0.0]))
    B = (np.array([0]), np.array([0]), np.array([-1.0]))
    i, j, v = ar.add_ref(A, B)
    assert i.tolist() == [0] and j.tolist() == [0] and v[0] == 0.0
    # zero_nan: the leading NaNs of BOTH operands go, a NaN after the first kept entry stays
    A = (np.array([0, 1]), np.array([0, 1]), np.array([nan, nan]))
    B = (np.array([0, 0]), np.array([0, 1]), np.array([nan, 2.0]))
    i, j, v = ar.add_ref(A, B, zero_nan=True)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (1, 1)] and v[0] == 2.0 and np.isnan(v[1])
    # A's tuples of a key come before B's: REPLACE keeps B's, LEAVE_ALONE A's
    A = (np.array([0]), np.array([0]), np.array([1.0]))
    B = (np.array([0]), np.array([0]), np.array([5.0]))
    assert ar.add_ref(A, B, policy=ar.REPLACE)[2].tolist() == [5.0]
    assert ar.add_ref(A, B, policy=ar.LEAVE_ALONE)[2].tolist() == [1.0]
    # alpha = 0 still multiplies: 0 * Inf is the x86 default NaN
    A = (np.array([0]), np.array([0]), np.array([np.inf]))
    v = ar.add_ref(A, (np.array([], np.int32),) * 2 + (np.array([]),), alpha=0.0)[2]
    assert v.view(np.uint64)[0] == np.uint64(0xFFF8000000000000)


def test_entry_point_is_declared_exported_and_bound():
    """Fails without the feature: the header declares spsamd_add, the built library exports it, capi binds it."""
    from spsparse_amd import build, capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spsparse_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+spsamd_add\s*\(", text)
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_add")
    assert "spsamd_add" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "add", None))
