"""Host restatement of spsamd_emult (include/spsparse_amd.h): the yardstick of the device kernels.

S_A is op(A) as the call takes it (tests/select_ref.operand_S: a raw operand consolidated by op()'s rows, an operand whose
sort0 names op()'s row order as stored).  Under TIMES S_B is op(B) taken the same way; under FIRST B is structural: only the
keys of op(B) count, whatever its values, duplicates and order are.  The result is the subsequence of S_A whose key is a key of
B (complement: is not), decided tuple by tuple through a dictionary from a key to the FIRST position of S_B that holds it:

    TIMES   v = (alpha * a) * b     two float64 multiplies, left to right, through dense_ref.mul: numpy's multiply with the
                                    x86-64 NaN rule written out (the left operand's NaN, quieted, else the right one's, else
                                    the default NaN).  numpy alone gives those bits whenever at most one operand is a NaN;
                                    for two NaNs its vector loops may return either (tests/test_emult_host.py checks both)
    FIRST   v = a                   bits untouched

emult_ref        vectorised: sorted unique keys of B, one searchsorted
emult_ref_loop   the dictionary, tuple by tuple: what test_emult_host.py pins emult_ref to
"""
import numpy as np

from tests import add_ref as ar
from tests import dense_ref as dr
from tests import select_ref as sr

TIMES, FIRST = 1, 2


def keys(rows, cols):
    return (np.asarray(rows, np.int64) << 32) | np.asarray(cols, np.int64)


def operands(A, B, op, tA='.', tB='.', policy=ar.ADD, zero_nan=False, sortA=-1, sortB=-1):
    """(S_A, S_B) for the stored tuples A, B = (idx0, idx1, val); under FIRST S_B is op(B)'s tuples as stored (only their
    keys are looked at, val may be None)."""
    SA = sr.operand_S(A, tA, policy, zero_nan, sortA)
    if op == TIMES:
        return SA, sr.operand_S(B, tB, policy, zero_nan, sortB)
    r, c = ar.op(B[0], B[1], tB)
    return SA, (np.asarray(r, np.int32), np.asarray(c, np.int32), None)


def times(alpha, a, b):
    return dr.mul(dr.mul(np.float64(alpha), np.asarray(a, np.float64)), np.asarray(b, np.float64))


def emult_ref(SA, SB, op, alpha=1.0, complement=False):
    """(rows, cols, vals) of the result; SA, SB as operands() returns them."""
    ra, ca, va = (np.asarray(x) for x in SA)
    ka, kb = keys(ra, ca), keys(SB[0], SB[1])
    ub, first = np.unique(kb, return_index=True)                # first: the first position of each key in S_B
    pos = np.searchsorted(ub, ka)
    hit = np.zeros(len(ka), bool)
    inb = pos < len(ub)
    hit[inb] = ub[pos[inb]] == ka[inb]
    keep = ~hit if complement else hit
    v = va[keep]
    if op == TIMES:
        v = times(alpha, v, np.asarray(SB[2], np.float64)[first[pos[keep]]])
    return ra[keep].astype(np.int32), ca[keep].astype(np.int32), np.asarray(v, np.float64)


def emult_ref_loop(SA, SB, op, alpha=1.0, complement=False):
    """The same, one tuple of S_A after the other."""
    where = {}
    for q, k in enumerate(zip(np.asarray(SB[0]).tolist(), np.asarray(SB[1]).tolist())):
        where.setdefault(k, q)
    oi, oj, ov = [], [], []
    for i, j, a in zip(np.asarray(SA[0]).tolist(), np.asarray(SA[1]).tolist(), np.asarray(SA[2], np.float64)):
        q = where.get((i, j))
        if (q is None) != bool(complement):
            continue
        if op == TIMES:
            a = times(alpha, np.array([a]), np.array([SB[2][q]]))[0]
        oi.append(i); oj.append(j); ov.append(a)
    return np.array(oi, np.int32), np.array(oj, np.int32), np.array(ov, np.float64)
