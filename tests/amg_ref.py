"""Host restatement of spsamd_amg_apply and spsamd_solve_pcg_amg (include/spsparse_amd.h): the yardstick of the device cycle.

A level is a dict {"n": n_l, "S": S_l, "P": P_l, "R": R_l}: S, P and R are (rows, cols, vals) of op() as the call takes them
(tests/select_ref.operand_S), P and R None on the last level.  Every product, sum and division is rounded on its own and a
NaN result carries x86-64's bits (dense_ref.mul / add, solve_ref.sub / div).

    d_l             solve_ref.diag_fold(S_l): +0.0 and every diagonal tuple of the row added in S's order
    apply(X, m, v)  per row of X a serial chain from +0.0 in X's order (dense_ref.apply_fast, ADD), m rows
    smooth0(b)      x_i = omega * (b_i / d_i)
    smooth(b, x)    q = apply(S, x);  x'_i = x_i + omega * ((b_i - q_i) / d_i)
    cycle(l, b)     the loop of the header, recursive; trace (a list) receives (level, name, vector) for every intermediate
    pcg             the loop of spsamd_solve_pcg's header (krylov_ref.pcg) with z = cycle(0, r)
    hierarchy       levels from aggregate_ref.reference and the Galerkin operator P^T A P of the tentative prolongator, summed
                    in float64 over values that are small integers, so that every sum is exact in any order
"""
import numpy as np

from tests import aggregate_ref as ag
from tests import dense_ref as dr
from tests import krylov_ref as kr
from tests import solve_ref as sr

CONVERGED, MAXITER, BREAKDOWN = kr.CONVERGED, kr.MAXITER, kr.BREAKDOWN


def apply(X, m, v):
    return dr.apply_fast(X[0], X[1], X[2], np.asarray(v, np.float64), np.zeros(m, np.float64))


def diagonals(levels):
    return [sr.diag_fold(lv["S"], lv["n"]) for lv in levels]


def smooth0(b, d, omega):
    return dr.mul(np.float64(omega), sr.div(b, d))


def smooth(S, n, b, d, x, omega):
    q = apply(S, n, x)
    return dr.add(x, dr.mul(np.float64(omega), sr.div(sr.sub(b, q), d)))


def cycle(levels, params, b, l=0, diag=None, trace=None):
    """x = cycle(l, b).  params = (pre, post, coarse, omega)."""
    pre, post, coarse, omega = params
    diag = diagonals(levels) if diag is None else diag
    lv, d = levels[l], diag[l]
    n, S = lv["n"], lv["S"]
    b = np.asarray(b, np.float64)
    note = (lambda name, v: trace.append((l, name, np.array(v, np.float64)))) if trace is not None else (lambda name, v: None)
    x = np.zeros(n, np.float64)
    last = l == len(levels) - 1
    for s in range(coarse if last else pre):
        x = smooth0(b, d, omega) if s == 0 else smooth(S, n, b, d, x, omega)
        note("coarse" if last else "pre", x)
    if last:
        return x
    r = b.copy() if pre == 0 else sr.sub(b, apply(S, n, x))
    note("r", r)
    bc = apply(lv["R"], levels[l + 1]["n"], r)
    note("bc", bc)
    e = cycle(levels, params, bc, l + 1, diag, trace)
    x = dr.add(x, apply(lv["P"], n, e))
    note("corrected", x)
    for _ in range(post):
        x = smooth(S, n, b, d, x, omega)
        note("post", x)
    return x


def pcg(levels, params, b, x0, tol, max_iter, fold_fn=kr.fold, precond=True):
    """The loop of krylov_ref.pcg on S_0 with z = cycle(0, r) (precond False: z = r)."""
    S, n = levels[0]["S"], levels[0]["n"]
    diag = diagonals(levels) if precond else None
    b = np.asarray(b, np.float64)
    x = np.array(x0, np.float64, copy=True)
    bb = kr.dot(b, b, fold_fn)
    thresh = np.float64(dr.mul(np.float64(tol) * np.float64(tol), bb))
    r = sr.sub(b, kr.apply(S, n, x))
    rr = kr.dot(r, r, fold_fn)
    k, hist, rr0 = 0, [rr], rr
    p = np.zeros(n, np.float64)
    rz = np.float64(0.0)
    while True:
        if rr <= thresh:
            reason = CONVERGED
            break
        if k == max_iter:
            reason = MAXITER
            break
        z = cycle(levels, params, r, 0, diag) if precond else r.copy()
        rz1 = kr.dot(r, z, fold_fn)
        if k == 0:
            p = z.copy()
        else:
            beta = np.float64(sr.div(rz1, rz))
            p = dr.add(z, dr.mul(beta, p))
        rz = rz1
        if not kr.usable(rz):
            reason = BREAKDOWN
            break
        q = kr.apply(S, n, p)
        pq = kr.dot(p, q, fold_fn)
        if not kr.usable(pq):
            reason = BREAKDOWN
            break
        alpha = np.float64(sr.div(rz, pq))
        x = dr.add(x, dr.mul(alpha, p))
        r = sr.sub(r, dr.mul(alpha, q))
        rr = kr.dot(r, r, fold_fn)
        k += 1
        hist.append(rr)
    return {"x": x, "hist": np.array(hist, np.float64), "iterations": k, "reason": reason,
            "bb": np.float64(bb), "rr0": np.float64(rr0), "rr": np.float64(rr)}


def transposed(P):
    """op(P)^T row-major, storage order inside a row: what the call takes for P passed with the other flag."""
    o = np.argsort(np.asarray(P[1]), kind="stable")
    return (np.asarray(P[1])[o].astype(np.int32), np.asarray(P[0])[o].astype(np.int32), np.asarray(P[2], np.float64)[o])


def galerkin(S, agg, nc):
    """P^T S P for the tentative prolongator of agg, row-major, zero sums dropped.  Exact for small-integer values."""
    assert np.all(S[2] == np.round(S[2])) and np.abs(S[2]).sum() < 2.0 ** 52, "the exact Galerkin sum needs small integers"
    agg = np.asarray(agg, np.int64)
    key = agg[np.asarray(S[0], np.int64)] * nc + agg[np.asarray(S[1], np.int64)]
    uk, inv = np.unique(key, return_inverse=True)
    v = np.bincount(inv, weights=np.asarray(S[2], np.float64), minlength=uk.size)
    keep = v != 0.0
    uk, v = uk[keep], v[keep]
    return (uk // nc).astype(np.int32), (uk % nc).astype(np.int32), np.ascontiguousarray(v, np.float64)


def hierarchy(S, n, max_levels=32, min_coarse=10, order=ag.HASH, seed=0):
    """Unsmoothed aggregation: per level the aggregates of aggregate_ref.reference, the tentative prolongator (one 1.0 per
    row), R = P^T and the Galerkin operator; stops at max_levels or at n <= min_coarse."""
    levels = []
    while True:
        lv = {"n": n, "S": S, "P": None, "R": None}
        levels.append(lv)
        if len(levels) >= max_levels or n <= min_coarse:
            return levels
        ref = ag.reference((S[0], S[1]), n, order, seed)
        nc = ref["naggregates"]
        if nc >= n:
            return levels
        lv["P"] = (np.arange(n, dtype=np.int32), ref["agg"].astype(np.int32), np.ones(n, np.float64))
        lv["R"] = transposed(lv["P"])
        S, n = galerkin(S, ref["agg"], nc), nc
