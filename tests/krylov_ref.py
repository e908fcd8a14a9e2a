"""Host restatement of spsamd_solve_pcg (include/spsparse_amd.h): the yardstick of the device loop.

S = (rows, cols, vals) is op(A) as the call takes it, F the same of op(M) (tests/select_ref.operand_S).  Every product and
sum is rounded on its own and a NaN result carries x86-64's bits (dense_ref.mul / add, solve_ref.sub / div).

    dot(u, w)   t[e] = u[e] * w[e];  fold(t, n)
    fold(t, m)  per chunk g of 1024 elements: lane l = 0 .. 63 adds t[1024 g + 64 k + l], k = 0 .. 15 (those below m) to +0.0
                in that order; a butterfly a_l = a_l + a_{l+s} for l < s, s = 32 .. 1; the partial is a_0.  One chunk: its
                partial; else fold(partials).  The fold of nothing is +0.0.
    q = A p     per row of S a serial chain from +0.0 in S's order (dense_ref.apply_fast, ADD)
    z = M^-1 r  NONE: r | JACOBI: r / d, d = solve_ref.diag_fold(S) | LU: solve_ref.solve_fast on F, LOWER | UNIT, then
                UPPER | NONUNIT

fold_ref  the fold element by element, as written (small cases)
fold      the same, every chunk and lane at once
pcg       the loop of the header; returns a dict of x, hist, iterations, reason, bb, rr0, rr
"""
import numpy as np

from tests import dense_ref as dr
from tests import solve_ref as sr

NONE, JACOBI, LU = 0, 1, 2
CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2
CHUNK, LANES = 1024, 64


def _add(a, b):
    """One addition on Python floats (IEEE doubles, rounded once); a NaN result goes through dense_ref.add for its bits."""
    r = a + b
    return r if r == r else float(dr.add(np.float64(a), np.float64(b)))


def fold_ref(t):
    t = np.asarray(t, np.float64)
    m = t.size
    if m == 0:
        return np.float64(0.0)
    c = (m + CHUNK - 1) // CHUNK
    out = np.empty(c, np.float64)
    tl = t.tolist()
    for g in range(c):
        a = [0.0] * LANES
        for l in range(LANES):
            for k in range(CHUNK // LANES):
                e = CHUNK * g + LANES * k + l
                if e < m:
                    a[l] = _add(a[l], tl[e])
        s = LANES // 2
        while s >= 1:
            for l in range(s):
                a[l] = _add(a[l], a[l + s])
            s //= 2
        out[g] = a[0]
    return out[0] if c == 1 else fold_ref(out)


def fold(t):
    t = np.ascontiguousarray(t, np.float64)
    while True:
        m = t.size
        if m == 0:
            return np.float64(0.0)
        c = (m + CHUNK - 1) // CHUNK
        pad = np.zeros(c * CHUNK, np.float64)
        pad[:m] = t
        live = (np.arange(c * CHUNK) < m).reshape(c, CHUNK // LANES, LANES)
        pad = pad.reshape(c, CHUNK // LANES, LANES)
        a = np.zeros((c, LANES), np.float64)
        for k in range(CHUNK // LANES):
            a = np.where(live[:, k, :], dr.add(a, pad[:, k, :]), a)
        s = LANES // 2
        while s >= 1:
            a[:, :s] = dr.add(a[:, :s], a[:, s:2 * s])
            s //= 2
        if c == 1:
            return np.float64(a[0, 0])
        t = a[:, 0].copy()


def dot(u, w, fold_fn=fold):
    return fold_fn(dr.mul(np.asarray(u, np.float64), np.asarray(w, np.float64)))


def apply(S, n, p):
    return dr.apply_fast(S[0], S[1], S[2], p, np.zeros(n, np.float64))


def usable(v):
    return bool(np.isfinite(v)) and v != 0.0


def precondition(precond, S, F, n, r, d=None):
    if precond == NONE:
        return r.copy()
    if precond == JACOBI:
        return sr.div(r, sr.diag_fold(S, n) if d is None else d)
    y = sr.solve_fast(F, n, r, sr.LOWER, sr.UNIT)
    return sr.solve_fast(F, n, y, sr.UPPER, sr.NONUNIT)


def pcg(S, n, b, x0, tol, max_iter, precond=NONE, F=None, fold_fn=fold):
    b = np.asarray(b, np.float64)
    x = np.array(x0, np.float64, copy=True)
    d = sr.diag_fold(S, n) if precond == JACOBI else None
    bb = dot(b, b, fold_fn)
    thresh = np.float64(dr.mul(np.float64(tol) * np.float64(tol), bb))
    r = sr.sub(b, apply(S, n, x))
    rr = dot(r, r, fold_fn)
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
        z = precondition(precond, S, F, n, r, d)
        rz1 = dot(r, z, fold_fn)
        if k == 0:
            p = z.copy()
        else:
            beta = np.float64(sr.div(rz1, rz))
            p = dr.add(z, dr.mul(beta, p))
        rz = rz1
        if not usable(rz):
            reason = BREAKDOWN
            break
        q = apply(S, n, p)
        pq = dot(p, q, fold_fn)
        if not usable(pq):
            reason = BREAKDOWN
            break
        alpha = np.float64(sr.div(rz, pq))
        x = dr.add(x, dr.mul(alpha, p))
        r = sr.sub(r, dr.mul(alpha, q))
        rr = dot(r, r, fold_fn)
        k += 1
        hist.append(rr)
    return {"x": x, "hist": np.array(hist, np.float64), "iterations": k, "reason": reason,
            "bb": np.float64(bb), "rr0": np.float64(rr0), "rr": np.float64(rr)}


def poisson2d(g):
    """The 5-point Laplacian of a g x g grid, sorted by (row, col): (rows, cols, vals), n."""
    n = g * g
    i = np.arange(n)
    x, y = i % g, i // g
    rr, cc, vv = [i], [i], [np.full(n, 4.0)]
    for ok, off in ((y > 0, -g), (x > 0, -1), (x < g - 1, 1), (y < g - 1, g)):
        rr.append(i[ok]); cc.append(i[ok] + off); vv.append(np.full(int(ok.sum()), -1.0))
    r, c, v = np.concatenate(rr), np.concatenate(cc), np.concatenate(vv)
    o = np.lexsort((c, r))
    return (r[o].astype(np.int32), c[o].astype(np.int32), v[o]), n
