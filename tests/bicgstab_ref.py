"""Host restatement of spsamd_solve_bicgstab (include/spsparse_amd.h): the yardstick of the device loop.

Right-preconditioned BiCGStab with rhat = r0 on the pieces of tests/krylov_ref.py -- its fold, dot, apply, precondition and
usable, so the reduction shape, the serial chains, the rounding and the NaN bits are those of spsamd_solve_pcg's reference.

bicgstab   the loop of the header; returns krylov_ref.pcg's dict plus `half`: whether the half-step exit was taken
convdiff2d the 5-point upwind convection-diffusion stencil of a g x g grid
"""
import numpy as np

from tests import dense_ref as dr
from tests import krylov_ref as kr
from tests import solve_ref as sr

NONE, JACOBI, LU = kr.NONE, kr.JACOBI, kr.LU
CONVERGED, MAXITER, BREAKDOWN = kr.CONVERGED, kr.MAXITER, kr.BREAKDOWN


def _precondition(precond, S, F, n, r, d, lev):
    if precond != LU or lev is None:
        return kr.precondition(precond, S, F, n, r, d)
    y = sr.solve_fast(F, n, r, sr.LOWER, sr.UNIT, lev[0])
    return sr.solve_fast(F, n, y, sr.UPPER, sr.NONUNIT, lev[1])


def bicgstab(S, n, b, x0, tol, max_iter, precond=NONE, F=None, fold_fn=kr.fold, lev=None):
    """lev: (levels of F's LOWER | UNIT triangle, of its UPPER | NONUNIT one) where the caller has them (solve_ref.levels);
    solve_fast works them out on every call otherwise."""
    b = np.asarray(b, np.float64)
    x = np.array(x0, np.float64, copy=True)
    d = sr.diag_fold(S, n) if precond == JACOBI else None
    f64 = np.float64
    bb = kr.dot(b, b, fold_fn)
    thresh = f64(dr.mul(f64(tol) * f64(tol), bb))
    r = sr.sub(b, kr.apply(S, n, x))
    rhat = r.copy()
    rr = kr.dot(r, r, fold_fn)
    rho1 = rr
    k, hist, rr0, half = 0, [rr], rr, False
    p = v = np.zeros(n, np.float64)
    rho = alpha = omega = f64(0.0)
    while True:
        if rr <= thresh:
            reason = CONVERGED
            break
        if k == max_iter:
            reason = MAXITER
            break
        if not kr.usable(rho1):
            reason = BREAKDOWN
            break
        if k == 0:
            p = r.copy()
        else:
            if not kr.usable(omega):
                reason = BREAKDOWN
                break
            beta = f64(dr.mul(f64(sr.div(rho1, rho)), f64(sr.div(alpha, omega))))
            p = dr.add(r, dr.mul(beta, sr.sub(p, dr.mul(omega, v))))
        rho = rho1
        y = _precondition(precond, S, F, n, p, d, lev)
        v = kr.apply(S, n, y)
        rv = kr.dot(rhat, v, fold_fn)
        if not kr.usable(rv):
            reason = BREAKDOWN
            break
        alpha = f64(sr.div(rho, rv))
        s = sr.sub(r, dr.mul(alpha, v))
        ss = kr.dot(s, s, fold_fn)
        if ss <= thresh:
            x = dr.add(x, dr.mul(alpha, y))
            rr = ss
            k += 1
            hist.append(rr)
            reason, half = CONVERGED, True
            break
        z = _precondition(precond, S, F, n, s, d, lev)
        t = kr.apply(S, n, z)
        ts = kr.dot(t, s, fold_fn)
        tt = kr.dot(t, t, fold_fn)
        if not kr.usable(tt):
            reason = BREAKDOWN
            break
        omega = f64(sr.div(ts, tt))
        x = dr.add(dr.add(x, dr.mul(alpha, y)), dr.mul(omega, z))
        r = sr.sub(s, dr.mul(omega, t))
        rr = kr.dot(r, r, fold_fn)
        rho1 = kr.dot(rhat, r, fold_fn)
        k += 1
        hist.append(rr)
    return {"x": x, "hist": np.array(hist, np.float64), "iterations": k, "reason": reason,
            "bb": np.float64(bb), "rr0": np.float64(rr0), "rr": np.float64(rr), "half": half}


def convdiff2d(g, cx=2.0, cy=1.0):
    """Upwind convection-diffusion on a g x g grid, sorted by (row, col): diagonal 4 + cx + cy, west -1 - cx, south -1 - cy,
    east and north -1.  (rows, cols, vals), n."""
    n = g * g
    i = np.arange(n)
    x, y = i % g, i // g
    rr, cc, vv = [i], [i], [np.full(n, 4.0 + cx + cy)]
    for ok, off, w in ((y > 0, -g, -1.0 - cy), (x > 0, -1, -1.0 - cx), (x < g - 1, 1, -1.0), (y < g - 1, g, -1.0)):
        rr.append(i[ok]); cc.append(i[ok] + off); vv.append(np.full(int(ok.sum()), w))
    r, c, v = np.concatenate(rr), np.concatenate(cc), np.concatenate(vv)
    o = np.lexsort((c, r))
    return (r[o].astype(np.int32), c[o].astype(np.int32), v[o]), n
