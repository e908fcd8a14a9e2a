"""Host restatement of spsamd_solve_gmres (include/spsparse_amd.h): the yardstick of the device loop.

Right-preconditioned restarted GMRES(m) on the pieces of tests/krylov_ref.py -- its fold, dot, apply, precondition and usable,
so the reduction shape, the serial chains, the rounding and the NaN bits are those of spsamd_solve_pcg's reference.  The
Arnoldi step is classical Gram-Schmidt done twice, the least-squares problem is kept triangular by Givens rotations, and
every cycle ends on b - A x recomputed: CONVERGED is only ever decided on that.  Square roots are reduce_ref.sqrt.

fold_rows  krylov_ref.fold over the rows of a matrix at once (the dots of one Gram-Schmidt pass)
gmres   the loop of the header; returns krylov_ref.pcg's dict plus `cycles`, how many cycles were begun, and `cycle_steps`,
        the steps that counted in each (a cycle may end on the estimate before j == m and the loop go on)
"""
import numpy as np

from tests import dense_ref as dr
from tests import krylov_ref as kr
from tests import reduce_ref as rr_
from tests import solve_ref as sr

NONE, JACOBI, LU = kr.NONE, kr.JACOBI, kr.LU
CONVERGED, MAXITER, BREAKDOWN = kr.CONVERGED, kr.MAXITER, kr.BREAKDOWN
MAX_RESTART = 256

f64 = np.float64


def _mul(a, b):
    return f64(dr.mul(f64(a), f64(b)))


def _add(a, b):
    return f64(dr.add(f64(a), f64(b)))


def _sub(a, b):
    return f64(sr.sub(f64(a), f64(b)))


def _div(a, b):
    return f64(sr.div(f64(a), f64(b)))


def _sqrt(a):
    return f64(rr_.sqrt(np.array([a], np.float64))[0])


def _neg(a):
    """The sign bit flipped, of a NaN too."""
    return (np.array([a], np.float64).view(np.uint64) ^ np.uint64(1 << 63)).view(np.float64)[0]


def fold_rows(T):
    """krylov_ref.fold of every row of T at once: the same chunks, lanes and butterfly, row by row the same bits."""
    T = np.ascontiguousarray(T, np.float64)
    rows = T.shape[0]
    while True:
        m = T.shape[1]
        if m == 0:
            return np.zeros(rows, np.float64)
        c = (m + kr.CHUNK - 1) // kr.CHUNK
        pad = np.zeros((rows, c * kr.CHUNK), np.float64)
        pad[:, :m] = T
        live = (np.arange(c * kr.CHUNK) < m).reshape(1, c, kr.CHUNK // kr.LANES, kr.LANES)
        pad = pad.reshape(rows, c, kr.CHUNK // kr.LANES, kr.LANES)
        a = np.zeros((rows, c, kr.LANES), np.float64)
        for k in range(kr.CHUNK // kr.LANES):
            a = np.where(live[:, :, k, :], dr.add(a, pad[:, :, k, :]), a)
        s = kr.LANES // 2
        while s >= 1:
            a[:, :, :s] = dr.add(a[:, :, :s], a[:, :, s:2 * s])
            s //= 2
        if c == 1:
            return a[:, 0, 0].copy()
        T = a[:, :, 0].copy()


def _dots(V, j, w, fold_fn):
    """[dot(v_i, w) for i = 0 .. j], all on the same w."""
    if fold_fn is kr.fold:
        return [f64(v) for v in fold_rows(dr.mul(V[:j + 1], w[None, :]))]
    return [kr.dot(V[i], w, fold_fn) for i in range(j + 1)]


def _precondition(precond, S, F, n, r, d, lev):
    if precond == NONE:
        return r                                                          # z is its input, no copy
    if precond != LU or lev is None:
        return kr.precondition(precond, S, F, n, r, d)
    y = sr.solve_fast(F, n, r, sr.LOWER, sr.UNIT, lev[0])
    return sr.solve_fast(F, n, y, sr.UPPER, sr.NONUNIT, lev[1])


def gmres(S, n, b, x0, tol, max_iter, restart, precond=NONE, F=None, fold_fn=kr.fold, lev=None):
    """lev: as bicgstab_ref.bicgstab's."""
    m = int(restart)
    assert 1 <= m <= MAX_RESTART
    b = np.asarray(b, np.float64)
    x = np.array(x0, np.float64, copy=True)
    d = sr.diag_fold(S, n) if precond == JACOBI else None
    bb = kr.dot(b, b, fold_fn)
    thresh = f64(dr.mul(f64(tol) * f64(tol), bb))
    r = sr.sub(b, kr.apply(S, n, x))
    rr = kr.dot(r, r, fold_fn)
    k, hist, rr0, cycles, cycle_steps = 0, [rr], rr, 0, []
    while True:
        if rr <= thresh:
            reason = CONVERGED
            break
        if k == max_iter:
            reason = MAXITER
            break
        if not kr.usable(rr):
            reason = BREAKDOWN
            break
        cycles += 1
        beta = _sqrt(rr)
        V = np.zeros((m, n), np.float64)
        V[0] = sr.div(r, beta)
        g = [beta] + [f64(0.0)] * m
        c, s = [f64(0.0)] * m, [f64(0.0)] * m
        R = [[f64(0.0)] * m for _ in range(m)]
        j, broken = 0, False
        while True:
            z = _precondition(precond, S, F, n, V[j], d, lev)
            w = kr.apply(S, n, z)
            h = _dots(V, j, w, fold_fn)
            for i in range(j + 1):
                w = sr.sub(w, dr.mul(h[i], V[i]))
            dd = _dots(V, j, w, fold_fn)
            for i in range(j + 1):
                w = sr.sub(w, dr.mul(dd[i], V[i]))
                h[i] = _add(h[i], dd[i])
            ww = kr.dot(w, w, fold_fn)
            hn = _sqrt(ww)
            for i in range(j):
                t = _add(_mul(c[i], h[i]), _mul(s[i], h[i + 1]))
                h[i + 1] = _sub(_mul(c[i], h[i + 1]), _mul(s[i], h[i]))
                h[i] = t
            den = _sqrt(_add(_mul(h[j], h[j]), _mul(hn, hn)))
            if not kr.usable(den):
                broken = True
                break
            c[j], s[j] = _div(h[j], den), _div(hn, den)
            for i in range(j):
                R[i][j] = h[i]
            R[j][j] = den
            g[j + 1] = _neg(_mul(s[j], g[j]))
            g[j] = _mul(c[j], g[j])
            k += 1
            j += 1
            est = _mul(g[j], g[j])
            hist.append(est)
            if est <= thresh or j == m or k == max_iter or not kr.usable(ww):
                if not np.isfinite(ww):
                    broken = True
                break
            V[j] = sr.div(w, hn)
        cycle_steps.append(j)
        if j > 0:
            y = [f64(0.0)] * j
            for i in range(j - 1, -1, -1):
                a = g[i]
                for l in range(i + 1, j):
                    a = _sub(a, _mul(R[i][l], y[l]))
                y[i] = _div(a, R[i][i])
            u = np.zeros(n, np.float64)
            for i in range(j):
                u = dr.add(u, dr.mul(y[i], V[i]))
            z = _precondition(precond, S, F, n, u, d, lev)
            x = dr.add(x, z)
            r = sr.sub(b, kr.apply(S, n, x))
            rr = kr.dot(r, r, fold_fn)
            hist[k] = rr
        if broken:
            reason = BREAKDOWN
            break
    return {"x": x, "hist": np.array(hist, np.float64), "iterations": k, "reason": reason,
            "bb": f64(bb), "rr0": f64(rr0), "rr": f64(rr), "cycles": cycles, "cycle_steps": cycle_steps}
