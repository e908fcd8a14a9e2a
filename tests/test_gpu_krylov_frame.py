"""What spsamd_solve_pcg, spsamd_solve_bicgstab and spsamd_solve_pcg_amg do alike around their iteration bodies, pinned for
all three in one table through the public calls: the launches of an iteration, the read-backs, the analyses of a raw factor
and a workspace that does not grow with the iteration count.  The returned bits are pinned by tests/test_gpu_krylov.py,
test_gpu_bicgstab.py and test_gpu_amg.py; here only counts are read.

Every case runs tol = 0, max_iter = 3 and pcg_check_every 1: the stop is MAXITER after exactly three enqueued iterations,
so stats.launches is three times what one iteration enqueues.  (At order 1 the Jacobi and the LU preconditioner are A^-1
itself and r is exactly 0 after the first iteration -- tests/krylov_ref.py and bicgstab_ref.py say so for this system --,
so there the stop is CONVERGED at k = 1; with a read of the state after every iteration nothing more is enqueued either.)
What an iteration enqueues, counted in the loops' text (k_krylov.hip, k_bicgstab.hip); a `finish` is the one-workgroup
kernel that folds a dot's partials and sets the scalar:

conjugate gradients, pcg_fuse 0 (every dot rides in the kernel that produces its vector)
    none     RZ finish, direction, SpMV, PQ finish, update, RR finish                                   6
    Jacobi   the division (with dot(r, z) inside) before them                                           7
    LU       the two level-scheduled solves (T launches, measured) and k_pcg_dot(r, z) before them      7 + T
    hook     the cycle (C launches, measured) and k_pcg_dot(r, z) before them                           7 + C
conjugate gradients, pcg_fuse 1 (every vector operation and every dot a launch of its own)
    none     RZ finish, direction, SpMV, dot(p, q), PQ finish, x update, r update, dot(r, r), RR finish 9
    Jacobi   the division and dot(r, z) before them                                                     11
    LU       T and dot(r, z) before them                                                                10 + T
    hook     C and dot(r, z) before them                                                                10 + C
BiCGStab, pcg_fuse 0
    none     direction, SpMV, RV finish, half step, SS finish, SpMV, TS_TT finish, update, RR_RHO finish 9
    Jacobi   a division before each SpMV (no dot follows either)                                        11
    LU       T before each SpMV                                                                         9 + 2 T
BiCGStab, pcg_fuse 1
    none     direction, SpMV, dot, RV finish, half step, dot, SS finish, SpMV, dot, dot, TS_TT finish,
             x update, r update, dot, dot, RR_RHO finish                                                16
    Jacobi   two divisions                                                                              18
    LU                                                                                                  16 + 2 T
a long row in S (no more long rows than chunks), per SpMV of an iteration -- one in conjugate gradients, two in BiCGStab
    pcg_fuse 0   the wave kernel over the long rows, then the partials of their chunks redone           + 2
    pcg_fuse 1   the wave kernel over the long rows (the whole dot runs anyway)                         + 1
"""
import numpy as np
import pytest

from tests import amg_ref as am
from tests.gpu_util import Knobs, coo as _coo, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

NONE, JACOBI, LU, HOOK = 0, 1, 2, 3
#        (loop, precond): (launches of an iteration net of T / C under pcg_fuse 0, under pcg_fuse 1, applications of M^-1)
OWN = {("pcg", NONE): (6, 9, 0), ("pcg", JACOBI): (7, 11, 0), ("pcg", LU): (7, 10, 1), ("pcg", HOOK): (7, 10, 1),
       ("bicgstab", NONE): (9, 16, 0), ("bicgstab", JACOBI): (11, 18, 0), ("bicgstab", LU): (9, 16, 2)}
LONG_ROW = (2, 1)                  # per SpMV, under pcg_fuse 0 and 1
SPMVS = {"pcg": 1, "bicgstab": 2}
PARAMS = (1, 1, 2, 2.0 / 3.0)      # the hook's cycle: V(1,1), two coarse sweeps
ORDERS = (1, 1024, 1025, 3000)     # one chunk, one full chunk, two chunks; three chunks with a long row
ARROW = 3000


def _system(n):
    """(S, b): a symmetric, strictly diagonally dominant band (offsets 1 and 32) of small integers, sorted by (row, col);
    at order ARROW row 0 and column 0 are full as well, so row 0 is above spmm_long_min."""
    i = np.arange(n)
    rr, cc, vv = [i], [i], [49.0 + i % 5]
    offs = [(i[off:], i[:n - off]) for off in (1, 32) if off < n]
    if n == ARROW:
        vv[0] = vv[0].copy()
        vv[0][0] = n + 49.0
        far = i[(i > 1) & (i != 32)]                                       # (1 and 32 are in the band already)
        offs.append((far, np.zeros(far.size, np.int64)))
    for lo, hi in offs:
        rr += [lo, hi]; cc += [hi, lo]; vv += [np.full(lo.size, -1.0)] * 2
    r, c, v = np.concatenate(rr), np.concatenate(cc), np.concatenate(vv)
    o = np.lexsort((c, r))
    return (r[o].astype(np.int32), c[o].astype(np.int32), v[o]), 1.0 + 0.25 * (i % 7)


def _two_levels(S, n):
    """S with the aggregates {2 k, 2 k + 1}: the tentative prolongator, its transpose and the Galerkin operator."""
    agg, nc = np.arange(n) // 2, (n + 1) // 2
    P = (np.arange(n, dtype=np.int32), agg.astype(np.int32), np.ones(n))
    return [(S, (n, n)), (P, (n, nc)), (am.transposed(P), (nc, n)), (am.galerkin(S, agg, nc), (nc, nc))]


@pytest.mark.parametrize("n", ORDERS)
def test_what_the_frame_owns(ctx, n):
    from spsparse_amd import capi
    S, b = _system(n)
    keep = []
    a = _coo(S, (n, n), keep=keep)
    # the factor, raw on the host (so each call analyses both triangles), and T by one stand-alone solve per triangle
    f = _coo(ctx.fetch(ctx.factor_ilu0(a)), (n, n), keep=keep)
    T = sum(int(ctx.solve_tri(f, b, uplo, diag, stats=True)[1].launches)
            for uplo, diag in ((capi.TRI_LOWER, capi.DIAG_UNIT), (capi.TRI_UPPER, capi.DIAG_NONUNIT)))
    # the two-level hierarchy, and C by one stand-alone cycle
    A0, P0, R0, A1 = (_coo(X, shape, keep=keep) for X, shape in _two_levels(S, n))
    levels = [(A0, '.', P0, '.', R0, '.'), (A1, '.', None, '.', None, '.')]
    Cy = int(ctx.amg_apply(levels, PARAMS, b)[1].launches_per_cycle)
    assert T >= 2 and Cy >= 1
    has_long = n == ARROW

    def run(loop, precond, max_iter):
        res, x = capi.Result(), np.zeros(n)
        if precond == HOOK:
            _, _, st, _ = ctx.solve_pcg_amg(levels, PARAMS, b, x, 0.0, max_iter, 2, result=res)
        else:
            call = ctx.solve_pcg if loop == "pcg" else ctx.solve_bicgstab
            _, _, st = call(a, b, x, precond, f if precond == LU else None, tol=0.0, max_iter=max_iter, hist_capacity=2, result=res)
        return st, int(res.workspace_bytes)

    for (loop, precond), (fused, unfused, applications) in OWN.items():
        for fuse in (0, 1):
            what = "n %d %s precond %d pcg_fuse %d" % (n, loop, precond, fuse)
            with Knobs(ctx, {"pcg_check_every": 1, "pcg_fuse": fuse}):
                st, used = run(loop, precond, 3)
                st1, used1 = run(loop, precond, 1)
            exact = n == 1 and precond in (JACOBI, LU)                        # M^-1 is A^-1: rr = 0 at k = 1
            stop = (1, capi.PCG_CONVERGED) if exact else (3, capi.PCG_MAXITER)
            assert (st.iterations, st.reason) == stop, "%s: stop (%d, %d)" % (what, st.iterations, st.reason)
            assert (st1.iterations, st1.reason) == (1, stop[1]), what
            want = (unfused if fuse else fused) + applications * (Cy if precond == HOOK else T) + has_long * SPMVS[loop] * LONG_ROW[fuse]
            print("%s: launches %d iterations %d, want %d per iteration; readbacks %d analyses %d workspace %d %d" % (
                what, st.launches, st.iterations, want, st.readbacks, st.analyses, used, used1))
            assert st.launches // st.iterations == want and st.launches % st.iterations == 0, "%s: %d launches" % (what, st.launches)
            assert st1.launches == want, what
            assert st.readbacks == st.iterations + 1 and st1.readbacks == 2, what
            assert st.analyses == st1.analyses == (2 if precond == LU else 0), what
            assert used == used1 and used > 0, "%s: workspace %d, %d" % (what, used, used1)
