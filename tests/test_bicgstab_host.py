"""tests/bicgstab_ref.py pinned on the host: the loop on systems small enough to follow with a pencil, every stop reason and
both ways to CONVERGED, the solution it returns on convection-diffusion against plain numpy -- where conjugate gradients on
the same operand does not converge -- and the resource pin of the device kernels (no GPU needed for any of it)."""
import numpy as np
import pytest

from tests import bicgstab_ref as br
from tests import factor_ref as fr
from tests import krylov_ref as kr
from tests import solve_ref as sr


def _dense(rows):
    a = np.array(rows, np.float64)
    i, j = np.nonzero(a)
    return (i.astype(np.int32), j.astype(np.int32), a[i, j]), a.shape[0]


def test_loop_by_hand_2x2():
    # A = [-2 -2; -1 -2], b = (-2, 0), x0 = 0, tol = 0:
    #   k = 0: r = (-2, 0), rho = 4, p = r, v = (4, 2), rv = -8, alpha = -1/2, s = (0, 1), ss = 1, t = (-2, -2), ts = -2,
    #          tt = 8, omega = -1/4, x = (1, -1/4), r = (-1/2, 1/2), rr = 1/2, rho' = 1
    #   k = 1: beta = (1/4) 2 = 1/2, p = (-1, 3/4), v = (1/2, -1/2), rv = -1, alpha = -1, s = (0, 0), ss = 0: the half-step exit
    S, n = _dense([[-2, -2], [-1, -2]])
    b = np.array([-2.0, 0.0])
    for fold in (kr.fold, kr.fold_ref):
        got = br.bicgstab(S, n, b, np.zeros(2), 0.0, 10, fold_fn=fold)
        assert list(got["x"]) == [2.0, -1.0] and list(got["hist"]) == [4.0, 0.5, 0.0]
        assert (got["iterations"], got["reason"], got["half"]) == (2, kr.CONVERGED, True)
        assert (got["bb"], got["rr0"], got["rr"]) == (4.0, 4.0, 0.0)
        one = br.bicgstab(S, n, b, np.zeros(2), 0.0, 1, fold_fn=fold)
        assert list(one["x"]) == [1.0, -0.25] and list(one["hist"]) == [4.0, 0.5]
        assert (one["iterations"], one["reason"], one["rr"], one["half"]) == (1, kr.MAXITER, 0.5, False)


def test_a_diagonal_under_jacobi_ends_at_the_half_step():
    # y = p / d, v = A y = p = r: rv = rho, alpha = 1, s = 0.  Without the half-step exit: t = 0 and omega = 0 / 0.
    d = np.array([1.0, 2.0, 4.0, 8.0, 0.5])
    i = np.arange(5, dtype=np.int32)
    b = np.array([1.0, -2.0, 3.0, 0.5, 7.0])
    got = br.bicgstab((i, i, d), 5, b, np.zeros(5), 0.0, 10, kr.JACOBI)
    assert (got["iterations"], got["reason"], got["half"], list(got["hist"])) == (1, kr.CONVERGED, True, [63.25, 0.0])
    assert list(got["x"]) == list(b / d)


def test_stop_reasons():
    S, n = _dense([[-2, -2], [-1, -2]])
    x0 = np.array([0.5, -0.25])
    zero = br.bicgstab(S, n, np.zeros(2), np.zeros(2), 1e-6, 10)             # b = 0: 0 <= 0
    assert (zero["iterations"], zero["reason"], zero["bb"], list(zero["hist"]), zero["half"]) == (0, kr.CONVERGED, 0.0, [0.0], False)
    none = br.bicgstab(S, n, np.array([1.0, 1.0]), x0, 1e-6, 0)              # max_iter = 0
    assert (none["iterations"], none["reason"], list(none["x"])) == (0, kr.MAXITER, list(x0)) and len(none["hist"]) == 1
    at = br.bicgstab(S, n, np.array([-2.0, 0.0]), np.array([2.0, -1.0]), 0.0, 10)    # a start that is the solution
    assert (at["iterations"], at["reason"], list(at["x"]), list(at["hist"]), at["half"]) == (0, kr.CONVERGED, [2.0, -1.0], [0.0], False)
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))          # A = 0: v = 0, rv = 0
    sing = br.bicgstab(E, 2, np.array([1.0, 1.0]), x0, 1e-6, 10)
    assert (sing["iterations"], sing["reason"], list(sing["x"]), list(sing["hist"])) == (0, kr.BREAKDOWN, list(x0), [2.0])
    nan = br.bicgstab(S, n, np.array([np.nan, 1.0]), np.zeros(2), 1e-6, 10)  # a NaN compares false, then rho' is not usable
    assert (nan["iterations"], nan["reason"]) == (0, kr.BREAKDOWN) and np.isnan(nan["rr"])
    # not usable(tt): A = [1 1; 0 0] (a projection), r = (1, 1): v = (2, 0), rv = 2 = rho, alpha = 1, s = (-1, 1), ss = 2,
    # t = A s = 0
    P, _ = _dense([[1, 1], [0, 0]])
    tt = br.bicgstab(P, 2, np.array([1.0, 1.0]), np.zeros(2), 0.0, 10)
    assert (tt["iterations"], tt["reason"], list(tt["x"]), list(tt["hist"]), tt["rr"]) == (0, kr.BREAKDOWN, [0.0, 0.0], [2.0], 2.0)
    # not usable(omega) at the top of the next iteration.  In exact arithmetic rhat . s = rho - alpha rv = 0, so omega = 0
    # (r = s) would be met by rho' = 0 first; here rho = 2^60 + 1 rounds to 2^60 and rho' comes out 1.
    # A = [0 1; 0 0], b = (2^30, 1): v = (1, 0), rv = 2^30, alpha = 2^30, s = (0, 1), ss = 1, t = (1, 0), ts = 0, tt = 1,
    # omega = 0, x = (2^60, 2^30), r = s, rr = 1, rho' = 1
    N, _ = _dense([[0, 1], [0, 0]])
    om = br.bicgstab(N, 2, np.array([2.0 ** 30, 1.0]), np.zeros(2), 0.0, 10)
    assert (om["iterations"], om["reason"], list(om["x"]), list(om["hist"])) == (1, kr.BREAKDOWN, [2.0 ** 60, 2.0 ** 30], [2.0 ** 60, 1.0])
    none0 = br.bicgstab(E, 0, np.zeros(0), np.zeros(0), 1e-6, 10)            # order 0
    assert (none0["iterations"], none0["reason"], list(none0["hist"])) == (0, kr.CONVERGED, [0.0])


@pytest.mark.parametrize("g", [24, 40])
@pytest.mark.parametrize("precond", [kr.NONE, kr.JACOBI, kr.LU])
def test_the_reference_solves_convection_diffusion(g, precond):
    """Upwind convection-diffusion (cx = 2, cy = 1), tol = 1e-8: CONVERGED within 100 iterations and ||b - A x|| <=
    2 tol ||b|| in plain numpy (the factor 2 only keeps the check from being an equality: the recursive residual drifts
    from the true one far below tol ||b||).  Conjugate gradients on the same operand, with the same preconditioner and the
    same 100 iterations, is still running: the reason this loop exists."""
    S, n = br.convdiff2d(g)
    A = np.zeros((n, n))
    A[S[0], S[1]] = S[2]
    rng = np.random.default_rng(2600 + g)
    b = rng.standard_normal(n)
    tol = 1e-8
    F = lev = None
    if precond == kr.LU:
        F = (S[0], S[1], fr.ilu0_ref(S, n)[0])
        lev = (sr.levels(F, n, sr.LOWER, sr.UNIT), sr.levels(F, n, sr.UPPER, sr.NONUNIT))
    got = br.bicgstab(S, n, b, np.zeros(n), tol, 100, precond, F, lev=lev)
    assert got["reason"] == kr.CONVERGED and 0 < got["iterations"] < 100
    assert np.linalg.norm(b - A @ got["x"]) <= 2 * tol * np.linalg.norm(b)
    assert len(got["hist"]) == got["iterations"] + 1 and got["hist"][-1] == got["rr"] <= tol * tol * got["bb"]
    if precond != kr.LU or g == 24:                                       # (krylov_ref.pcg works F's levels out per solve)
        assert kr.pcg(S, n, b, np.zeros(n), tol, 100, precond, F)["reason"] == kr.MAXITER


def test_no_bicgstab_kernel_uses_scratch():
    """Every kernel of k_bicgstab.hip in the built library: no scratch, no spill (resource figures only, no GPU).  The vector
    kernels the loop shares with conjugate gradients are k_krylov.hip's (tests/test_krylov_host.py checks those)."""
    from scripts import kernel_resources
    from spsparse_amd import build
    found = {name: f for name, f in kernel_resources.library_kernels(build.build()).items() if "k_bicg" in name}
    want = ("direction", "half", "update", "finish")
    assert all(any("k_bicg_" + k in name for name in found) for k in want), sorted(found)
    for name, f in found.items():
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (name, f)
