"""tests/gmres_ref.py pinned on the host: the loop on systems small enough to follow with a pencil, every stop reason, a
cycle ended by the estimate and one by max_iter, the step and cycle counts on convection-diffusion with the true residual
through plain numpy -- where BiCGStab on the same operand reports CONVERGED on a residual it does not have -- and the
resource pin of the device kernels (no GPU needed for any of it)."""
import numpy as np
import pytest

from tests import bicgstab_ref as br
from tests import gmres_ref as gr
from tests import krylov_ref as kr


def _dense(rows):
    a = np.array(rows, np.float64)
    i, j = np.nonzero(a)
    return (i.astype(np.int32), j.astype(np.int32), a[i, j]), a.shape[0]


E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))


def test_fold_rows_is_the_fold_of_every_row():
    rng = np.random.default_rng(2700)
    for m in (0, 1, 63, 64, 65, 1024, 1025, 3000, 1024 * 1024 + 5):
        T = rng.standard_normal((3, m)) * 10.0 ** rng.integers(-8, 9, (3, m))
        if m > 2:
            T[1, 2] = np.nan
        got = gr.fold_rows(T)
        want = np.array([kr.fold(T[i]) for i in range(3)])
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), m


def test_loop_by_hand_2x2():
    # A = [0 1; 2 1], b = (2, 0), x0 = 0, tol = 0, m = 2:
    #   top:   rr = 4, beta = 2, v_0 = (1, 0), g = (2)
    #   j = 0: w = A v_0 = (0, 2), h_0 = 0, w = (0, 2), d_0 = 0, ww = 4, hn = 2, den = sqrt(0 + 4) = 2, c_0 = 0, s_0 = 1,
    #          R00 = 2, g = (0, -2), k = 1, est = 4, v_1 = (0, 1)
    #   j = 1: w = A v_1 = (1, 1), h = (1, 1), w = (0, 0), d = (0, 0), ww = 0, hn = 0; the rotation: t = 0*1 + 1*1 = 1,
    #          h_1 = 0*1 - 1*1 = -1, h_0 = 1; den = sqrt(1 + 0) = 1, c_1 = -1, s_1 = 0, R01 = 1, R11 = 1,
    #          g_2 = -(0 * -2) = +0.0, g_1 = (-1)(-2) = 2, k = 2, est = 0 <= thresh
    #   end:   y_1 = 2 / 1 = 2, y_0 = (0 - 1*2) / 2 = -1, u = -1 (1, 0) + 2 (0, 1) = (-1, 2) = x, r = b - A x = 0, rr = 0
    S, n = _dense([[0, 1], [2, 1]])
    b = np.array([2.0, 0.0])
    for fold in (kr.fold, kr.fold_ref):
        got = gr.gmres(S, n, b, np.zeros(2), 0.0, 10, 2, fold_fn=fold)
        assert list(got["x"]) == [-1.0, 2.0] and list(got["hist"]) == [4.0, 4.0, 0.0]
        assert (got["iterations"], got["reason"], got["cycles"]) == (2, kr.CONVERGED, 1)
        assert (got["bb"], got["rr0"], got["rr"]) == (4.0, 4.0, 0.0)
        # max_iter = 1 ends the cycle after j = 0: y_0 = g_0 / R00 = 0 / 2, x = 0, and the true rr = 4 replaces est = 4
        one = gr.gmres(S, n, b, np.zeros(2), 0.0, 1, 2, fold_fn=fold)
        assert list(one["x"]) == [0.0, 0.0] and list(one["hist"]) == [4.0, 4.0]
        assert (one["iterations"], one["reason"], one["rr"], one["cycles"]) == (1, kr.MAXITER, 4.0, 1)
    # m = 1: every step is a cycle, and each one returns y_0 = 0: stagnation ends in MAXITER
    stag = gr.gmres(S, n, b, np.zeros(2), 0.0, 5, 1)
    assert (stag["iterations"], stag["reason"], stag["cycles"], list(stag["hist"]), list(stag["x"])) == (
        5, kr.MAXITER, 5, [4.0] * 6, [0.0, 0.0])


def test_a_diagonal_under_jacobi_ends_at_step_one():
    # z = v_0 / d, w = A z = v_0 up to rounding: after the two passes of Gram-Schmidt nothing usable is left of w, and
    # x = M^-1 (y_0 v_0) = b / d
    d = np.arange(1.0, 8.0)
    i = np.arange(7, dtype=np.int32)
    b = d * d
    got = gr.gmres((i, i, d), 7, b, np.zeros(7), 1e-12, 10, 5, kr.JACOBI)
    assert (got["iterations"], got["reason"], got["cycles"], list(got["hist"])) == (1, kr.CONVERGED, 1, [4676.0, 0.0])
    assert list(got["x"]) == list(d)


def test_order_one_and_an_empty_operand():
    # n = 1: A = (2), b = (3): beta = 3, v_0 = 1, w = 2, h_0 = 2, w = 0, hn = 0, den = 2, c_0 = 1, s_0 = 0, g = (3, -0.0),
    # est = 0, y_0 = 3 / 2
    S, n = _dense([[2]])
    got = gr.gmres(S, n, np.array([3.0]), np.zeros(1), 1e-8, 10, 4)
    assert (got["iterations"], got["reason"], got["cycles"], list(got["hist"]), list(got["x"])) == (1, kr.CONVERGED, 1, [9.0, 0.0], [1.5])
    # A = 0: w = 0, every h is 0, den = 0 is not usable: the step is discarded, j == 0 and x stays
    x0 = np.array([0.5, -0.25])
    sing = gr.gmres(E, 2, np.array([1.0, 1.0]), x0, 1e-6, 10, 3)
    assert (sing["iterations"], sing["reason"], sing["cycles"], list(sing["x"]), list(sing["hist"])) == (0, kr.BREAKDOWN, 1, list(x0), [2.0])
    none0 = gr.gmres(E, 0, np.zeros(0), np.zeros(0), 1e-6, 10, 3)           # order 0
    assert (none0["iterations"], none0["reason"], list(none0["hist"])) == (0, kr.CONVERGED, [0.0])


def test_the_cyclic_shift():
    # A e_i = e_{i+1 mod 6}, b = e_0: the Krylov vectors are e_0, e_1, ...; every h_i is 0 and hn = 1 until the space is
    # whole, so every estimate is 1 and nothing shorter than m = 6 moves x at all
    n = 6
    i = np.arange(n, dtype=np.int32)
    S = (((i + 1) % n).astype(np.int32), i, np.ones(n))
    o = np.lexsort((S[1], S[0]))
    S = (S[0][o], S[1][o], S[2][o])
    b = np.zeros(n)
    b[0] = 1.0
    two = gr.gmres(S, n, b, np.zeros(n), 1e-8, 8, 2)
    assert (two["iterations"], two["reason"], two["cycles"], list(two["hist"]), list(two["x"])) == (8, kr.MAXITER, 4, [1.0] * 9, [0.0] * n)
    six = gr.gmres(S, n, b, np.zeros(n), 1e-8, 8, 6)
    assert (six["iterations"], six["reason"], six["cycles"], list(six["hist"])) == (6, kr.CONVERGED, 1, [1.0] * 6 + [0.0])
    assert list(six["x"]) == [0.0] * 5 + [1.0]                              # A e_5 = e_0


def test_stop_reasons():
    S, n = _dense([[0, 1], [2, 1]])
    x0 = np.array([0.5, -0.25])
    zero = gr.gmres(S, n, np.zeros(2), np.zeros(2), 1e-6, 10, 2)             # b = 0: 0 <= 0
    assert (zero["iterations"], zero["reason"], zero["bb"], list(zero["hist"]), zero["cycles"]) == (0, kr.CONVERGED, 0.0, [0.0], 0)
    none = gr.gmres(S, n, np.array([1.0, 1.0]), x0, 1e-6, 0, 2)              # max_iter = 0
    assert (none["iterations"], none["reason"], list(none["x"]), none["cycles"]) == (0, kr.MAXITER, list(x0), 0) and len(none["hist"]) == 1
    at = gr.gmres(S, n, np.array([2.0, 0.0]), np.array([-1.0, 2.0]), 0.0, 10, 2)     # a start that is the solution
    assert (at["iterations"], at["reason"], list(at["x"]), list(at["hist"])) == (0, kr.CONVERGED, [-1.0, 2.0], [0.0])
    nan = gr.gmres(S, n, np.array([np.nan, 1.0]), np.zeros(2), 1e-6, 10, 2)  # a NaN compares false, then rr is not usable
    assert (nan["iterations"], nan["reason"], nan["cycles"]) == (0, kr.BREAKDOWN, 0) and np.isnan(nan["rr"])
    # h_0 * h_0 overflows: A = 1e200 I, b = (1, 1): h_0 is about 1e200 and den = sqrt(Inf) is not usable; the step is discarded
    # at j == 0 and x stays
    B, _ = _dense([[1e200, 0], [0, 1e200]])
    big = gr.gmres(B, 2, np.array([1.0, 1.0]), x0 * 0, 1e-6, 10, 2)
    assert (big["iterations"], big["reason"], big["cycles"], list(big["x"]), list(big["hist"])) == (0, kr.BREAKDOWN, 1, [0.0, 0.0], [2.0])
    # a breakdown after a step that counts: A = [1 1; 0 0] (a projection), b = (1, 1), which no x solves.  j = 0: v_0 =
    # (1, 1) / sqrt 2, w = (sqrt 2, 0), the step counts and brings x = (1/2, 1/2), rr = 1; at j = 1 w = A v_1 lies in the span
    # of v_0 and v_1, nothing is left of it and den is not usable: the cycle ends with j == 1, x moves, then BREAKDOWN
    P, _ = _dense([[1, 1], [0, 0]])
    pr = gr.gmres(P, 2, np.array([1.0, 1.0]), np.zeros(2), 1e-10, 10, 2)
    assert (pr["iterations"], pr["reason"], pr["cycles"], list(pr["hist"]), pr["rr"]) == (1, kr.BREAKDOWN, 1, [2.0, 1.0], 1.0)
    assert pr["x"][0] == pr["x"][1] and abs(pr["x"][0] - 0.5) <= 2.0 ** -52      # (sqrt 2 is rounded)


def test_cycles_ended_by_the_estimate_and_by_max_iter():
    S, n = br.convdiff2d(12)
    b = kr.apply(S, n, np.ones(n))
    est = gr.gmres(S, n, b, np.zeros(n), 1e-3, 500, 30)                      # est <= thresh at a step that is no multiple of m
    assert est["reason"] == kr.CONVERGED and est["iterations"] % 30 != 0
    assert est["cycles"] == est["iterations"] // 30 + 1 and len(est["hist"]) == est["iterations"] + 1
    assert est["hist"][-1] == est["rr"] <= 1e-6 * est["bb"]
    cut = gr.gmres(S, n, b, np.zeros(n), 1e-14, 7, 5)                        # k == max_iter at j == 2 of the second cycle
    assert (cut["iterations"], cut["reason"], cut["cycles"]) == (7, kr.MAXITER, 2)
    five = gr.gmres(S, n, b, np.zeros(n), 1e-14, 5, 5)                       # ... whose first cycle is that of max_iter = 5
    assert np.array_equal(cut["hist"][:6], five["hist"]) and cut["hist"][7] == cut["rr"]
    assert np.all(np.diff(cut["hist"][:6]) <= 0) and max(cut["hist"]) <= cut["rr0"]
    # the true value of a cycle's last step is the estimate up to rounding
    four = gr.gmres(S, n, b, np.zeros(n), 1e-14, 4, 5)
    assert abs(four["hist"][4] - five["hist"][4]) <= 1e-9 * five["hist"][4] and np.array_equal(four["hist"][:4], five["hist"][:4])


def test_a_cycle_that_ends_on_the_estimate_and_goes_on():
    """The estimate and the true residual part ways at rounding level: a cycle ends on est <= thresh (or with the Krylov space
    whole, restart > n), the recomputed rr is still above the threshold, and the loop begins another cycle from it --
    `goto cycle` in the header.  The steps of each cycle are pinned; tests/test_gpu_gmres.py runs the same cases."""
    S, n = _dense([[0, 0, 1], [0, 1, -1], [-1, 3, 3]])
    b = np.array([1.0, 2.0, 3.0])
    for max_iter in (4, 5, 12):                                              # the trajectory does not depend on max_iter >= 4
        got = gr.gmres(S, n, b, np.zeros(3), 1e-15, max_iter, 5)
        assert (got["iterations"], got["reason"], got["cycles"], got["cycle_steps"]) == (4, kr.CONVERGED, 2, [3, 1])
        assert got["hist"][3] > 1e-30 * got["bb"] >= got["hist"][4] == got["rr"]   # the first cycle's true rr missed the threshold
    cut = gr.gmres(S, n, b, np.zeros(3), 1e-15, 3, 5)                        # ... and max_iter = 3 stops on that rr
    assert (cut["iterations"], cut["reason"], cut["cycle_steps"]) == (3, kr.MAXITER, [3])
    S, n = _dense([[-1, -3, 2], [-1, 0, -1], [-2, 1, -1]])
    got = gr.gmres(S, n, np.array([-3.0, 3.0, 1.0]), np.zeros(3), 1e-16, 6, 6)       # restart > n, then MAXITER
    assert (got["iterations"], got["reason"], got["cycle_steps"]) == (6, kr.MAXITER, [3, 3])
    S, n = _dense([[-1, 2, -1], [1, 2, 2], [-3, 3, 2]])
    got = gr.gmres(S, n, np.array([1.0, -2.0, 3.0]), np.zeros(3), 1e-16, 6, 3)       # a short second cycle, the third cut by max_iter
    assert (got["iterations"], got["reason"], got["cycle_steps"]) == (6, kr.MAXITER, [3, 2, 1])


COUNTS = {24: (150, 5), 40: (269, 9), 128: (581, 20)}                       # GMRES(30), tol = 1e-8, b = A 1: (steps, cycles)


@pytest.mark.parametrize("g", sorted(COUNTS))
def test_the_reference_solves_convection_diffusion(g):
    """Upwind convection-diffusion (cx = 2, cy = 1), b = A 1, x0 = 0, tol = 1e-8, no preconditioner, m = 30: the step and
    cycle counts, a history that never exceeds rr0, and ||b - A x|| <= tol (1 + 1e-9) ||b|| through plain numpy (the stop
    is on the recomputed residual: the slack is for the two ways of summing it).  At 128^2 BiCGStab on the same system
    reports CONVERGED with a true residual above 100 tol: the reason this loop exists."""
    S, n = br.convdiff2d(g)
    b = kr.apply(S, n, np.ones(n))
    tol = 1e-8

    def true_rel(x):
        ax = np.zeros(n)
        np.add.at(ax, S[0], S[2] * x[S[1]])
        return np.linalg.norm(b - ax) / np.linalg.norm(b)

    got = gr.gmres(S, n, b, np.zeros(n), tol, 10000, 30)
    assert (got["iterations"], got["cycles"], got["reason"]) == COUNTS[g] + (kr.CONVERGED,)
    assert max(got["hist"]) <= got["rr0"] and len(got["hist"]) == got["iterations"] + 1
    assert got["hist"][-1] == got["rr"] <= tol * tol * got["bb"]
    assert true_rel(got["x"]) <= tol * (1 + 1e-9)
    if g == 128:
        bi = br.bicgstab(S, n, b, np.zeros(n), tol, 10000)
        assert bi["reason"] == kr.CONVERGED and true_rel(bi["x"]) > 100 * tol


def test_jacobi_changes_no_count_on_a_constant_diagonal():
    S, n = br.convdiff2d(24)
    b = kr.apply(S, n, np.ones(n))
    got = gr.gmres(S, n, b, np.zeros(n), 1e-8, 10000, 30, kr.JACOBI)
    assert (got["iterations"], got["cycles"], got["reason"]) == COUNTS[24] + (kr.CONVERGED,)


def test_no_gmres_kernel_uses_scratch():
    """Every kernel of k_gmres.hip in the built library: no scratch, no spill (resource figures only, no GPU)."""
    from scripts import kernel_resources
    from spsparse_amd import build
    found = {name: f for name, f in kernel_resources.library_kernels(build.build()).items() if "k_gmres" in name}
    want = ("project", "fold", "subtract", "hess", "scale", "backsub", "combine", "addx", "finish")
    assert all(any("k_gmres_" + k in name for name in found) for k in want), sorted(found)
    for name, f in found.items():
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (name, f)
