"""spsamd_solve_gmres on the device against tests/gmres_ref.py (pinned on the host by tests/test_gmres_host.py): x, the
history, the step count, the stop reason, bb, rr0 and rr, every float as an int64 bit pattern with zero tolerance -- each is
defined by the loop of the header, reduction shape included, so there is nothing to tolerate.  The gmres_path knob runs so
that the block kernels and the launch-per-operation shape meet one definition.  The operand makers and the comparison are
those of tests/test_gpu_krylov.py."""
import ctypes as C

import numpy as np
import pytest

from tests import add_ref as ar
from tests import bicgstab_ref as br
from tests import factor_ref as fr
from tests import gmres_ref as gr
from tests import krylov_ref as kr
from tests import select_ref as sel
from tests.gpu_util import Knobs, coo as _coo, ctx  # noqa: F401
from tests.test_gpu_krylov import EDGES, KINDS, SENT, _matrix, _mixed, _operand, _same

pytestmark = pytest.mark.gpu


def _run(ctx, a, b, x0, precond=kr.NONE, m=None, tA='.', tM='.', tol=1e-8, max_iter=100, restart=30, pol=ar.ADD, zn=False,
         device=False, cap=None, result=None):
    """One call; b is checked untouched.  Returns (the dict gmres_ref.gmres returns, cycles = readbacks - 1; PcgStats)."""
    b = np.ascontiguousarray(b, np.float64)
    if device:
        import torch
        tb, tx = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(np.array(x0, np.float64)).cuda()
        torch.cuda.synchronize()
        _, hist, st = ctx.solve_gmres(a, tb, tx, precond, m, tA, tM, tol, max_iter, restart, cap, pol, zn, result)
        gx, gb = tx.cpu().numpy(), tb.cpu().numpy()
    else:
        gb, gx = b.copy(), np.array(x0, np.float64)
        _, hist, st = ctx.solve_gmres(a, gb, gx, precond, m, tA, tM, tol, max_iter, restart, cap, pol, zn, result)
    assert np.array_equal(gb.view(np.int64), b.view(np.int64)), "b was written"
    got = {"x": gx, "hist": hist, "iterations": int(st.iterations), "reason": int(st.reason),
           "bb": np.float64(st.bb), "rr0": np.float64(st.rr0), "rr": np.float64(st.rr), "cycles": int(st.readbacks) - 1}
    return got, st


def _same_all(got, want, what, hist=True):
    _same(got, want, what, hist)
    assert got["cycles"] == want["cycles"], "%s: %d cycles, want %d" % (what, got["cycles"], want["cycles"])


# ---------------------------------------------------------------- the semantic fuzz

RESTARTS = (1, 2, 5, 64)


def test_semantic_fuzz(ctx):
    """120 operands of order 1 .. 40.  The kind is the trial's base-5 digit; the digits above it run through the 24
    (precond, gmres_path, restart) settings -- restart 64 is above every order, so the Krylov space is exhausted -- and, on
    other periods, through the transposes, the memory of the vectors and the four operand forms, so every kind meets every
    value of every setting; the coverage is asserted, the three reasons, a cycle ended by the estimate, a cycle ended by
    max_iter, a BREAKDOWN before the first step and a cycle that ended early with the loop going on (tol 1e-15 is there for
    that: the estimate and the true residual part ways at rounding level) included."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2712)
    seen, ends = set(), set()
    for trial in range(120):
        kind, j = trial % 5, trial // 5
        precond, path, restart = j % 3, (j // 3) % 2, RESTARTS[(j // 6) % 4]
        tA, tM = '.T'[j % 2], '.T'[(j // 3) % 2]
        device, form_a, form_m = bool((j // 2) % 2), (j + j // 4) % 4, (j // 3 + j // 12) % 4
        n = int(rng.integers(1, 41))
        pol, zn = int(rng.integers(3)), bool(rng.integers(5) == 0)
        tol = (0.0, 1e-6, 1e-2, 1e-15)[int(rng.integers(4))]
        max_iter = (0, 1, 3, 25)[int(rng.integers(4))] if kind > 1 else 45
        keep, handles = [], []
        what = "trial %d n %d %s precond %d path %d restart %d %s %s dev %d forms %d %d pol %d zn %d tol %g max %d" % (
            trial, n, KINDS[kind], precond, path, restart, tA, tM, device, form_a, form_m, pol, zn, tol, max_iter)
        try:
            a, S = _operand(ctx, _matrix(rng, n, kind), n, tA, form_a, pol, zn, keep, handles)
            m = F = None
            if precond == kr.LU:
                if form_a == 2 and form_m == 2:                        # both chained: M is the factor of A, in the other output set
                    res = ctx.factor_ilu0(a, tA, pol, zn)
                    m, F = capi.result_operand(res), sel.operand_S(ctx.fetch(res), tM, pol, zn, 0)
                else:
                    if kind < 2:                                       # the factor of A itself (its keys sorted: a trusted S is not)
                        Ss = fr.sorted_unique(*S)
                        D = (Ss[0], Ss[1], fr.ilu0_ref(Ss, n)[0])
                    else:
                        D = _matrix(rng, n, 1)
                    m, F = _operand(ctx, D, n, tM, form_m, pol, zn, keep, handles)
            b = rng.standard_normal(n)
            if kind == 4 and rng.integers(3) == 0:
                b[int(rng.integers(n))] = (np.nan, np.inf, -0.0)[int(rng.integers(3))]
            x0 = np.zeros(n) if rng.integers(2) else rng.standard_normal(n)
            want = gr.gmres(S, n, b, x0, tol, max_iter, restart, precond, F)
            with Knobs(ctx, {"gmres_path": path}):
                got, st = _run(ctx, a, b, x0, precond, m, tA, tM, tol, max_iter, restart, pol, zn, device)
            _same_all(got, want, what)
            assert st.analyses == (0 if precond != kr.LU else 2), what        # (no handle here was solved with before)
            if precond == kr.LU and form_m == 3:                               # ... and now M's handle has both schedules
                before = handles[-1].bytes
                with Knobs(ctx, {"gmres_path": path}):
                    again, st2 = _run(ctx, a, b, x0, precond, m, tA, tM, tol, max_iter, restart, pol, zn, device)
                _same_all(again, want, what + " again")
                assert st2.analyses == 0 and handles[-1].bytes == before, what
        finally:
            for h in handles:
                h.close()
        k = want["iterations"]
        ends.add(("reason", want["reason"]))
        if want["reason"] == kr.CONVERGED and 0 < k < max_iter and k % restart:
            ends.add("estimate")                                       # the last cycle ended before j == m, and not by max_iter
        if want["reason"] == kr.MAXITER and k % restart:
            ends.add("max_iter")                                       # ... by k == max_iter before j == m
        if want["reason"] == kr.BREAKDOWN and k == 0:
            ends.add("breakdown at 0")
        if restart > n and k >= n:
            ends.add("exhausted")
        if any(c < restart for c in want["cycle_steps"][:-1]):
            ends.add("continued")                                      # a cycle ended before j == m and the loop went on
        seen.add(("set", kind, precond, path, restart)); seen.add(("tA", kind, tA)); seen.add(("dev", kind, device))
        seen.add(("fa", kind, form_a))
        if precond == kr.LU:
            seen.add(("tM", kind, tM)); seen.add(("fm", kind, form_m))
    count = lambda tag: len([s for s in seen if s[0] == tag])
    assert count("set") == 5 * 24 and count("tA") == 10 and count("dev") == 10 and count("fa") == 20
    assert count("tM") == 10 and count("fm") == 20
    assert {e[1] for e in ends if e[0] == "reason"} == {kr.CONVERGED, kr.MAXITER, kr.BREAKDOWN}
    assert {"estimate", "max_iter", "breakdown at 0", "exhausted", "continued"} <= ends, ends


# ---------------------------------------------------------------- the folds and the chunks at their edges

@pytest.mark.parametrize("n", EDGES)
def test_fold_and_chunk_edges(ctx, n):
    """An upper bidiagonal A with b of mixed magnitudes, restart 3 and max_iter 5: two cycles, the second cut by max_iter, and
    the block kernels at j = 0, 1, 2 -- the projection, the per-vector folds over one, two and three levels, both
    subtractions, the scale and the combination meet every chunk edge.  Plain and Jacobi, on both paths."""
    rng = np.random.default_rng(2720 + n % 1000)
    b = _mixed(rng, n)
    keep = []
    d = np.arange(n, dtype=np.int32)
    D = fr.sorted_unique(np.r_[d, d[:-1]], np.r_[d, d[1:]], np.r_[1.0 + rng.random(n), 0.25 * rng.random(n - 1)])
    x0 = rng.standard_normal(n)
    a = _coo(D, (n, n), 0, device=True, keep=keep)
    for precond in (kr.NONE, kr.JACOBI):
        want = gr.gmres(D, n, b, x0, 0.0, 5, 3, precond)
        assert (want["iterations"], want["cycles"]) == (5, 2) or n == 1
        for path in (0, 1):
            with Knobs(ctx, {"gmres_path": path}):
                got, _ = _run(ctx, a, b, x0, precond, tol=0.0, max_iter=5, restart=3, device=True)
            _same_all(got, want, "bidiagonal A, n %d precond %d path %d" % (n, precond, path))


def test_the_block_at_its_cap(ctx):
    """n = 1500, restart = max_iter = 256: one cycle whose last step folds 256 arrays in one launch, with R at full size and
    the back substitution over 256 rows."""
    from spsparse_amd import capi
    assert capi.GMRES_MAX_RESTART == gr.MAX_RESTART == 256
    n = 1500
    rng = np.random.default_rng(2730)
    S = fr.sorted_unique(np.r_[np.arange(n), rng.integers(0, n, 3 * n)], np.r_[np.arange(n), rng.integers(0, n, 3 * n)],
                         np.r_[4.0 + rng.random(n), 0.8 * rng.standard_normal(3 * n)])
    b = rng.standard_normal(n)
    want = gr.gmres(S, n, b, np.zeros(n), 0.0, 256, 256, kr.JACOBI)
    assert (want["iterations"], want["cycles"]) == (256, 1)
    keep = []
    got, _ = _run(ctx, _coo(S, (n, n), 0, device=True, keep=keep), b, np.zeros(n), kr.JACOBI, tol=0.0, max_iter=256, restart=256,
                  device=True)
    _same_all(got, want, "restart 256")


def test_restart_one(ctx):
    """Every step is a cycle: GMRES(1) on convection-diffusion 12^2 converges slowly but does, each step on the true residual."""
    S, n = br.convdiff2d(12)
    b = np.random.default_rng(2740).standard_normal(n)
    want = gr.gmres(S, n, b, np.zeros(n), 1e-2, 40, 1, kr.JACOBI)
    assert want["cycles"] == want["iterations"] > 3
    keep = []
    a = _coo(S, (n, n), 0, keep=keep)
    for path in (0, 1):
        with Knobs(ctx, {"gmres_path": path}):
            got, _ = _run(ctx, a, b, np.zeros(n), kr.JACOBI, tol=1e-2, max_iter=40, restart=1)
        _same_all(got, want, "restart 1 path %d" % path)


# ---------------------------------------------------------------- a cycle that ends early, and the loop goes on

# (A, b, restart, tol, max_iter, the steps of each cycle): a cycle ends on the estimate -- or with the Krylov space whole,
# restart > n -- while the true residual is still above the threshold, so k falls behind the steps the host has enqueued
CONTINUED = (
    ([[0, 0, 1], [0, 1, -1], [-1, 3, 3]], [1, 2, 3], 5, 1e-15, 5, [3, 1]),        # CONVERGED at k = 4 < max_iter, restart > n
    ([[0, 0, 1], [0, 1, -1], [-1, 3, 3]], [1, 2, 3], 5, 1e-15, 12, [3, 1]),
    ([[-1, -3, 2], [-1, 0, -1], [-2, 1, -1]], [-3, 3, 1], 6, 1e-16, 6, [3, 3]),  # MAXITER, restart > n
    ([[-1, 2, -1], [1, 2, 2], [-3, 3, 2]], [1, -2, 3], 3, 1e-16, 6, [3, 2, 1]),  # MAXITER in mid-cycle after a short cycle
)


@pytest.mark.parametrize("case", range(len(CONTINUED)))
def test_a_cycle_ends_early_and_the_loop_goes_on(ctx, case):
    """The cycles are sized from the k that was read, min(restart, max_iter - k): after a short cycle the host neither enqueues
    past max_iter nor waits on an empty batch, and every cycle still ends within its steps.  The bits and the cycle count of
    the reference on both paths, host and device vectors."""
    rows, b, restart, tol, max_iter, steps = CONTINUED[case]
    A = np.array(rows, np.float64)
    i, j = np.nonzero(A)
    D = (i.astype(np.int32), j.astype(np.int32), A[i, j])
    n = A.shape[0]
    b = np.array(b, np.float64)
    want = gr.gmres(D, n, b, np.zeros(n), tol, max_iter, restart)
    assert want["cycle_steps"] == steps and any(c < restart for c in steps[:-1])
    keep = []
    for path in (0, 1):
        for device in (False, True):
            with Knobs(ctx, {"gmres_path": path}):
                got, _ = _run(ctx, _coo(D, (n, n), 0, keep=keep), b, np.zeros(n), tol=tol, max_iter=max_iter, restart=restart, device=device)
            _same_all(got, want, "case %d path %d device %d" % (case, path, device))


# ---------------------------------------------------------------- the reason this loop exists

def test_convection_diffusion_128(ctx):
    """Upwind convection-diffusion 128^2, b = A 1, tol = 1e-8, no preconditioner: GMRES(30) takes the steps and cycles of the
    host reference (tests/test_gmres_host.py) and its x has a true relative residual, through multiply_dense and plain
    numpy, of at most tol (1 + 1e-9); spsamd_solve_bicgstab on the same operands reports CONVERGED on a true residual
    above 100 tol."""
    from tests.test_gmres_host import COUNTS
    S, n = br.convdiff2d(128)
    b = kr.apply(S, n, np.ones(n))
    tol = 1e-8
    keep = []
    a = _coo(S, (n, n), 0, keep=keep)

    def true_rel(x):
        ax = np.zeros(n)
        ctx.multiply_dense(a, x, ax)
        return np.linalg.norm(b - ax) / np.linalg.norm(b)

    got, st = _run(ctx, a, b, np.zeros(n), tol=tol, max_iter=10000, restart=30)
    assert (got["iterations"], got["cycles"], got["reason"]) == COUNTS[128] + (kr.CONVERGED,)
    assert max(got["hist"]) <= got["rr0"] and got["hist"][-1] == got["rr"] <= tol * tol * got["bb"]
    assert true_rel(got["x"]) <= tol * (1 + 1e-9)
    _, _, sb = ctx.solve_bicgstab(a, b, xb := np.zeros(n), tol=tol, max_iter=10000)
    assert sb.reason == kr.CONVERGED and true_rel(xb) > 100 * tol


# ---------------------------------------------------------------- what a call enqueues and allocates

def _launches(path, precond, restart, max_iter, cycles):
    """The launches of `cycles` enqueued cycles on an operand without long rows, every cycle but the last one whole: cycle c
    then begins at k = c restart and enqueues min(restart, max_iter - c restart) steps and one cycle end.  A step at position s: the preconditioner (Jacobi: 1), the SpMV, then on path 0 two
    projections, two folds, two subtractions, on path 1 2 (s + 1) times a dot, a fold and a subtraction and the dot of ww;
    the Hessenberg kernel and the scale.  A cycle end: the back substitution, the combination, under Jacobi the division
    and x += z, the SpMV, the residual (on path 1 with a dot of its own), the finish and the scale."""
    pre = 1 if precond == kr.JACOBI else 0
    total = 0
    for c in range(cycles):
        for s in range(min(restart, max_iter - c * restart)):
            total += pre + 1 + (6 if path == 0 else 6 * (s + 1) + 1) + 2
        total += 2 + 2 * pre + 1 + 1 + path + 2
    return total


def test_launches_and_workspace(ctx):
    """launches is what the enqueued cycles account for, the steps behind an in-cycle end included; nothing is allocated per
    step: the workspace of max_iter 2 is that of 400 at a fixed restart."""
    from spsparse_amd import capi
    S, n = br.convdiff2d(24)
    b = kr.apply(S, n, np.ones(n))
    keep = []
    a = _coo(S, (n, n), 0, device=True, keep=keep)
    for precond in (kr.NONE, kr.JACOBI):
        for path in (0, 1):
            for tol, max_iter, restart in ((1e-8, 40, 7), (1e-3, 500, 30)):   # cut by max_iter in mid-cycle | ended by the estimate
                with Knobs(ctx, {"gmres_path": path}):
                    got, st = _run(ctx, a, b, np.zeros(n), precond, tol=tol, max_iter=max_iter, restart=restart, device=True)
                assert got["iterations"] % restart, (precond, path, tol)
                assert got["reason"] == (kr.MAXITER if max_iter == 40 else kr.CONVERGED)
                assert st.launches == _launches(path, precond, restart, max_iter, got["cycles"]), (precond, path, tol, st.launches)
    used = {}
    for path in (0, 1):
        for max_iter in (2, 400):
            res = capi.Result()
            with Knobs(ctx, {"gmres_path": path}):
                _, stw = _run(ctx, a, b, np.zeros(n), kr.JACOBI, tol=0.0, max_iter=max_iter, restart=20, device=True, cap=1, result=res)
            assert stw.iterations == max_iter or stw.reason != kr.MAXITER
            used[(path, max_iter)] = int(res.workspace_bytes)
        assert used[(path, 2)] == used[(path, 400)] > 0, used


def test_a_prepared_factor_is_analysed_once(ctx):
    """PRECOND_LU on convection-diffusion 24^2 with M a prepared handle: two analyses on the first call (the handle grows),
    none on the second; the bits of the reference both times."""
    from spsparse_amd import capi
    S, n = br.convdiff2d(24)
    b = np.random.default_rng(2750).standard_normal(n)
    keep = []
    a = _coo(S, (n, n), 0, keep=keep)
    f = ctx.fetch(ctx.factor_ilu0(a))
    F = (f[0].copy(), f[1].copy(), f[2].copy())
    want = gr.gmres(S, n, b, np.zeros(n), 1e-8, 100, 10, kr.LU, F)
    assert want["reason"] == kr.CONVERGED and want["cycles"] >= 2
    h = capi.Operand(ctx, _coo(F, (n, n), 0, keep=keep), '.', capi.AS_A)
    try:
        b0 = h.bytes
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tol=1e-8, max_iter=100, restart=10)
        _same_all(got, want, "prepared F, first call")
        b1 = h.bytes
        assert st.analyses == 2 and b1 > b0
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tol=1e-8, max_iter=100, restart=10, device=True)
        _same_all(got, want, "prepared F, second call")
        assert st.analyses == 0 and h.bytes == b1
    finally:
        h.close()


# ---------------------------------------------------------------- errors and trivia

def _raw(ctx, a, b, x, mem, precond=0, m=None, tol=1e-8, max_iter=10, restart=5, pol=ar.ADD):
    return ctx.L.spsamd_solve_gmres(ctx.h, C.byref(a), b'.', precond, None if m is None else C.byref(m), b'.', b, x, mem, tol,
                                    max_iter, restart, None, 0, pol, 0, None, None)


def test_errors_leave_x(ctx):
    from spsparse_amd import capi
    S, n = br.convdiff2d(4)
    keep = []
    a, wide = _coo(S, (n, n), 0, keep=keep), _coo(S, (n, n + 1), 0, keep=keep)
    b, x = np.ones(n), np.full(n, SENT)
    pb, px = b.ctypes.data, x.ctypes.data
    bad = [dict(restart=0), dict(restart=257), dict(tol=-1e-8), dict(tol=float("nan")), dict(m=a), dict(precond=kr.LU),
           dict(precond=3), dict(mem=2), dict(pol=3)]
    for kw in bad:
        mem = kw.pop("mem", capi.MEM_HOST)
        assert _raw(ctx, a, pb, px, mem, **kw) == -2, kw
    assert _raw(ctx, wide, pb, px, capi.MEM_HOST) == -1
    assert _raw(ctx, a, pb, pb, capi.MEM_HOST) == -2                     # x aliasing b
    assert _raw(ctx, a, pb, None, capi.MEM_HOST) == -2
    assert np.all(x == SENT) and np.all(b == 1.0)
    got, _ = _run(ctx, a, b, np.zeros(n), restart=256)                   # ... and the context still works, at the largest restart
    _same_all(got, gr.gmres(S, n, b, np.zeros(n), 1e-8, 100, 256), "after the refusals")


def test_trivia(ctx):
    keep = []
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    got, st = _run(ctx, _coo(E, (0, 0), -1, keep=keep), np.zeros(0), np.zeros(0))
    assert (got["iterations"], got["reason"], list(got["hist"])) == (0, kr.CONVERGED, [0.0])
    assert (st.bb, st.rr0, st.rr, st.launches) == (0.0, 0.0, 0.0, 0)
    # the hand cases of the host test
    x0 = np.array([0.5, -0.25])
    cases = (([[0, 1], [2, 1]], [2.0, 0.0], 10, 2, 0.0), ([[0, 1], [2, 1]], [2.0, 0.0], 1, 2, 0.0), ([[0, 1], [2, 1]], [2.0, 0.0], 5, 1, 0.0),
             ([[1, 1], [0, 0]], [1.0, 1.0], 10, 2, 1e-10), ([[1e200, 0], [0, 1e200]], [1.0, 1.0], 10, 2, 1e-6),
             ([[0, 1], [2, 1]], [np.nan, 1.0], 10, 2, 1e-6), ([[0, 1], [2, 1]], [0.0, 0.0], 10, 2, 1e-6))
    for rows, b, max_iter, restart, tol in cases:
        A = np.array(rows, np.float64)
        i, j = np.nonzero(A)
        D = (i.astype(np.int32), j.astype(np.int32), A[i, j])
        for path in (0, 1):
            with Knobs(ctx, {"gmres_path": path}):
                got, _ = _run(ctx, _coo(D, (2, 2), 0, keep=keep), np.array(b), np.zeros(2), tol=tol, max_iter=max_iter, restart=restart)
            _same_all(got, gr.gmres(D, 2, np.array(b), np.zeros(2), tol, max_iter, restart),
                      "hand case %r max %d restart %d path %d" % (rows, max_iter, restart, path))
    # an empty A: BREAKDOWN before the first step, x untouched
    got, _ = _run(ctx, _coo(E, (2, 2), -1, keep=keep), np.array([1.0, 1.0]), x0, tol=1e-6, max_iter=10, restart=3)
    _same_all(got, gr.gmres(E, 2, np.array([1.0, 1.0]), x0, 1e-6, 10, 3), "empty A")
    assert (got["iterations"], got["reason"], list(got["x"])) == (0, kr.BREAKDOWN, list(x0))
    # the cyclic shift of order 6: stagnation under m = 2, the exact solution at step 6 under m = 6
    n = 6
    i = np.arange(n, dtype=np.int32)
    S = fr.sorted_unique(((i + 1) % n).astype(np.int32), i, np.ones(n))
    b = np.zeros(n)
    b[0] = 1.0
    for restart, path in ((2, 0), (2, 1), (6, 0), (6, 1)):
        with Knobs(ctx, {"gmres_path": path}):
            got, _ = _run(ctx, _coo(S, (n, n), 0, keep=keep), b, np.zeros(n), max_iter=8, restart=restart)
        _same_all(got, gr.gmres(S, n, b, np.zeros(n), 1e-8, 8, restart), "shift, restart %d path %d" % (restart, path))
    assert (got["iterations"], got["reason"], list(got["hist"])) == (6, kr.CONVERGED, [1.0] * 6 + [0.0])
    # the history's capacity
    S, n = br.convdiff2d(6)
    b = np.arange(1.0, n + 1)
    want = gr.gmres(S, n, b, np.zeros(n), 1e-8, 100, 8)
    k = want["iterations"]
    assert want["reason"] == kr.CONVERGED and k > 8
    a = _coo(S, (n, n), 0, keep=keep)
    for cap in (0, 1, 3, k + 1, k + 10):
        for device in (False, True):
            got, _ = _run(ctx, a, b, np.zeros(n), restart=8, cap=cap, device=device)
            _same_all(got, want, "cap %d" % cap, hist=False)
            assert np.array_equal(got["hist"].view(np.int64), want["hist"][:cap].view(np.int64)), cap
    # hist_host NULL with a capacity, stats and result NULL
    x = np.zeros(n)
    rc = ctx.L.spsamd_solve_gmres(ctx.h, C.byref(a), b'.', 0, None, b'.', b.ctypes.data, x.ctypes.data, 0, 1e-8, 100, 8, None, 5,
                                  ar.ADD, 0, None, None)
    assert rc == 0 and np.array_equal(x.view(np.int64), want["x"].view(np.int64))
