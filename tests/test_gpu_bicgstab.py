"""spsamd_solve_bicgstab on the device against tests/bicgstab_ref.py (pinned on the host by tests/test_bicgstab_host.py): x,
the history, the iteration count, the stop reason, bb, rr0 and rr, every float as an int64 bit pattern with zero tolerance --
each is defined by the loop of the header, reduction shape included, so there is nothing to tolerate.  The pcg_fuse and
pcg_check_every knobs run so that both launch shapes and several batch lengths meet one definition.  The operand makers and
the comparison are those of tests/test_gpu_krylov.py."""
import ctypes as C

import numpy as np
import pytest

from tests import add_ref as ar
from tests import bicgstab_ref as br
from tests import factor_ref as fr
from tests import krylov_ref as kr
from tests import select_ref as sel
from tests.gpu_util import Knobs, coo as _coo, ctx  # noqa: F401
from tests.test_gpu_krylov import EDGES, KINDS, SENT, _matrix, _mixed, _operand, _same, _stored

pytestmark = pytest.mark.gpu


def _run(ctx, a, b, x0, precond=kr.NONE, m=None, tA='.', tM='.', tol=1e-8, max_iter=100, pol=ar.ADD, zn=False, device=False,
         cap=None, result=None):
    """One call; b is checked untouched.  Returns (the dict bicgstab_ref.bicgstab returns, without `half`; PcgStats)."""
    b = np.ascontiguousarray(b, np.float64)
    if device:
        import torch
        tb, tx = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(np.array(x0, np.float64)).cuda()
        torch.cuda.synchronize()
        _, hist, st = ctx.solve_bicgstab(a, tb, tx, precond, m, tA, tM, tol, max_iter, cap, pol, zn, result)
        gx, gb = tx.cpu().numpy(), tb.cpu().numpy()
    else:
        gb, gx = b.copy(), np.array(x0, np.float64)
        _, hist, st = ctx.solve_bicgstab(a, gb, gx, precond, m, tA, tM, tol, max_iter, cap, pol, zn, result)
    assert np.array_equal(gb.view(np.int64), b.view(np.int64)), "b was written"
    got = {"x": gx, "hist": hist, "iterations": int(st.iterations), "reason": int(st.reason),
           "bb": np.float64(st.bb), "rr0": np.float64(st.rr0), "rr": np.float64(st.rr)}
    return got, st


# ---------------------------------------------------------------- the semantic fuzz

def test_semantic_fuzz(ctx):
    """150 operands of order 1 .. 40.  The kind is the trial's base-5 digit; the digits above it run through the 18
    (precond, pcg_fuse, pcg_check_every) settings and, on other periods, through the transposes, the memory of the vectors
    and the four operand forms, so every kind meets every value of every setting; the coverage is asserted, the three
    reasons and both ways to CONVERGED (the loop's top and the half step) included."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2610)
    seen, ends = set(), set()
    for trial in range(150):
        kind, j = trial % 5, trial // 5
        precond, fuse, every = j % 3, (j // 3) % 2, (0, 1, 3)[(j // 6) % 3]
        tA, tM = '.T'[j % 2], '.T'[(j // 3) % 2]
        device, form_a, form_m = bool((j // 2) % 2), (j + j // 4) % 4, (j // 3 + j // 12) % 4
        n = int(rng.integers(1, 41))
        pol, zn = int(rng.integers(3)), bool(rng.integers(5) == 0)
        tol = (0.0, 1e-6, 1e-2)[int(rng.integers(3))]
        max_iter = (0, 1, 3, 25)[int(rng.integers(4))] if kind > 1 else 60
        keep, handles = [], []
        what = "trial %d n %d %s precond %d fuse %d every %d %s %s dev %d forms %d %d pol %d zn %d tol %g max %d" % (
            trial, n, KINDS[kind], precond, fuse, every, tA, tM, device, form_a, form_m, pol, zn, tol, max_iter)
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
            want = br.bicgstab(S, n, b, x0, tol, max_iter, precond, F)
            with Knobs(ctx, {"pcg_fuse": fuse, "pcg_check_every": every}):
                got, st = _run(ctx, a, b, x0, precond, m, tA, tM, tol, max_iter, pol, zn, device)
            _same(got, want, what)
            assert st.analyses == (0 if precond != kr.LU else 2), what        # (no handle here was solved with before)
            if precond == kr.LU and form_m == 3:                               # ... and now M's handle has both schedules
                before = handles[-1].bytes
                with Knobs(ctx, {"pcg_fuse": fuse, "pcg_check_every": every}):
                    again, st2 = _run(ctx, a, b, x0, precond, m, tA, tM, tol, max_iter, pol, zn, device)
                _same(again, want, what + " again")
                assert st2.analyses == 0 and handles[-1].bytes == before, what
            assert st.readbacks <= st.iterations // (every or capi.pcg_check_every) + 2, what
        finally:
            for h in handles:
                h.close()
        ends.add((want["reason"], want["half"], want["iterations"] > 0))
        seen.add(("set", kind, precond, fuse, every)); seen.add(("tA", kind, tA)); seen.add(("dev", kind, device))
        seen.add(("fa", kind, form_a))
        if precond == kr.LU:
            seen.add(("tM", kind, tM)); seen.add(("fm", kind, form_m))
    count = lambda tag: len([s for s in seen if s[0] == tag])
    assert count("set") == 5 * 18 and count("tA") == 10 and count("dev") == 10 and count("fa") == 20
    assert count("tM") == 10 and count("fm") == 20
    assert {e[0] for e in ends} == {kr.CONVERGED, kr.MAXITER, kr.BREAKDOWN}
    # CONVERGED at the half step, and at the loop's top after whole iterations
    assert (kr.CONVERGED, True, True) in ends and (kr.CONVERGED, False, True) in ends, ends


# ---------------------------------------------------------------- the folds at their edges

@pytest.mark.parametrize("n", EDGES)
def test_fold_edges(ctx, n):
    """An empty A, x0 = 0, max_iter = 0: bb and rr0 are dot(b, b), b of mixed magnitudes so that the order shows.  Then an
    upper bidiagonal A and two iterations, plain and Jacobi, fused and not: the two SpMVs with one and two folds, the half
    step, the update with two folds, the Jacobi division and the direction meet the same chunk edges, and the finish kernel
    folds one, two and three levels twice over."""
    rng = np.random.default_rng(2620 + n % 1000)
    b = _mixed(rng, n)
    keep = []
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    want = br.bicgstab(E, n, b, np.zeros(n), 1e-8, 0)
    for fuse in (0, 1):
        with Knobs(ctx, {"pcg_fuse": fuse}):
            got, _ = _run(ctx, _coo(E, (n, n), -1, keep=keep), b, np.zeros(n), max_iter=0, device=bool(fuse))
        _same(got, want, "empty A, n %d fuse %d" % (n, fuse))
    d = np.arange(n, dtype=np.int32)
    D = fr.sorted_unique(np.r_[d, d[:-1]], np.r_[d, d[1:]], np.r_[1.0 + rng.random(n), 0.25 * rng.random(n - 1)])
    x0 = rng.standard_normal(n)
    a = _coo(D, (n, n), 0, device=True, keep=keep)
    for precond in (kr.NONE, kr.JACOBI):
        want = br.bicgstab(D, n, b, x0, 0.0, 2, precond)
        assert want["iterations"] == 2 or n == 1
        for fuse in (0, 1):
            with Knobs(ctx, {"pcg_fuse": fuse}):
                got, _ = _run(ctx, a, b, x0, precond, tol=0.0, max_iter=2, device=True)
            _same(got, want, "bidiagonal A, n %d precond %d fuse %d" % (n, precond, fuse))


# ---------------------------------------------------------------- long rows

def test_long_rows(ctx):
    """An unsymmetric arrow of order 3000: row 0 and column 0 full, with different weights.  Row 0 is far above
    spmm_long_min, so both SpMVs go through the wave kernel of k_spmm.hip and the partials of chunk 0 -- of both arrays
    behind the second SpMV -- are redone.  The same bits with every row serial (spmm_path 1)."""
    from spsparse_amd import capi
    n = 3000
    rng = np.random.default_rng(2630)
    i = np.arange(1, n)
    D = fr.sorted_unique(np.r_[np.arange(n), np.zeros(n - 1, int), i], np.r_[np.arange(n), i, np.zeros(n - 1, int)],
                         np.r_[float(n), 2.0 + rng.random(n - 1), 0.5 * rng.random(n - 1), -0.3 * rng.random(n - 1)])
    b = _mixed(rng, n)
    keep = []
    for precond in (kr.NONE, kr.JACOBI):
        want = br.bicgstab(D, n, b, np.zeros(n), 1e-10, 12, precond)
        assert want["iterations"] >= 2
        for fuse, form in ((0, 0), (1, 0), (0, 3)):
            handles = []
            try:
                a, _ = _operand(ctx, D, n, '.', form, ar.ADD, False, keep, handles)
                with Knobs(ctx, {"pcg_fuse": fuse}):
                    got, st = _run(ctx, a, b, np.zeros(n), precond, tol=1e-10, max_iter=12, device=True)
            finally:
                for h in handles:
                    h.close()
            _same(got, want, "arrow precond %d fuse %d form %d" % (precond, fuse, form))
    with Knobs(ctx, {"spmm_path": 1}):
        got, st1 = _run(ctx, _coo(D, (n, n), 0, keep=keep), b, np.zeros(n), kr.JACOBI, tol=1e-10, max_iter=12)
    _same(got, want, "arrow, serial rows")
    assert st1.launches < st.launches
    assert capi.pcg_chunk == kr.CHUNK
    # nothing is allocated per iteration: the workspace of 2 iterations is that of 400 (tol = 0: none of them is spared)
    used = {}
    for fuse in (0, 1):
        for max_iter in (2, 400):
            res = capi.Result()
            with Knobs(ctx, {"pcg_fuse": fuse}):
                _, stw = _run(ctx, _coo(D, (n, n), 0, keep=keep), b, np.zeros(n), kr.JACOBI, tol=0.0, max_iter=max_iter, device=True,
                              cap=1, result=res)
            assert stw.iterations == max_iter or stw.reason != kr.MAXITER
            used[(fuse, max_iter)] = int(res.workspace_bytes)
        assert used[(fuse, 2)] == used[(fuse, 400)] > 0, used


def test_long_rows_in_three_chunks(ctx):
    """Long rows in the first, a middle and the last chunk of 5000 rows, and a short last chunk, the rows and their columns
    weighted differently: the fused SpMVs serve the short rows, the wave kernel the long ones, and the partials of their
    chunks alone are redone -- the bits of the reference and of the serial rows, and fewer launches than with every dot a
    launch of its own.  Then so many long rows (spmm_long_min 1) that the whole dots run instead."""
    n = 5000
    rng = np.random.default_rng(2631)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [40.0 + rng.random(n)]
    for r, m in ((3, 70), (2500, 300), (n - 1, 65)):
        c = rng.choice(n, m, replace=False)
        c = c[c != r]
        rows += [np.full(c.size, r), c]; cols += [c, np.full(c.size, r)]
        vals += [0.05 * rng.standard_normal(c.size), 0.08 * rng.standard_normal(c.size)]
    D = fr.sorted_unique(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))
    b = _mixed(rng, n)
    keep = []
    a = _coo(D, (n, n), 0, device=True, keep=keep)
    want = br.bicgstab(D, n, b, np.zeros(n), 1e-12, 6)
    assert want["iterations"] >= 3
    got, st0 = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=6, device=True)
    _same(got, want, "three long rows, fused")
    with Knobs(ctx, {"pcg_fuse": 1}):
        got, st1 = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=6, device=True)
    _same(got, want, "three long rows, unfused")
    assert st0.launches < st1.launches
    with Knobs(ctx, {"spmm_path": 1}):
        got, st2 = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=6, device=True)
    _same(got, want, "three long rows, serial")
    assert st2.launches < st0.launches
    with Knobs(ctx, {"spmm_long_min": 1}):
        got, _ = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=6, device=True)
    _same(got, want, "every coupled row long")


# ---------------------------------------------------------------- the batch never shows

def _stops(S, n, b, half):
    """A tolerance at which convection-diffusion stops CONVERGED, by the half-step exit or not, at an iteration count that
    is no multiple of 2, 7 or 64: (tol, the reference's outcome)."""
    for tol in (1e-8, 1e-7, 1e-9, 1e-6, 1e-10, 1e-5, 1e-11, 1e-4, 1e-12, 1e-3):
        w = br.bicgstab(S, n, b, np.zeros(n), tol, 500)
        if w["reason"] == kr.CONVERGED and w["half"] == half and all(w["iterations"] % d for d in (2, 7, 64)):
            return tol, w
    raise AssertionError("no such stop")


@pytest.mark.parametrize("half", [False, True])
def test_the_batch_never_shows(ctx, half):
    """Convection-diffusion 24^2 stopped in the middle of a batch, at the loop's top and by the half-step exit, under
    pcg_check_every 1, 2, 7, 64: the same bits, at most iterations / every + 2 reads of the state, and
    launches = launches per iteration x iterations enqueued."""
    S, n = br.convdiff2d(24)
    b = np.random.default_rng(2640).standard_normal(n)
    tol, want = _stops(S, n, b, half)
    keep = []
    a = _coo(S, (n, n), 0, device=True, keep=keep)
    launches = {}
    for every in (1, 2, 7, 64):
        with Knobs(ctx, {"pcg_check_every": every}):
            got, st = _run(ctx, a, b, np.zeros(n), tol=tol, max_iter=500, device=True)
        _same(got, want, "every %d" % every)
        assert st.readbacks <= st.iterations // every + 2, (every, st.readbacks)
        launches[every] = st.launches
    k = want["iterations"]
    per = launches[1] // k
    assert launches[1] == per * k                                        # a batch of one: nothing is enqueued after the stop
    assert [launches[e] for e in (2, 7, 64)] == [per * ((k + e - 1) // e) * e for e in (2, 7, 64)]


# ---------------------------------------------------------------- schedules are built once

def test_schedules(ctx):
    """PRECOND_LU on convection-diffusion 24^2.  A raw F: two analyses whatever the iteration count.  A prepared F: two on
    the first call (the handle grows), none on the second, and the handle then serves spsamd_solve_pcg and spsamd_solve_tri
    without another analysis."""
    from spsparse_amd import capi
    S, n = br.convdiff2d(24)
    b = np.random.default_rng(2650).standard_normal(n)
    keep = []
    a = _coo(S, (n, n), 0, keep=keep)
    f = ctx.fetch(ctx.factor_ilu0(a))
    F = (f[0].copy(), f[1].copy(), f[2].copy())
    want = br.bicgstab(S, n, b, np.zeros(n), 1e-8, 100, kr.LU, F)
    assert want["reason"] == kr.CONVERGED
    for max_iter in (1, 100):
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, _coo(F, (n, n), -1, keep=keep), tol=1e-8, max_iter=max_iter, device=True)
        assert st.analyses == 2, max_iter
    _same(got, want, "raw F")
    h = capi.Operand(ctx, _coo(F, (n, n), 0, keep=keep), '.', capi.AS_A)
    try:
        b0 = h.bytes
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tol=1e-8, max_iter=100)
        _same(got, want, "prepared F, first call")
        b1 = h.bytes
        assert st.analyses == 2 and b1 > b0
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tol=1e-8, max_iter=100, device=True)
        _same(got, want, "prepared F, second call")
        assert st.analyses == 0 and h.bytes == b1
        _, _, sp = ctx.solve_pcg(a, b, None, kr.LU, h.coo, tol=1e-8, max_iter=3)
        assert sp.analyses == 0 and h.bytes == b1
        y, s1 = ctx.solve_tri(h.coo, b, capi.TRI_LOWER, capi.DIAG_UNIT, stats=True)
        _, s2 = ctx.solve_tri(h.coo, y, capi.TRI_UPPER, capi.DIAG_NONUNIT, stats=True)
        assert (s1.analysis_reused, s2.analysis_reused) == (1, 1) and h.bytes == b1
    finally:
        h.close()


# ---------------------------------------------------------------- errors and trivia

def _raw(ctx, a, b, x, mem, precond=0, m=None, tol=1e-8, max_iter=10, pol=ar.ADD):
    return ctx.L.spsamd_solve_bicgstab(ctx.h, C.byref(a), b'.', precond, None if m is None else C.byref(m), b'.', b, x, mem, tol,
                                       max_iter, None, 0, pol, 0, None, None)


def test_errors_leave_x(ctx):
    from spsparse_amd import capi
    S, n = br.convdiff2d(4)
    keep = []
    a, wide = _coo(S, (n, n), 0, keep=keep), _coo(S, (n, n + 1), 0, keep=keep)
    S5, n5 = br.convdiff2d(5)
    other = _coo(S5, (n5, n5), 0, keep=keep)
    b, x = np.ones(n), np.full(n, SENT)
    pb, px = b.ctypes.data, x.ctypes.data
    bad = [dict(tol=-1e-8), dict(tol=float("nan")), dict(tol=float("inf")), dict(m=a), dict(precond=kr.LU), dict(precond=3),
           dict(precond=-1), dict(mem=2), dict(mem=-1), dict(pol=3)]
    for kw in bad:
        mem = kw.pop("mem", capi.MEM_HOST)
        assert _raw(ctx, a, pb, px, mem, **kw) == -2, kw
    assert _raw(ctx, wide, pb, px, capi.MEM_HOST) == -1
    assert _raw(ctx, a, pb, px, capi.MEM_HOST, kr.LU, other) == -1
    assert _raw(ctx, a, pb, pb, capi.MEM_HOST) == -2                     # x aliasing b
    assert _raw(ctx, a, pb, pb + 8, capi.MEM_HOST) == -2                 # ... or overlapping it
    assert _raw(ctx, a, pb, None, capi.MEM_HOST) == -2
    assert _raw(ctx, a, pb, a.val, capi.MEM_HOST) == -2                  # x over A's values
    assert ctx.L.spsamd_solve_bicgstab(ctx.h, None, b'.', 0, None, b'.', pb, px, capi.MEM_HOST, 1e-8, 10, None, 0, ar.ADD, 0,
                                       None, None) == -2                 # A NULL
    oob = _coo((np.array([0, n], np.int32), np.array([0, 0], np.int32), np.ones(2)), (n, n), -1, keep=keep)
    assert _raw(ctx, oob, pb, px, capi.MEM_HOST) == -2
    unsorted = _coo((S[0][::-1].copy(), S[1][::-1].copy(), S[2][::-1].copy()), (n, n), 0, keep=keep)   # a false sort0
    assert _raw(ctx, unsorted, pb, px, capi.MEM_HOST) == -2
    assert np.all(x == SENT) and np.all(b == 1.0)
    res = ctx.consolidate(a, 0)                                          # a device x inside an output set
    assert _raw(ctx, a, res.val, res.val + 8 * n, capi.MEM_DEVICE) == -2
    got, _ = _run(ctx, a, b, np.zeros(n))                                # ... and the context still works
    _same(got, br.bicgstab(S, n, b, np.zeros(n), 1e-8, 100), "after the refusals")


def test_trivia(ctx):
    keep = []
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    got, st = _run(ctx, _coo(E, (0, 0), -1, keep=keep), np.zeros(0), np.zeros(0))
    assert (got["iterations"], got["reason"], list(got["hist"])) == (0, kr.CONVERGED, [0.0])
    assert (st.bb, st.rr0, st.rr, st.launches) == (0.0, 0.0, 0.0, 0)
    # the hand cases of the host test: the half-step exit at k = 1, the same stopped by max_iter, the breakdown of omega
    for rows, b, max_iter in (([[-2, -2], [-1, -2]], [-2.0, 0.0], 10), ([[-2, -2], [-1, -2]], [-2.0, 0.0], 1),
                              ([[0, 1], [0, 0]], [2.0 ** 30, 1.0], 10), ([[1, 1], [0, 0]], [1.0, 1.0], 10)):
        A = np.array(rows, np.float64)
        i, j = np.nonzero(A)
        D = (i.astype(np.int32), j.astype(np.int32), A[i, j])
        for fuse in (0, 1):
            with Knobs(ctx, {"pcg_fuse": fuse}):
                got, _ = _run(ctx, _coo(D, (2, 2), 0, keep=keep), np.array(b), np.zeros(2), tol=0.0, max_iter=max_iter)
            _same(got, br.bicgstab(D, 2, np.array(b), np.zeros(2), 0.0, max_iter), "hand case %r max %d fuse %d" % (rows, max_iter, fuse))
    S, n = br.convdiff2d(6)
    b = np.arange(1.0, n + 1)
    want = br.bicgstab(S, n, b, np.zeros(n), 1e-8, 100)
    k = want["iterations"]
    assert want["reason"] == kr.CONVERGED and k > 3
    a = _coo(S, (n, n), 0, keep=keep)
    for cap in (0, 1, 3, k + 1, k + 10):
        for device in (False, True):
            got, _ = _run(ctx, a, b, np.zeros(n), cap=cap, device=device)
            _same(got, want, "cap %d" % cap, hist=False)
            assert np.array_equal(got["hist"].view(np.int64), want["hist"][:cap].view(np.int64)), cap
    # hist_host NULL with a capacity, stats and result NULL
    x = np.zeros(n)
    rc = ctx.L.spsamd_solve_bicgstab(ctx.h, C.byref(a), b'.', 0, None, b'.', b.ctypes.data, x.ctypes.data, 0, 1e-8, 100, None, 5,
                                     ar.ADD, 0, None, None)
    assert rc == 0 and np.array_equal(x.view(np.int64), want["x"].view(np.int64))
