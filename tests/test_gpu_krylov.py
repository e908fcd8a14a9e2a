"""spsamd_solve_pcg on the device against tests/krylov_ref.py (pinned on the host by tests/test_krylov_host.py): x, the
history, the iteration count, the stop reason, bb, rr0 and rr, every float as an int64 bit pattern with zero tolerance --
each is defined by the loop of the header, reduction shape included, so there is nothing to tolerate.  The pcg_fuse and
pcg_check_every knobs run so that both launch shapes and several batch lengths meet one definition."""
import ctypes as C

import numpy as np
import pytest

from tests import add_ref as ar
from tests import factor_ref as fr
from tests import krylov_ref as kr
from tests import select_ref as sel
from tests.gpu_util import Knobs, coo as _coo, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = -7.5


def _run(ctx, a, b, x0, precond=kr.NONE, m=None, tA='.', tM='.', tol=1e-8, max_iter=100, pol=ar.ADD, zn=False, device=False,
         cap=None):
    """One call; b is checked untouched.  Returns (the dict krylov_ref.pcg returns, PcgStats)."""
    b = np.ascontiguousarray(b, np.float64)
    if device:
        import torch
        tb, tx = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(np.array(x0, np.float64)).cuda()
        torch.cuda.synchronize()
        _, hist, st = ctx.solve_pcg(a, tb, tx, precond, m, tA, tM, tol, max_iter, cap, pol, zn)
        gx, gb = tx.cpu().numpy(), tb.cpu().numpy()
    else:
        gb, gx = b.copy(), np.array(x0, np.float64)
        _, hist, st = ctx.solve_pcg(a, gb, gx, precond, m, tA, tM, tol, max_iter, cap, pol, zn)
    assert np.array_equal(gb.view(np.int64), b.view(np.int64)), "b was written"
    got = {"x": gx, "hist": hist, "iterations": int(st.iterations), "reason": int(st.reason),
           "bb": np.float64(st.bb), "rr0": np.float64(st.rr0), "rr": np.float64(st.rr)}
    return got, st


def _same(got, want, what, hist=True):
    assert (got["iterations"], got["reason"]) == (want["iterations"], want["reason"]), "%s: stop (%d, %d), want (%d, %d)" % (
        what, got["iterations"], got["reason"], want["iterations"], want["reason"])
    for key in ("bb", "rr0", "rr", "x") + (("hist",) if hist else ()):
        g, w = np.atleast_1d(np.asarray(got[key], np.float64)), np.atleast_1d(np.asarray(want[key], np.float64))
        assert g.shape == w.shape, "%s: %s has shape %r, want %r" % (what, key, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
        assert bad.size == 0, "%s: %s differs in %d places, first at %d: %r (%#x) vs %r (%#x)" % (
            what, key, bad.size, bad[0], g[bad[0]], g.view(np.uint64)[bad[0]], w[bad[0]], w.view(np.uint64)[bad[0]])


# ---------------------------------------------------------------- the semantic fuzz

KINDS = ("spd", "unsymmetric", "singular", "missing diagonal", "special values")


def _sparse(rng, n, per_row):
    m = max(1, per_row * n)
    return rng.integers(0, n, m), rng.integers(0, n, m), rng.standard_normal(m)


def _matrix(rng, n, kind):
    """op()'s tuples of one fuzz operand, in random order (duplicate keys except for the SPD kinds)."""
    if kind in (0, 2):
        B = np.zeros((n, n))
        i, j, v = _sparse(rng, n, 2)
        B[i, j] = 0.5 * v
        A = B @ B.T + np.eye(n)
        if kind == 2:
            if rng.integers(2) == 0:
                A[:] = 0.0                                             # pq = 0 at once
            else:
                z = int(rng.integers(n))
                A[z, :] = 0.0; A[:, z] = 0.0                           # a zero row and column
        i, j = np.nonzero(A)
        v = A[i, j]
    else:
        i, j, v = _sparse(rng, n, 3)
        v = 0.3 * v
        d = np.arange(n)
        if kind == 3:
            d = d[rng.random(n) < 0.7]
        i, j, v = np.r_[i, d], np.r_[j, d], np.r_[v, 2.0 + rng.random(d.size)]
        if kind == 4:
            pick = rng.random(v.size) < 0.15
            spec = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0])
            v = np.where(pick, spec[rng.integers(0, 5, v.size)], v)
            nan = np.isnan(v)
            v.view(np.uint64)[nan] |= rng.integers(1, 1 << 20, int(nan.sum())).astype(np.uint64)   # quiet NaNs with payloads
    o = rng.permutation(len(v))
    return i[o].astype(np.int32), j[o].astype(np.int32), np.ascontiguousarray(v[o], np.float64)


def _stored(D, t):
    return D if t == '.' else (D[1], D[0], D[2])


def _operand(ctx, D, n, t, form, pol, zn, keep, handles):
    """op()'s tuples D as an operand of one of the four forms: (Coo struct, S)."""
    from spsparse_amd import capi
    X = _stored(D, t)
    lead = 1 if t == 'T' else 0
    if form == 1:                                                      # trusted: rows of op() ascending, stored on the device
        o = np.argsort(X[lead], kind="stable")
        X = tuple(x[o] for x in X)
        return _coo(X, (n, n), lead, device=True, keep=keep), sel.operand_S(X, t, pol, zn, lead)
    if form == 2:                                                      # a SINK_COO result of this context
        res = ctx.consolidate(_coo(X, (n, n), -1, keep=keep), 0, pol, zn)
        return capi.result_operand(res), sel.operand_S(ctx.fetch(res), t, pol, zn, 0)
    if form == 3:                                                      # a prepared handle of the same transpose
        h = capi.Operand(ctx, _coo(X, (n, n), -1, keep=keep), t, capi.AS_A, pol, zn)
        handles.append(h)
        return h.coo, sel.operand_S(X, t, pol, zn, -1)
    return _coo(X, (n, n), -1, keep=keep), sel.operand_S(X, t, pol, zn, -1)


def test_semantic_fuzz(ctx):
    """150 operands of order 1 .. 40.  The kind is the trial's base-5 digit; the digits above it run through the 18
    (precond, pcg_fuse, pcg_check_every) settings and, on other periods, through the transposes, the memory of the vectors
    and the four operand forms, so every kind meets every value of every setting; the coverage is asserted."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2310)
    seen, reasons = set(), set()
    for trial in range(150):
        kind, j = trial % 5, trial // 5
        precond, fuse, every = j % 3, (j // 3) % 2, (0, 1, 3)[(j // 6) % 3]
        tA, tM = '.T'[j % 2], '.T'[(j // 3) % 2]
        device, form_a, form_m = bool((j // 2) % 2), (j + j // 4) % 4, (j // 3 + j // 12) % 4
        n = int(rng.integers(1, 41))
        pol, zn = int(rng.integers(3)), bool(rng.integers(5) == 0)
        tol = (0.0, 1e-6, 1e-2)[int(rng.integers(3))]
        max_iter = (0, 1, 3, 25)[int(rng.integers(4))] if kind else 60
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
                    if kind == 0:                                      # the factor of A itself (its keys sorted: a trusted S is not)
                        Ss = fr.sorted_unique(*S)
                        D = (Ss[0], Ss[1], fr.ilu0_ref(Ss, n)[0])
                    else:
                        D = _matrix(rng, n, 1)
                    m, F = _operand(ctx, D, n, tM, form_m, pol, zn, keep, handles)
            b = rng.standard_normal(n)
            if kind == 4 and rng.integers(3) == 0:
                b[int(rng.integers(n))] = (np.nan, np.inf, -0.0)[int(rng.integers(3))]
            x0 = np.zeros(n) if rng.integers(2) else rng.standard_normal(n)
            want = kr.pcg(S, n, b, x0, tol, max_iter, precond, F)
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
        reasons.add(want["reason"])
        seen.add(("set", kind, precond, fuse, every)); seen.add(("tA", kind, tA)); seen.add(("dev", kind, device))
        seen.add(("fa", kind, form_a))
        if precond == kr.LU:
            seen.add(("tM", kind, tM)); seen.add(("fm", kind, form_m))
    count = lambda tag: len([s for s in seen if s[0] == tag])
    assert count("set") == 5 * 18 and count("tA") == 10 and count("dev") == 10 and count("fa") == 20
    assert count("tM") == 10 and count("fm") == 20
    assert reasons == {kr.CONVERGED, kr.MAXITER, kr.BREAKDOWN}


# ---------------------------------------------------------------- the fold at its edges

EDGES = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1]


def _mixed(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)


@pytest.mark.parametrize("n", EDGES)
def test_fold_edges(ctx, n):
    """An empty A, x0 = 0, max_iter = 0: bb and rr0 are dot(b, b), b of mixed magnitudes so that the order shows.  Then a
    diagonal A and two iterations, plain and Jacobi, fused and not: the fused update, the fused SpMV dot, the Jacobi
    division and p = z + beta p meet the same chunk edges."""
    rng = np.random.default_rng(2320 + n % 1000)
    b = _mixed(rng, n)
    keep = []
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    want = kr.pcg(E, n, b, np.zeros(n), 1e-8, 0)
    for fuse in (0, 1):
        with Knobs(ctx, {"pcg_fuse": fuse}):
            got, _ = _run(ctx, _coo(E, (n, n), -1, keep=keep), b, np.zeros(n), max_iter=0, device=bool(fuse))
        _same(got, want, "empty A, n %d fuse %d" % (n, fuse))
    d = np.arange(n, dtype=np.int32)
    D = (d, d, 1.0 + rng.random(n))
    x0 = rng.standard_normal(n)
    a = _coo(D, (n, n), 0, device=True, keep=keep)
    for precond in (kr.NONE, kr.JACOBI):
        want = kr.pcg(D, n, b, x0, 0.0, 2, precond)
        assert want["iterations"] == 2 or n == 1                         # (order 1: exact after one iteration)
        for fuse in (0, 1):
            with Knobs(ctx, {"pcg_fuse": fuse}):
                got, _ = _run(ctx, a, b, x0, precond, tol=0.0, max_iter=2, device=True)
            _same(got, want, "diagonal A, n %d precond %d fuse %d" % (n, precond, fuse))


# ---------------------------------------------------------------- long rows

def test_long_rows(ctx):
    """An arrow matrix of order 3000: row 0 is far above spmm_long_min, so the SpMV goes through the wave kernels of
    k_spmm.hip and dot(p, q) through the dot kernel alone."""
    from spsparse_amd import capi
    n = 3000
    rng = np.random.default_rng(2330)
    i = np.arange(1, n)
    w = 0.5 * rng.random(n - 1)
    D = fr.sorted_unique(np.r_[np.arange(n), np.zeros(n - 1, int), i], np.r_[np.arange(n), i, np.zeros(n - 1, int)],
                         np.r_[float(n), 2.0 + rng.random(n - 1), w, w])
    b = _mixed(rng, n)
    keep = []
    for precond in (kr.NONE, kr.JACOBI):
        want = kr.pcg(D, n, b, np.zeros(n), 1e-10, 12, precond)
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
    # the same operand with every row serial: the other SpMV, the same bits
    with Knobs(ctx, {"spmm_path": 1}):
        got, st1 = _run(ctx, _coo(D, (n, n), 0, keep=keep), b, np.zeros(n), kr.JACOBI, tol=1e-10, max_iter=12)
    _same(got, want, "arrow, serial rows")
    assert st1.launches < st.launches
    assert capi.pcg_chunk == kr.CHUNK
    # nothing is allocated per iteration: the workspace of 2 iterations is that of 400 (tol = 0: none of them is spared)
    import torch
    used = {}
    for fuse in (0, 1):
        for max_iter in (2, 400):
            res = capi.Result()
            tb, tx = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda")
            with Knobs(ctx, {"pcg_fuse": fuse}):
                _, _, stw = ctx.solve_pcg(_coo(D, (n, n), 0, keep=keep), tb, tx, kr.JACOBI, tol=0.0, max_iter=max_iter,
                                          hist_capacity=1, result=res)
            assert stw.iterations == max_iter or stw.reason != kr.MAXITER
            used[(fuse, max_iter)] = int(res.workspace_bytes)
        assert used[(fuse, 2)] == used[(fuse, 400)] > 0, used


def test_one_long_row_keeps_the_fused_dot(ctx):
    """Long rows in the first, a middle and the last chunk of 5000 rows, and a short last chunk: the fused SpMV serves the
    short rows, the wave kernel the long ones, and the partials of their chunks alone are redone -- the bits of the
    reference, and fewer launches than with every dot a launch of its own.  Then so many long rows (spmm_long_min 1) that
    the whole dot runs instead."""
    n = 5000
    rng = np.random.default_rng(2331)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [40.0 + rng.random(n)]
    for r, m in ((3, 70), (2500, 300), (n - 1, 65)):
        c = rng.choice(n, m, replace=False)
        c = c[c != r]
        rows += [np.full(c.size, r), c]; cols += [c, np.full(c.size, r)]
        w = 0.05 * rng.standard_normal(c.size)
        vals += [w, w]
    D = fr.sorted_unique(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))
    b = _mixed(rng, n)
    keep = []
    a = _coo(D, (n, n), 0, device=True, keep=keep)
    want = kr.pcg(D, n, b, np.zeros(n), 1e-12, 8)
    assert want["iterations"] >= 3
    got, st0 = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=8, device=True)
    _same(got, want, "three long rows, fused")
    with Knobs(ctx, {"pcg_fuse": 1}):
        got, st1 = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=8, device=True)
    _same(got, want, "three long rows, unfused")
    assert st0.launches < st1.launches
    with Knobs(ctx, {"spmm_long_min": 1}):
        got, st2 = _run(ctx, a, b, np.zeros(n), tol=1e-12, max_iter=8, device=True)
    _same(got, want, "every coupled row long")


# ---------------------------------------------------------------- the batch never shows

def test_the_batch_never_shows(ctx):
    """Poisson 24^2 stopped at an iteration count that is no multiple of 2, 7 or 64, under pcg_check_every 1, 2, 7, 64: the
    same bits, at most iterations / every + 2 reads of the state, and launch counts that differ."""
    S, n = kr.poisson2d(24)
    rng = np.random.default_rng(2340)
    b = rng.standard_normal(n)
    want = None
    for tol in (1e-8, 1e-7, 1e-9, 1e-6, 1e-10, 1e-5):
        w = kr.pcg(S, n, b, np.zeros(n), tol, 500)
        if w["reason"] == kr.CONVERGED and all(w["iterations"] % d for d in (2, 7, 64)):
            want = w
            break
    assert want is not None
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

def test_schedules_are_built_once(ctx):
    """PRECOND_LU on Poisson 64^2.  A raw F: two analyses whatever the iteration count.  A prepared F solved with both
    triangles before: none, and the handle does not grow.  The factor of the natural and of the coloured ordering both
    converge, each to the bits of the reference loop."""
    from spsparse_amd import capi
    S, n = kr.poisson2d(64)
    rng = np.random.default_rng(2350)
    b = rng.standard_normal(n)
    keep = []
    a = _coo(S, (n, n), 0, keep=keep)
    f = ctx.fetch(ctx.factor_ilu0(a))
    F = (f[0].copy(), f[1].copy(), f[2].copy())
    want = kr.pcg(S, n, b, np.zeros(n), 1e-8, 300, kr.LU, F)
    assert want["reason"] == kr.CONVERGED
    for max_iter in (1, 300):
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, _coo(F, (n, n), -1, keep=keep), tol=1e-8, max_iter=max_iter, device=True)
        assert st.analyses == 2, max_iter
    _same(got, want, "natural order, raw F")
    h = capi.Operand(ctx, _coo(F, (n, n), 0, keep=keep), '.', capi.AS_A)
    try:
        y = ctx.solve_tri(h.coo, b, capi.TRI_LOWER, capi.DIAG_UNIT)
        ctx.solve_tri(h.coo, y, capi.TRI_UPPER, capi.DIAG_NONUNIT)
        before = h.bytes
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tol=1e-8, max_iter=300, device=True)
        assert st.analyses == 0 and h.bytes == before
        _same(got, want, "natural order, prepared F")
    finally:
        h.close()
    # the coloured ordering: P A P^T by spsamd_color + spsamd_extract, factored, solved for P b
    _color, perm, _ptr = ctx.color(a, capi.COLOR_ORDER_DEGREE, flags=capi.COLOR_SYMMETRIC)
    pa = ctx.fetch(ctx.extract(a, perm, perm))
    Sp = (pa[0].copy(), pa[1].copy(), pa[2].copy())
    ap = _coo(Sp, (n, n), 0, keep=keep)
    fp = ctx.fetch(ctx.factor_ilu0(ap))
    Fp = (fp[0].copy(), fp[1].copy(), fp[2].copy())
    bp = b[perm]
    wantp = kr.pcg(Sp, n, bp, np.zeros(n), 1e-8, 300, kr.LU, Fp)
    gotp, _ = _run(ctx, ap, bp, np.zeros(n), kr.LU, _coo(Fp, (n, n), 0, keep=keep), tol=1e-8, max_iter=300)
    _same(gotp, wantp, "coloured order")
    assert wantp["reason"] == kr.CONVERGED
    print("Poisson 64^2, ILU(0), tol 1e-8: %d iterations in the natural order, %d in the coloured one" % (
        want["iterations"], wantp["iterations"]))


@pytest.mark.parametrize("tM", ['.', 'T'])
def test_a_prepared_factor_keeps_its_schedules(ctx, tM):
    """M a prepared handle of transpose tM (stored transposed under 'T'): the first call builds and keeps the LOWER | UNIT and
    UPPER | NONUNIT schedules (analyses 2, the handle grows), the second finds them (analyses 0, no growth); a handle prepared
    the other way round is analysed per call.  The same bits every time."""
    from spsparse_amd import capi
    S, n = kr.poisson2d(12)
    rng = np.random.default_rng(2351)
    lo = S[0] > S[1]
    Sv = S[2].copy()
    Sv[lo] = Sv[lo] * (1.0 + 0.1 * rng.random(int(lo.sum())))                # F unsymmetric: a wrong triangle would show
    F = (S[0], S[1], fr.ilu0_ref((S[0], S[1], Sv), n)[0])
    b = rng.standard_normal(n)
    keep = []
    a = _coo(S, (n, n), 0, keep=keep)
    want = kr.pcg(S, n, b, np.zeros(n), 1e-10, 200, kr.LU, F)
    assert want["reason"] == kr.CONVERGED
    h = capi.Operand(ctx, _coo(_stored(F, tM), (n, n), -1, keep=keep), tM, capi.AS_A)
    try:
        b0 = h.bytes
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tM=tM, tol=1e-10, max_iter=200)
        _same(got, want, "first call, %s" % tM)
        b1 = h.bytes
        assert st.analyses == 2 and b1 > b0
        got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tM=tM, tol=1e-10, max_iter=200, device=True)
        _same(got, want, "second call, %s" % tM)
        assert st.analyses == 0 and h.bytes == b1
        # solve_tri finds the same two schedules
        y, s1 = ctx.solve_tri(h.coo, b, capi.TRI_LOWER, capi.DIAG_UNIT, tM, stats=True)
        _, s2 = ctx.solve_tri(h.coo, y, capi.TRI_UPPER, capi.DIAG_NONUNIT, tM, stats=True)
        assert (s1.analysis_reused, s2.analysis_reused) == (1, 1) and h.bytes == b1
    finally:
        h.close()
    other = 'T' if tM == '.' else '.'
    h = capi.Operand(ctx, _coo(_stored(F, tM), (n, n), -1, keep=keep), other, capi.AS_A)
    try:
        b1 = h.bytes
        for k in range(2):
            got, st = _run(ctx, a, b, np.zeros(n), kr.LU, h.coo, tM=tM, tol=1e-10, max_iter=200)
            _same(got, want, "a handle of the other transpose, %s" % tM)
            assert st.analyses == 2 and h.bytes == b1
    finally:
        h.close()


# ---------------------------------------------------------------- errors and trivia

def _raw(ctx, a, b, x, mem, precond=0, m=None, tol=1e-8, max_iter=10, pol=ar.ADD):
    return ctx.L.spsamd_solve_pcg(ctx.h, C.byref(a), b'.', precond, None if m is None else C.byref(m), b'.', b, x, mem, tol,
                                  max_iter, None, 0, pol, 0, None, None)


def test_errors_leave_x(ctx):
    from spsparse_amd import capi
    S, n = kr.poisson2d(4)
    keep = []
    a, wide = _coo(S, (n, n), 0, keep=keep), _coo(S, (n, n + 1), 0, keep=keep)
    S5, n5 = kr.poisson2d(5)
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
    oob = _coo((np.array([0, n], np.int32), np.array([0, 0], np.int32), np.ones(2)), (n, n), -1, keep=keep)
    assert _raw(ctx, oob, pb, px, capi.MEM_HOST) == -2
    assert np.all(x == SENT) and np.all(b == 1.0)
    res = ctx.consolidate(a, 0)                                          # a device x inside an output set
    assert _raw(ctx, a, res.val, res.val + 8 * n, capi.MEM_DEVICE) == -2
    got, _ = _run(ctx, a, b, np.zeros(n))                                # ... and the context still works
    _same(got, kr.pcg(S, n, b, np.zeros(n), 1e-8, 100), "after the refusals")


def test_trivia(ctx):
    keep = []
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    got, st = _run(ctx, _coo(E, (0, 0), -1, keep=keep), np.zeros(0), np.zeros(0))
    assert (got["iterations"], got["reason"], list(got["hist"])) == (0, kr.CONVERGED, [0.0])
    assert (st.bb, st.rr0, st.rr, st.launches) == (0.0, 0.0, 0.0, 0)
    S, n = kr.poisson2d(6)
    b = np.arange(1.0, n + 1)
    want = kr.pcg(S, n, b, np.zeros(n), 1e-8, 100)
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
    rc = ctx.L.spsamd_solve_pcg(ctx.h, C.byref(a), b'.', 0, None, b'.', b.ctypes.data, x.ctypes.data, 0, 1e-8, 100, None, 5,
                                ar.ADD, 0, None, None)
    assert rc == 0 and np.array_equal(x.view(np.int64), want["x"].view(np.int64))
