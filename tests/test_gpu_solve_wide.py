"""spsamd_solve_tri where the analysis leaves one workgroup: frontiers above capi.peel_thin_max rows (k_peel_wide, one
level per launch, capi.peel_batch launches between two looks of the host at the frontier size), the hand-overs between it
and k_peel_thin, frontiers and levels wider than a capped grid, hub rows and columns, and offsets beyond 2^32 values.

Checked as tests/test_gpu_solve.py checks: every value of X as a bit pattern against tests/solve_ref.py, the schedule's
figures equal.  The operands are built with their level vector known (solve_ref.by_levels; tests/test_solve_host.py pins
the builders), a level's rows scattered over the triangle, and every test asserts that the peel launches the call reports
equal solve_ref.peel_plan of its own level sizes -- and that this plan holds what the test is named for."""
import functools

import numpy as np
import pytest

from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import select_ref as sel
from tests import solve_ref as sr
from tests.gpu_util import bits_same as _bits_same, coo as _coo, ctx, forced, rhs as _rhs, solve as _solve  # noqa: F401

pytestmark = pytest.mark.gpu


def _TK():
    from spsparse_amd import capi
    return capi.peel_thin_max, capi.peel_batch


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(sizes):
    return sr.peel_plan(sizes, *_TK())


def _check(ctx, A, n, lev, B, want, what, sort0=0, uplo=0, diag=0, t='.', pol=ar.ADD, S=None, a=None):
    """One device solve of the operand against `want`; the schedule's figures and the peel launches against lev.  S: the
    operand as the call takes it, where tuples_used and zero_pivot have to be counted; without it A is a by_levels operand
    solved NONUNIT on its own triangle: every stored tuple is used and every diagonal is positive."""
    keep = []
    if a is None:
        a = _coo(A, (n, n), sort0, device=True, keep=keep)
    X, st = _solve(ctx, a, B, uplo, diag, t, pol, device=True)
    sizes = np.bincount(lev)
    assert (st.peel_thin_launches, st.peel_wide_launches) == _plan(sizes), what
    _bits_same(X, want, what)
    assert (st.levels, st.max_level_rows) == (sizes.size, sizes.max()), what
    if S is None:
        assert diag == 0 and (st.tuples_used, st.zero_pivot) == (len(A[2]), -1), what
    else:
        assert st.tuples_used == sr.tuples_used(S, uplo, diag) and st.zero_pivot == sr.zero_pivot(S, n, uplo, diag), what
    assert st.analysis_reused == 0
    return st


# ---------------------------------------------------------------- runs of wide levels

def _run_sizes(k):
    T, K = _TK()
    if k in ("cut", "2K-cut"):                                         # one / two full batches, then five rows: a thin launch after them
        return [T + 1] * (K if k == "cut" else 2 * K) + [5]
    return [T + 1] * {"K-1": K - 1, "K": K, "K+1": K + 1, "2K": 2 * K, "2K+1": 2 * K + 1}.get(k, k)


@pytest.mark.parametrize("k", [1, 2, 3, "K-1", "K", "K+1", "2K", "2K+1", "cut", "2K-cut"])
def test_runs_of_wide_levels(ctx, k):
    """k consecutive frontiers of peel_thin_max + 1 rows: none, part, all of a batch, and batches that begin on the second
    and third of the rotating counters; `cut`, `2K-cut`: the host finds a thin frontier behind one and behind two full
    batches, so k_peel_thin starts from the second and from the third counter."""
    K = _TK()[1]
    sizes = _run_sizes(k)
    n_lev = len(sizes)
    want_plan = (0, 0) if n_lev == 1 else (1, n_lev // K * K) if sizes[-1] == 5 else (0, K * -(-n_lev // K))
    assert _plan(sizes) == want_plan
    rng = np.random.default_rng(100 + n_lev)
    A, n, lev = sr.by_levels(rng, sizes)
    B = _rhs(rng, n, 2, 0.0)
    _check(ctx, A, n, lev, B, sr.solve_fast(A, n, B, lev=lev), "run %s" % k, S=A)


def test_a_schedule_built_by_the_wide_path_is_kept(ctx):
    """A prepared handle on K + 1 wide levels: the second solve, after an unrelated multiply has overwritten the workspace,
    reuses the schedule: no peel launch, equal bits."""
    from spsparse_amd import capi
    T, K = _TK()
    sizes = _run_sizes("K+1")
    rng = np.random.default_rng(31)
    A, n, lev = sr.by_levels(rng, sizes)
    B = _rhs(rng, n, 2, 0.0)
    want = sr.solve_fast(A, n, B, lev=lev)
    keep = []
    h = capi.Operand(ctx, _coo(A, (n, n), -1, False, keep), '.', capi.AS_A, capi.ADD, False)
    try:
        st = _check(ctx, A, n, lev, B, want, "prepared, first", S=A, a=h.coo)
        assert st.peel_wide_launches == 2 * K
        m, mkeep = capi.host_coo(*wl.rmat(12, seed=2))
        assert ctx.multiply(m, m, sink=capi.SINK_DIGEST).nnz > 0
        X, st2 = _solve(ctx, h.coo, B, device=True)
        _bits_same(X, want, "prepared, again")
        assert (st2.analysis_reused, st2.peel_thin_launches, st2.peel_wide_launches) == (1, 0, 0)
        assert (st2.levels, st2.max_level_rows, st2.tuples_used, st2.zero_pivot) == (K + 1, T + 1, len(A[2]), -1)
    finally:
        h.close()


# ---------------------------------------------------------------- the threshold

def test_the_threshold_between_the_two_peels(ctx):
    """Frontiers of T - 1, T and T + 1 rows, T = peel_thin_max: T rows behind a thin level stay in the workgroup; T rows
    as the first thing the host sees after a batch go back into it; T + 1 leave it.  Three thin stretches, two of them
    longer than a batch, with wide stretches between: k_peel_thin is entered after a batch twice, and left for a wide
    frontier three times."""
    T, K = _TK()
    filler = ([T, T - 1, T + 1, 9] * K)[:K - 1]
    sizes = ([3, T - 1, T, 7]                                          # thin launch 1: T follows a thin level
             + [T + 1] + filler                                        # batch 1: K levels, thin and wide ones inside it
             + [T] + [50] * (K + 2)                                    # the host sees T: thin launch 2, more than K levels
             + [T + 1, T + 1] + [40] * (K - 2)                         # batch 2
             + [T - 1] + [33] * (K + 1)                                # thin launch 3, more than K levels
             + [T + 1])                                                # batch 3: the last level and K - 1 empty frontiers
    assert _plan(sizes) == (3, 3 * K)
    assert sizes[4 + K] == T                                           # (the level the host reads after batch 1)
    rng = np.random.default_rng(32)
    A, n, lev = sr.by_levels(rng, sizes)
    B = _rhs(rng, n, 2, 0.0)
    _check(ctx, A, n, lev, B, sr.solve_fast(A, n, B, lev=lev), "threshold", S=A)


# ---------------------------------------------------------------- wider than the grid

def test_frontiers_wider_than_the_peel_grid(ctx):
    """Two consecutive frontiers of one row more than k_peel_wide's grid holds (8 workgroups of 256 per CU): its
    grid-stride loop takes a second trip, in two launches running."""
    K = _TK()[1]
    G = _cus() * 8 * 256 + 1
    sizes = [300, G, G, 100]
    assert _plan(sizes) == (1, K)
    rng = np.random.default_rng(33)
    A, n, lev = sr.by_levels(rng, sizes)
    B = _rhs(rng, n, 1, 0.0)
    _check(ctx, A, n, lev, B, sr.solve_fast(A, n, B, lev=lev), "two frontiers of %d rows" % G)


# ---------------------------------------------------------------- hubs

H = 20000


@functools.lru_cache(maxsize=None)
def _hub(case):
    """(A, n, lev, B, X wanted) of a hub case, built once: the UPPER tests mirror it."""
    T, K = _TK()
    rng = np.random.default_rng({"a": 41, "b": 42, "c": 43}[case])
    if case == "a":                                                    # alone in its frontier; its H dependants are a wide one
        sizes, kw, plan = [1, H, 60], {"fan": {0: H}}, (1, K)
    elif case == "b":                                                  # one of T + 1 frontier rows, the others with 1 or 2 dependants
        sizes, kw, plan = [T + 1, H + T + T // 2, 60], {"fan": {0: H}}, (0, K)
    else:                                                              # H rows of one wide level decrement one in-degree
        sizes, kw, plan = [30, H + 100, 50, 20], {"gather": {2: H}}, (1, K)
    assert _plan(sizes) == plan and max(sizes) > T
    A, n, lev = sr.by_levels(rng, sizes, **kw)
    B = _rhs(rng, n, 3, 0.0)
    return A, n, lev, B, sr.solve_fast(A, n, B, lev=lev)


@pytest.mark.parametrize("upper", [0, 1])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_hubs(ctx, case, upper):
    """A column of H = 20000 dependants walked by one thread of k_peel_thin (a) and inside a wave of k_peel_wide whose other
    rows have one or two (b); a row of H used tuples naming one wide level (c), solved by every long-row kernel.  upper:
    the same graph under the numbering n - 1 - i, stored transposed and solved as the UPPER triangle under 'T'."""
    A, n, lev, B, want = _hub(case)
    sort0, t = 0, '.'
    if upper:
        U, lev = sr.mirrored(A, n, lev)
        B = B[::-1].copy()
        want = sr.solve_fast(U, n, B, sr.UPPER, lev=lev)
        A, sort0, t = (U[1], U[0], U[2]), 1, 'T'
        assert np.array_equal(sel.operand_S(A, 'T', sort0=1)[0], U[0])
    for row in (0, 2, 3) if case == "c" else (0,):
        with forced(ctx, "solve_row", row):
            _check(ctx, A, n, lev, B, want, "hub %s upper %d solve_row %d" % (case, upper, row), sort0, upper, 0, t)


# ---------------------------------------------------------------- semantics on wide frontiers

@functools.lru_cache(maxsize=None)
def _noisy():
    T = _TK()[0]
    rng = np.random.default_rng(51)
    A, n, lev = sr.by_levels(rng, [T + 1] * 3)
    drop, nz = (int(x) for x in np.flatnonzero(lev == 1)[[5, 900]])
    return sr.pattern_noise(rng, A, n, lev, drop, nz), n, lev, _rhs(rng, n, 3, 0.0), min(drop, nz)


@pytest.mark.parametrize("diag", [0, 1])
@pytest.mark.parametrize("t", ['.', 'T'])
@pytest.mark.parametrize("uplo", [0, 1])
def test_semantics_on_wide_frontiers_trusted(ctx, uplo, t, diag):
    """Three frontiers of T + 1 rows of a trusted operand with duplicated and explicit-zero off-diagonal tuples (each
    decrements once), the other triangle populated (NaN: never read), a missing and a -0.0 diagonal."""
    K = _TK()[1]
    N, n, lev, B, zp = _noisy()
    if uplo:
        N, lev = sr.mirrored(N, n, lev)
        B = B[::-1].copy()
    A, sort0 = ((N[1], N[0], N[2]), 1) if t == 'T' else (N, 0)
    S = sel.operand_S(A, t, sort0=sort0)                               # trusted: S is N as stored
    assert np.array_equal(S[0], N[0]) and np.array_equal(S[1], N[1])
    assert _plan(np.bincount(lev)) == (0, K)
    want = sr.solve_fast(S, n, B, uplo, diag, lev=lev)
    what = "trusted uplo %d %s diag %d" % (uplo, t, diag)
    st = _check(ctx, A, n, lev, B, want, what, sort0, uplo, diag, t, S=S)
    assert (st.zero_pivot >= 0) == (diag == 0) and np.all(np.isfinite(want)) == bool(diag), what
    assert uplo or diag or st.zero_pivot == zp, what


@pytest.mark.parametrize("pol,uplo,t,diag", [(ar.LEAVE_ALONE, 0, '.', 0), (ar.ADD, 1, 'T', 0), (ar.REPLACE, 0, 'T', 1)])
def test_semantics_on_wide_frontiers_raw(ctx, pol, uplo, t, diag):
    """The same tuples raw, in shuffled order: consolidated under each duplicate policy (duplicates merged, zeros
    dropped), then three wide frontiers all the same."""
    K = _TK()[1]
    N, n, lev, B, _ = _noisy()
    if uplo:
        N, lev = sr.mirrored(N, n, lev)
        B = B[::-1].copy()
    rng = np.random.default_rng(52 + pol)
    o = rng.permutation(len(N[2]))
    A = (N[1][o], N[0][o], N[2][o]) if t == 'T' else tuple(x[o] for x in N)
    S = sel.operand_S(A, t, pol, False, -1)
    assert len(S[2]) < len(N[2])
    assert np.array_equal(sr.levels(S, n, uplo, diag), lev) and _plan(np.bincount(lev)) == (0, K)
    want = sr.solve_fast(S, n, B, uplo, diag, lev=lev)
    _check(ctx, A, n, lev, B, want, "raw pol %d uplo %d %s diag %d" % (pol, uplo, t, diag), -1, uplo, diag, t, pol, S=S)


# ---------------------------------------------------------------- the numeric phase past its capped grid

def test_levels_with_more_pairs_than_the_serial_grid(ctx):
    """Two levels of 256 rows per CU and one more, at 64 right-hand sides: 64 (row, rhs) pairs more than k_solve_serial's
    capped grid of 64 workgroups per CU has threads, so it strides -- under the default path and with a launch per level."""
    K = _TK()[1]
    R = _cus() * 256 + 1
    sizes = [R, R]
    assert R * 64 > _cus() * 64 * 256 and _plan(sizes) == (0, K)
    rng = np.random.default_rng(61)
    A, n, lev = sr.by_levels(rng, sizes)
    B = _rhs(rng, n, 64, 0.0)
    want = sr.solve_fast(A, n, B, lev=lev)
    for path in (0, 1):
        with forced(ctx, "solve_path", path):
            st = _check(ctx, A, n, lev, B, want, "solve_path %d" % path, S=A)
        assert (st.launches, st.fused_levels) == (2, 0)


# ---------------------------------------------------------------- offsets beyond 2^32 values

def test_offsets_beyond_2_to_the_32(ctx):
    """n * ld > 2^32 values (B = X about 34 GB on the device, solved in place), the dependencies among rows 0, 1 and the last
    40: row * ld in 64 bits in the serial, fused, lanes and fold kernels.  Every row of X[:, :3] is compared, and the rest of
    the array is still zero."""
    import torch
    dev = torch.device("cuda", 0)
    n, ld, nrhs = (1 << 22) + 8, 1025, 3
    assert n * ld > 1 << 32
    rng = np.random.default_rng(71)
    A, lev, named = sr.far_rows(rng, n)
    Bh = np.zeros((n, nrhs))
    Bh[named] = rng.standard_normal((named.size, nrhs))
    want = sr.solve_fast(A, n, Bh, lev=lev)
    assert np.all(want[named] != 0)
    keep = []
    a = _coo(A, (n, n), 0, device=True, keep=keep)
    X = torch.zeros((n, ld), dtype=torch.float64, device=dev)
    idx = torch.from_numpy(named.astype(np.int64)).to(dev)
    try:
        for row in (0, 2, 3):
            X[idx, :nrhs] = torch.from_numpy(Bh[named]).to(dev)
            torch.cuda.synchronize()
            with forced(ctx, "solve_row", row):
                _, st = ctx.solve_tri(a, X[:, :nrhs], X=X[:, :nrhs], stats=True)
            _bits_same(X[:, :nrhs].cpu().numpy(), want, "64-bit solve_row %d" % row)
            assert (st.levels, st.max_level_rows, st.tuples_used, st.zero_pivot) == (42, n - 41, len(A[2]), -1)
            assert (st.peel_thin_launches, st.peel_wide_launches) == _plan(np.bincount(lev))
        assert int(torch.count_nonzero(X[:, nrhs:])) == 0, "the padding of X was written"
    finally:
        del X
        torch.cuda.empty_cache()
