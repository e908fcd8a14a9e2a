"""tests/amg_ref.py pinned by hand-written cases (no GPU): the cycle of spsamd_amg_apply's header step by step, the rounding
order of the smoother, the signed zeros of pre = 0, the degenerate sweep counts, and the direction the feature rests on."""
from fractions import Fraction

import numpy as np
import pytest

from tests import amg_ref as am
from tests import krylov_ref as kr


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), "%s: %r, want %r" % (what, got, want)


def _dense(A):
    A = np.asarray(A, np.float64)
    i, j = np.nonzero(A)
    return i.astype(np.int32), j.astype(np.int32), A[i, j]


def _path4():
    """The path 0 - 1 - 2 - 3 with aggregates {0, 1} and {2, 3}: the Galerkin operator is [[2, -1], [-1, 2]]."""
    S = _dense([[2, -1, 0, 0], [-1, 2, -1, 0], [0, -1, 2, -1], [0, 0, -1, 2]])
    P = (np.arange(4, dtype=np.int32), np.array([0, 0, 1, 1], np.int32), np.ones(4))
    Sc = am.galerkin(S, [0, 0, 1, 1], 2)
    _same(Sc[2], [2.0, -1.0, -1.0, 2.0], "the Galerkin operator of the path")
    return [{"n": 4, "S": S, "P": P, "R": am.transposed(P)}, {"n": 2, "S": Sc, "P": None, "R": None}]


def test_two_level_cycle_on_a_path_step_by_step():
    """V(1,1), omega = 1/2, b = (4, 0, 8, -4): every intermediate is an integer or a dyadic fraction, worked by hand."""
    levels, trace = _path4(), []
    x = am.cycle(levels, (1, 1, 1, 0.5), [4.0, 0.0, 8.0, -4.0], trace=trace)
    want = [(0, "pre", [1.0, 0.0, 2.0, -1.0]),                  # 1/2 * (b / 2)
            (0, "r", [2.0, 3.0, 3.0, 0.0]),                     # b - (2, -3, 5, -4)
            (0, "bc", [5.0, 3.0]),
            (1, "coarse", [1.25, 0.75]),                        # 1/2 * (bc / 2)
            (0, "corrected", [2.25, 1.25, 2.75, -0.25]),
            (0, "post", [2.4375, 1.875, 3.625, -0.4375])]       # x + 1/2 * ((b - (3.25, -2.5, 4.5, -3.25)) / 2)
    assert [(l, name) for l, name, _ in trace] == [(l, name) for l, name, _ in want]
    for (l, name, got), (_, _, w) in zip(trace, want):
        _same(got, w, "level %d %s" % (l, name))
    _same(x, want[-1][2], "the cycle")
    # a second coarse sweep: q = (1.75, 0.25), e = (1.25, 0.75) + 1/2 * ((5 - 1.75, 3 - 0.25) / 2)
    trace = []
    am.cycle(levels, (1, 0, 2, 0.5), [4.0, 0.0, 8.0, -4.0], trace=trace)
    _same([t for t in trace if t[:2] == (1, "coarse")][-1][2], [2.0625, 1.4375], "two coarse sweeps")
    _same(trace[-1][2], [1.0 + 2.0625, 0.0 + 2.0625, 2.0 + 1.4375, -1.0 + 1.4375], "V(1,0) with two coarse sweeps")


def test_the_smoother_rounds_in_the_order_of_the_header():
    """diag(5, 7), b = (1.1, 1.1), omega = 2/3, two sweeps on one level.  Row 1 tells omega * (b / d) from (omega / d) * b in
    smooth0; row 0 tells omega * ((b - q) / d) from (omega / d) * (b - q) and from a fused x + omega * t in smooth."""
    om = 2.0 / 3.0
    d, b = np.array([5.0, 7.0]), np.array([1.1, 1.1])
    levels = [{"n": 2, "S": _dense(np.diag(d)), "P": None, "R": None}]
    x0 = [om * (b[i] / d[i]) for i in range(2)]
    assert x0[1] != (om / d[1]) * b[1]
    _same(am.cycle(levels, (0, 0, 1, om), b), x0, "smooth0")
    q = d[0] * x0[0]
    t = (b[0] - q) / d[0]
    x1 = x0[0] + om * t
    assert x1 != x0[0] + (om / d[0]) * (b[0] - q), "the case does not tell the two orders apart"
    assert x1 != float(Fraction(x0[0]) + Fraction(om) * Fraction(t)), "the case does not tell an FMA"
    got = am.cycle(levels, (0, 0, 2, om), b)
    assert _bits(got)[0] == _bits([x1])[0]


def test_pre_zero_takes_b_as_it_is_and_adds_the_correction_to_plus_zero():
    """pre = 0: r has b's bits (a NaN payload and a -0.0 included), and x = +0.0 + (P e): a correction built from e = -0.0
    comes out as +0.0, a negative one as itself."""
    S = _dense(np.diag([2.0, 2.0, 2.0]))
    P = (np.arange(3, dtype=np.int32), np.array([0, 1, 1], np.int32), np.ones(3))
    levels = [{"n": 3, "S": S, "P": P, "R": am.transposed(P)}, {"n": 2, "S": _dense(np.diag([-2.0, 4.0])), "P": None, "R": None}]
    b = np.array([0.0, -0.0, -8.0])
    b0 = b.copy()
    trace = []
    x = am.cycle(levels, (0, 0, 1, 0.5), b, trace=trace)
    named = {(l, name): v for l, name, v in trace}
    _same(named[(0, "r")], b0, "r under pre = 0")
    _same(named[(0, "bc")], [0.0, -8.0], "bc")                          # +0.0 + 1 * -0.0 is +0.0
    _same(named[(1, "coarse")], [-0.0, -1.0], "e")                      # 1/2 * (+0.0 / -2) is -0.0
    _same(x, [0.0, -1.0, -1.0], "x")
    nan = np.array([1.0, 2.0, 3.0])
    nan.view(np.uint64)[1] = 0x7FF80000DEADBEEF
    trace = []
    am.cycle(levels, (0, 1, 0, 0.5), nan, trace=trace)
    _same(trace[0][2], nan, "r under pre = 0 with a NaN")


def test_coarse_zero_and_a_single_level():
    levels = _path4()
    b = np.array([4.0, 0.0, 8.0, -4.0])
    # coarse = 0: e is +0.0, the correction changes nothing but a -0.0
    _same(am.cycle(levels, (1, 0, 0, 0.5), b), [1.0, 0.0, 2.0, -1.0], "V(1,0), coarse = 0")
    _same(am.cycle(levels, (1, 0, 0, -0.5), [4.0, 0.0, 8.0, -4.0]), [-1.0, 0.0, -2.0, 1.0], "a -0.0 of the sweep becomes +0.0")
    one = levels[:1]
    one = [{"n": 4, "S": one[0]["S"], "P": None, "R": None}]
    _same(am.cycle(one, (3, 3, 0, 0.5), b), np.zeros(4), "one level, coarse = 0")
    _same(am.cycle(one, (3, 3, 1, 0.5), b), [1.0, 0.0, 2.0, -1.0], "one level, coarse = 1: pre and post are not read")
    _same(am.cycle(one, (0, 0, 2, 0.5), b), [1.0 + 0.5, 0.0 + 0.75, 2.0 + 0.75, -1.0 + 0.0], "one level, coarse = 2")  # b - q = (2, 3, 3, 0)


def test_hierarchy_of_poisson_16_matches_the_issue_table():
    S, n = kr.poisson2d(16)
    levels = am.hierarchy(S, n)
    assert [lv["n"] for lv in levels] == [256, 37, 6]
    for lv in levels[:-1]:
        assert np.array_equal(np.sort(lv["R"][1]), np.arange(lv["n"])) and np.all(np.diff(lv["R"][0]) >= 0)


def test_no_amg_kernel_uses_scratch():
    from scripts import kernel_resources
    from spsparse_amd import build
    rows = {k: v for k, v in kernel_resources.library_kernels(build.build()).items() if "k_amg_" in k}
    names = "".join(rows)
    for word in ("k_amg_smooth0", "k_amg_smooth", "k_amg_residual", "k_amg_restrict", "k_amg_prolong", "k_amg_long", "k_amg_tail"):
        assert word in names, "%s is not in the library" % word
    for k, r in rows.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, "%s: %r" % (k, r)


def test_the_v_cycle_cuts_the_iterations_on_poisson_32():
    """On the reference alone: PCG with V(1,1), omega = 2/3, 4 coarse sweeps converges on Poisson 32^2 in fewer iterations
    than without a preconditioner."""
    S, n = kr.poisson2d(32)
    levels = am.hierarchy(S, n)
    assert [lv["n"] for lv in levels] == [1024, 150, 18, 3]
    b = kr.apply(S, n, np.ones(n))
    plain = am.pcg(levels, None, b, np.zeros(n), 1e-8, 400, precond=False)
    amg = am.pcg(levels, (1, 1, 4, 2.0 / 3.0), b, np.zeros(n), 1e-8, 400)
    assert plain["reason"] == am.CONVERGED and amg["reason"] == am.CONVERGED
    assert amg["iterations"] < plain["iterations"], (amg["iterations"], plain["iterations"])
    want = kr.pcg(S, n, b, np.zeros(n), 1e-8, 400)
    assert plain["iterations"] == want["iterations"] and np.array_equal(_bits(plain["x"]), _bits(want["x"]))
