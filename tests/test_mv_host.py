"""The inputs and the yardstick of tests/test_gpu_mv.py, without a GPU: the builders of tests/mv_ref.py reach every row
class (and the class boundaries exactly), the oracle's MV loop equals its MM loops on V as a k x 1 matrix bit for bit,
and the expected values of the sort0 == 0 / zero_nan cases are fixed here, by the oracle."""
import numpy as np
import pytest

from oracle import binding as orc
from tests import mv_ref as mr

K = 200000


def _same(a, b):
    """Index arrays equal, values bit-identical (NaN counts as NaN)."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2], equal_nan=True) and \
        np.array_equal(np.signbit(a[2]), np.signbit(b[2]))


def test_row_lengths_hold_every_boundary():
    lens = mr.row_lengths(np.random.default_rng(1), K)
    for n in mr.BOUNDARY_LENS + (K,):
        assert n in lens
    assert len(lens) == len(mr.BOUNDARY_LENS) + 1 + 180
    assert lens[len(mr.BOUNDARY_LENS) + 1:].min() >= 1 and lens[len(mr.BOUNDARY_LENS) + 1:].max() <= 9000
    small = mr.row_lengths(np.random.default_rng(1), 8193)
    assert small.max() == 8193 and 20000 not in small


def test_long_row_matrix_has_the_lengths_it_was_asked_for():
    rng = np.random.default_rng(2)
    lens = mr.row_lengths(rng, 30000, 40)
    A = mr.long_row_matrix(rng, 30000, lens, signed=True)
    assert A.shape == (len(lens), 30000) and A.nnz == lens.sum()
    assert np.array_equal(np.bincount(A.idx0, minlength=len(lens)), lens)
    key = A.idx0.astype(np.int64) * 30000 + A.idx1
    assert np.unique(key).size == key.size                     # distinct columns in every row
    assert np.any(np.diff(key) < 0)                            # shuffled storage order
    assert (A.val < 0).any() and (A.val > 0).any() and not (A.val == 0).any()
    D = mr.long_row_matrix(np.random.default_rng(3), 30000, lens[:20], dups=500, zeros=300, tile_rows=3)
    assert D.shape == (23, 30000) and (D.val == 0).sum() == 300
    nz = D.val != 0
    places = np.unique(D.idx0[nz].astype(np.int64) * 30000 + D.idx1[nz])
    per_row = np.bincount(places // 30000, minlength=23)
    assert np.array_equal(per_row[:20], lens[:20])              # duplicates repeat places, they add none
    assert np.all((per_row[20:] >= 200) & (per_row[20:] <= mr.TILE_LMAX)) and D.idx1[D.idx0 >= 20][nz[D.idx0 >= 20]].max() < mr.DENSE_K
    assert D.nnz == per_row.sum() + 500 + 300


@pytest.mark.parametrize("k", [K, K // 2])
def test_dense_v_reaches_every_class_and_the_boundaries(k):
    """With a dense V a row's product count is its length, so the classes are known by construction."""
    rng = np.random.default_rng(1)
    lens = mr.row_lengths(rng, k)
    A = mr.long_row_matrix(rng, k, lens)
    rc = mr.row_classes(A, mr.dense_vec(rng, k))
    assert np.array_equal(rc.products, lens)
    for p in (64, 65, 4096, 4097):
        assert rc.at(p) >= 1
    assert rc.rows_light == ((lens >= 1) & (lens <= 64)).sum() >= 4
    assert rc.rows_mid == ((lens > 64) & (lens <= 4096)).sum() >= 10
    assert rc.rows_heavy == (lens > 4096).sum() >= 8
    assert rc.total == lens.sum() and not rc.all_light
    assert rc.tile_rows_heavy == 0                             # a heavy MV row has more than 4096 tuples of A: never a tile row
    rt = mr.row_classes(mr.transposed(A), mr.dense_vec(rng, k), tA='T')
    assert np.array_equal(rt.products, lens)


def test_every_gpu_input_has_rows_in_each_class():
    """The class counts of the other inputs tests/test_gpu_mv.py multiplies (same seeds, same arguments)."""
    from tests import test_gpu_mv as g
    seen = 0
    for name, (A, V, kw) in g.mv_cases().items():
        rc = mr.row_classes(A, V, tA=kw.get("tA", "."), scalei=kw.get("scalei"), scalej=kw.get("scalej"),
                            duplicate_policy=kw.get("duplicate_policy", orc.ADD), zero_nan=kw.get("zero_nan", False))
        assert rc.rows_light > 0 and rc.rows_mid > 0 and rc.rows_heavy > 0, name
        seen += 1
    assert seen >= 8
    A = g.narrow_a()
    for n in mr.NARROW_N:
        B, kw = g.narrow_case(n)
        rc = mr.row_classes(A, B, tB=kw["tB"])
        assert rc.rows_light > 0 and rc.rows_heavy > 0, n
        if n >= 63:
            assert rc.tile_rows_heavy > 0, n                    # 200+ tuples of A x full B rows of n >= 63 columns
    C, kinds = mr.cancel_matrix(g.K_CANCEL)
    rc = mr.row_classes(C, mr.ones_vec(g.K_CANCEL))
    assert (rc.rows_light, rc.rows_mid, rc.rows_heavy) == (6, 6, 6)


def test_scales_and_policies_change_the_product_count():
    """row_classes against a count by hand on a small case.  Consolidation drops explicit zeros BEFORE it merges duplicates
    (so no policy can bring one back) and keeps a merged sum of 0 as a tuple; a scalej entry that is absent drops a
    product, one that is 0 does not; a scalei entry that is absent or 0 drops the row."""
    A = orc.Mat([0, 0, 0, 1, 1, 2, 2], [0, 1, 1, 0, 2, 2, 2], [1., 2., -2., 0., 3., 1., 0.], (3, 3))
    V = orc.Vec([0, 1, 2, 2], [1., 1., 0., 5.], 3)
    for pol in (orc.ADD, orc.REPLACE, orc.LEAVE_ALONE):
        # row 0: (0,0) and the merged (0,1) (2 - 2 = 0 under ADD: still a tuple); row 1: (1,2); row 2: (2,2) = 1; V[2] = 5
        assert mr.row_classes(A, V, duplicate_policy=pol).products.tolist() == [2, 1, 1]
        assert len(orc.multiply_mv(A, V, duplicate_policy=pol)[0]) == 3
    assert mr.row_classes(A, orc.Vec([0, 2, 2], [1., 0., 0.], 3)).products.tolist() == [1, 0, 0]
    assert mr.row_classes(A, V, scalej=orc.Vec([0, 1], [1., 0.], 3)).products.tolist() == [2, 0, 0]
    assert mr.row_classes(A, V, scalei=orc.Vec([0, 1], [0., 2.], 3)).products.tolist() == [0, 1, 0]
    assert mr.row_classes(mr.transposed(A), V, tA='T').products.tolist() == [2, 1, 1]
    rc = mr.row_classes(A, V)
    assert (rc.rows_light, rc.rows_mid, rc.rows_heavy, rc.total, rc.all_light) == (3, 0, 0, 4, True)


@pytest.mark.parametrize("kw", [{}, {"scalei": True}, {"scalej": True}, {"scalei": True, "scalej": True, "C_": -2.5}],
                         ids=["plain", "scalei", "scalej", "all"])
@pytest.mark.parametrize("tA", [".", "T"])
def test_oracle_mv_equals_mm_on_a_column(kw, tA):
    """orc.multiply_mv(A, V) == orc.multiply(A, V as k x 1) bit for bit, for the reference's inner-product loop and for
    the row-wise checker (k reduced: the reference's loop is quadratic), signed values, duplicates and zeros."""
    rng = np.random.default_rng(5)
    m, k = 40, 3000
    A = mr.long_row_matrix(rng, k, np.concatenate([[0, 1, 64, 65, k], rng.integers(1, k, m - 5)]), signed=True, dups=400, zeros=200)
    if tA == "T":
        A = mr.transposed(A)
    V = mr.messy_vec(rng, k, 2 * k)
    V.val *= rng.choice([-1.0, 1.0], V.nnz)
    args = dict(tA=tA, C_=kw.get("C_", 1.0), scalei=mr.scale_vec(rng, m) if kw.get("scalei") else None,
                scalej=mr.scale_vec(rng, k) if kw.get("scalej") else None)
    mv = orc.multiply_mv(A, V, **args)
    assert len(mv[0]) > 20 and mv[1] is None and mv[3] == (m,)
    for rowwise in (False, True):
        mm = orc.multiply(A, mr.as_column(V), rowwise=rowwise, **args)
        assert mm[3] == (m, 1) and not mm[1].any()
        assert _same(mv, mm), rowwise


def test_oracle_mv_equals_mm_at_full_size():
    """The same identity at the size the GPU tests use, for the row-wise checker (the GPU test compares MM with one output
    column to the MV result through it)."""
    rng = np.random.default_rng(1)
    A = mr.long_row_matrix(rng, K, mr.row_lengths(rng, K), signed=True)
    V = mr.dense_vec(rng, K, signed=True)
    si = mr.scale_vec(rng, A.shape[0])
    for args in ({}, {"scalei": si}):
        assert _same(orc.multiply_mv(A, V, **args), orc.multiply(A, mr.as_column(V), rowwise=True, nthreads=4, **args))


def test_sorted_v_is_taken_as_stored_under_zero_nan():
    """Consolidate<> trusts a V that carries sort order {0} (algorithm.hpp:360): its leading NaN, and an explicit zero,
    stay in the join whatever zero_nan says.  A V without the order is consolidated, and zero_nan then drops the NaN
    that leads the sequence and every zero.  These are the expected values of the GPU cases."""
    A = orc.Mat([0, 0], [0, 1], [1., 1.], (1, 2))
    for zn in (False, True):
        got = orc.multiply_mv(A, orc.Vec([0, 1], [np.nan, 2.0], 2, 0), zero_nan=zn)
        assert got[0].tolist() == [0] and np.isnan(got[2][0])
    assert np.isnan(orc.multiply_mv(A, orc.Vec([0, 1], [np.nan, 2.0], 2, -1), zero_nan=False)[2][0])
    assert orc.multiply_mv(A, orc.Vec([0, 1], [np.nan, 2.0], 2, -1), zero_nan=True)[2].tolist() == [2.0]
    # an explicit zero of a sorted V meets an Inf of A: Inf * 0 = NaN poisons the row; consolidated, the zero is gone
    Ai = orc.Mat([0, 0], [0, 1], [np.inf, 1.], (1, 2))
    for zn in (False, True):
        assert np.isnan(orc.multiply_mv(Ai, orc.Vec([0, 1], [0.0, 2.0], 2, 0), zero_nan=zn)[2][0])
        assert orc.multiply_mv(Ai, orc.Vec([0, 1], [0.0, 2.0], 2, -1), zero_nan=zn)[2].tolist() == [2.0]
