"""The row-block partition of spsamd_multiply_stream, restated in numpy (include/spsparse_amd.h).

Over the consolidated op(A) and op(B): P_r = sum over the tuples (r, k) of op(A) of len_op(B)(k), bound_r =
min(P_r, cols(op(B))); the blocks are the maximal runs of consecutive rows, from row 0, whose bounds sum to at most the
budget.  A bound over the budget is SPSAMD_ECAPACITY."""
import numpy as np


class Capacity(Exception):
    def __init__(self, smallest):
        super().__init__("smallest budget that works: %d" % smallest)
        self.smallest = smallest


def row_bounds(a_rows, a_inner, nrow, b_rowlen, ncol):
    """Bounds of the rows of op(A).  a_rows / a_inner: op(A)'s consolidated tuples (each (r, k) once); b_rowlen: the
    tuple count of each row of op(B)."""
    P = np.zeros(int(nrow), np.uint64)
    np.add.at(P, np.asarray(a_rows, np.int64), np.asarray(b_rowlen, np.uint64)[np.asarray(a_inner, np.int64)])
    return np.minimum(P, np.uint64(ncol))


def blocks(bound, budget):
    """Row boundaries [r0, r1, ..., nrow] of the blocks; Capacity where a bound exceeds the budget."""
    bound = np.asarray(bound, np.uint64)
    if bound.size and int(bound.max()) > budget:
        raise Capacity(int(bound.max()))
    S = np.concatenate([[0], np.cumsum(bound, dtype=np.uint64)]).astype(np.uint64)
    edges = [0]
    b = 0
    while b < bound.size:
        lim = min(int(S[b]) + int(budget), (1 << 64) - 1)
        e = int(np.searchsorted(S, np.uint64(lim), side="right")) - 1
        edges.append(e)
        b = e
    return edges


def block_count(a_rows, a_inner, nrow, b_rowlen, ncol, budget):
    """stats.blocks: 0 when either consolidated operand is empty (nothing is computed)."""
    if len(a_rows) == 0 or int(np.sum(b_rowlen)) == 0:
        return 0
    return len(blocks(row_bounds(a_rows, a_inner, nrow, b_rowlen, ncol), budget)) - 1
