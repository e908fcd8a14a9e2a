"""spsamd_dist_multiply (csrc/dist.hip) at world sizes 3 .. 64 and at its kernels' edges.  GPU only.

All ranks of a communicator run in ONE process (tests/dist_ranks.py: a thread, a context and an spsamd_dist per rank on
device 0, a live all-to-allv between the threads as the transport callback), so every rank executes the C code of a
multi-GPU step: block consolidation, the status / mask / row-length round, the per-peer scans, the pack kernel, the panel
and its row array, the block product in its own configuration.  The cases come from tests/dist_ref.py, whose numpy model
says what every rank must SEND; tests/test_dist_host.py shows on the CPU that the model is sound and that each case is what
it claims.  Every comparison is bit for bit: small integer values, every sum exact in any order.

Per case and rank: the COO sink (SINK_ORDERED) equals the oracle's product of the whole matrices restricted to the rank's
rows; the digest sink's count, hash and sum are exact; every recorded send buffer of every call equals the model's bytes;
the four DistStats counters equal the model's; the transport is called exactly 5 times a step (6 under zero_nan, whose key
round is internal: those steps are checked end to end).  Errors and the communicator's state are host logic: nothing here
faults the GPU."""
import numpy as np
import pytest

from oracle import binding as orc
from tests import dist_ranks as dk
from tests import dist_ref as dr
from tests.gpu_util import Knobs, check_tuples, coo

pytestmark = pytest.mark.gpu

EINVAL, EHIP, EPEER = -2, -3, -7
COUNTERS = ("rows_heavy", "products", "products_tiles", "products_heavy", "shape0", "shape1", "nnz")


def blocks(c, rank, keep):
    """The rank's blocks of the stored operands as C structs over host arrays (B: None where B is A)."""
    a, b = c.block_a(rank), c.block_b(rank)
    return coo(a[:3], a[3], keep=keep), None if b is None else coo(b[:3], b[3], keep=keep)


def one_step(c, rank, ctx, dd, ex, zero_nan, sink, flags=0, ops=None):
    """One step of the case on this rank: (result, stats, the calls the transport recorded for it)."""
    keep = []
    sa, sb = ops if ops is not None else blocks(c, rank, keep)
    first = len(ex.log[rank])
    with Knobs(ctx, c.knobs):
        res, st = dd.multiply(sa, sb, c.b_bounds, tA=c.tA, tB=c.tB, duplicate_policy=c.policy, zero_nan=zero_nan, sink=sink, flags=flags)
    return res, st, ex.log[rank][first:]


def run_case(name, zero_nan=False):
    """Both sinks on every rank.  Returns (case, per rank a dict of what the rank got)."""
    from spsparse_amd import capi
    c = dr.case(name)
    ex = dk.Exchange(c.world)

    def fn(rank, ctx, dd):
        out = {}
        for key, sink, flags in (("coo", capi.SINK_COO, capi.SINK_ORDERED), ("digest", capi.SINK_DIGEST, 0)):
            res, st, calls = one_step(c, rank, ctx, dd, ex, zero_nan, sink, flags)
            out[key] = dict({k: int(getattr(res, k)) for k in COUNTERS}, hash=int(res.hash), sum=float(res.sum), calls=calls,
                            stats={k: int(getattr(st, k)) for k in ("block_nnz_a", "panel_tuples", "remote_tuples", "sent_tuples")})
            if sink == capi.SINK_COO:
                out[key]["tuples"] = tuple(ctx.fetch(res))
        return out
    ranks = dk.run_ranks(c.world, fn, exchange=ex)
    ranks.raise_first()
    return c, ranks.values


def check_product(c, got, zero_nan, what):
    """Every rank's COO tuples and digest against the oracle's whole product restricted to the rank's rows."""
    want = dr.oracle_product(c, zero_nan)
    for q in range(c.world):
        w = dr.rows_of(want, c.a_bounds[q], c.a_bounds[q + 1])
        g = got[q]
        check_tuples(g["coo"]["tuples"], w, "%s: rank %d of %d: COO sink" % (what, q, c.world))
        cnt, vsum, h = orc.digest(*w)
        d = g["digest"]
        assert (d["nnz"], d["hash"]) == (cnt, h), "%s: rank %d: digest sink: nnz %d hash %x, want %d %x" % (what, q, d["nnz"], d["hash"], cnt, h)
        assert d["sum"] == vsum or (np.isnan(d["sum"]) and np.isnan(vsum)), "%s: rank %d: digest sink: sum %r, want %r" % (what, q, d["sum"], vsum)
        for key in ("coo", "digest"):
            assert (g[key]["shape0"], g[key]["shape1"]) == (c.nrow, c.ncol), "%s: rank %d: shape" % (what, q)


def check_sends(c, m, got, what):
    """What every rank sent in both steps, its counters and the number of transport calls, against the model."""
    for q in range(c.world):
        for key in ("coo", "digest"):
            w = "%s, %s step" % (what, key)
            dr.compare_sends(m, q, got[q][key]["calls"], w)
            assert got[q][key]["stats"] == m.stats(q), "%s: rank %d: stats %r, want %r" % (w, q, got[q][key]["stats"], m.stats(q))


PLAIN = [n for n in dr.CATALOGUE if not n.startswith(("panel_rows", "planned_tiles", "zero_nan"))]


@pytest.mark.parametrize("name", PLAIN)
def test_rounds_and_product(name):
    """grid_edges (own blocks of 0, 1, 255 .. 1025 rows; n_inner + 1 at the block and the scan-tile edge), worlds (3 .. 64:
    the [peer][own row] tables, one to six scan batches, all PackDst slots, empty blocks, both 'T' flags, three policies,
    B_block = NULL), pack_edges (nothing / a selection / the whole block as it stands, also under a mask that is not all
    ones)."""
    c, got = run_case(name)
    check_product(c, got, False, name)
    check_sends(c, dr.model(name), got, name)


@pytest.mark.parametrize("n_inner", dr.PANEL_INNER)
def test_panel_row_array(n_inner):
    """The panel's row array (k_rows_from_ptr, k_rows_long) under a heavy hub row that reads every entry of it: 64-row
    groups with n_inner % 64 of 0, 1 and 63, empty rows inside a group, a wholly empty group, rows of exactly 2048 and 2049
    tuples, a long row that is the last one."""
    name = "panel_rows_%d" % n_inner
    c, got = run_case(name)
    for key in ("coo", "digest"):
        assert got[dr.PANEL_HUB_RANK][key]["rows_heavy"] >= 1, "%s, %s step: the hub row is not heavy: the row array was not read" % (name, key)
    check_product(c, got, False, name)
    check_sends(c, dr.model(name), got, name)


@pytest.mark.parametrize("kind,W", list(dr.PLANNED_A_BOUNDS))
def test_block_product_on_planned_tiles(kind, W):
    """The block product's own configuration -- a Prepared view over the panel's row pointer, the static tile walk -- on
    planned tiles (an L class under the second-generation hash tiles, a full-range bitmap cell), A cut by rows, B over the
    inner index."""
    name = "planned_tiles_%s_W%d" % (kind, W)
    c, got = run_case(name)
    for q in range(W):
        cut = dr.planned_cut(c, q)
        for key in ("coo", "digest"):
            g = got[q][key]
            assert g["rows_heavy"] == cut.rows_heavy, "%s: rank %d, %s step: rows_heavy %d, planned %d" % (name, q, key, g["rows_heavy"], cut.rows_heavy)
            assert (g["products_tiles"] > 0) == (cut.products_tiles > 0), "%s: rank %d, %s step: products_tiles %d, planned %d" % (
                name, q, key, g["products_tiles"], cut.products_tiles)
            assert g["products"] == cut.products
    check_product(c, got, False, name)
    check_sends(c, dr.model(name), got, name)


@pytest.mark.parametrize("zn", [False, True], ids=["keep_nan", "zero_nan"])
@pytest.mark.parametrize("W,same", dr.ZERO_NAN)
def test_zero_nan_leading_run_of_the_whole_matrix(W, same, zn):
    """The first kept tuple of op(B)'s reference sequence lies in the last rank's block, one block is all NaN and zeros: a
    leading run taken per block drops other NaNs than the reference.  Under zero_nan end to end (6 transport calls); with the
    NaNs kept the sends are the model's too."""
    c = dr.zero_nan(W, same)
    c, got = run_case(c.name, zero_nan=zn)
    check_product(c, got, zn, "%s, zero_nan %d" % (c.name, zn))
    if zn:
        for q in range(W):
            assert [len(got[q][key]["calls"]) for key in ("coo", "digest")] == [6, 6], "rank %d: transport calls" % q
    else:
        check_sends(c, dr.model(c.name), got, c.name)


# ---- errors and the communicator's state (host logic)

def error_case(W=4):
    rng = np.random.default_rng(7500)
    M = dr.rand_mat(rng, (30, 30), 300)
    b = [0, 6, 15, 21, 30]
    return dr.Case("errors", W, M, orc.Mat(M.idx0, M.idx1, M.val, M.shape), '.', '.', dr.ADD, b, b)


def spoiled(c, rank, kind, keep):
    """The rank's blocks with one of them spoiled: "miscut" -- the whole of B instead of its block; "index" -- an op(A) row
    index past the shape."""
    a, b = c.block_a(rank), c.block_b(rank)
    if kind == "miscut":
        b = (c.B.idx0, c.B.idx1, c.B.val, c.B.shape)
    if kind == "index":
        i0 = a[0].copy()
        i0[0] = c.nrow + 5
        a = (i0,) + a[1:]
    return coo(a[:3], a[3], keep=keep), coo(b[:3], b[3], keep=keep)


def failed_step(c, rank, ctx, dd, ex, ops=None, b_bounds=None):
    """(error code, message, transport calls) of a step that must fail."""
    from spsparse_amd import capi
    keep = []
    sa, sb = ops if ops is not None else blocks(c, rank, keep)
    first = len(ex.log[rank])
    try:
        dd.multiply(sa, sb, b_bounds or c.b_bounds, sink=capi.SINK_COO)
    except capi.SpsamdError as e:
        return e.code, e.msg, len(ex.log[rank]) - first
    raise AssertionError("rank %d: the step should have failed" % rank)


def good_step(c, rank, ctx, dd, ex):
    from spsparse_amd import capi
    res, st, calls = one_step(c, rank, ctx, dd, ex, False, capi.SINK_COO, capi.SINK_ORDERED)
    return tuple(ctx.fetch(res)), len(calls)


def check_good(c, values, what):
    want = dr.oracle_product(c, False)
    for q, (tuples, ncalls) in enumerate(values):
        check_tuples(tuples, dr.rows_of(want, c.a_bounds[q], c.a_bounds[q + 1]), "%s: rank %d" % (what, q))
        assert ncalls == 5


@pytest.mark.parametrize("bad", [{1: "miscut"}, {1: "index", 3: "miscut"}], ids=["one_in_the_middle", "two_in_different_ways"])
def test_errors_are_agreed_on(bad):
    """A bad rank that is neither first nor last, then two that are bad in different ways: each returns its own EINVAL, the
    others EPEER, all after round 1 (3 transport calls); a good step on the same communicators gives the right product."""
    c = error_case()
    ex = dk.Exchange(c.world)

    def fn(rank, ctx, dd):
        keep = []
        err = failed_step(c, rank, ctx, dd, ex, ops=spoiled(c, rank, bad.get(rank), keep))
        return err, good_step(c, rank, ctx, dd, ex)
    out = dk.run_ranks(c.world, fn, exchange=ex)
    out.raise_first()
    for q, ((code, msg, ncalls), _) in enumerate(out.values):
        assert code == (EINVAL if q in bad else EPEER), "rank %d: %d (%s)" % (q, code, msg)
        assert ncalls == 3, "rank %d: %d transport calls in the failed step" % (q, ncalls)
        if bad.get(q) == "miscut":
            assert "b_bounds" in msg, msg
        if bad.get(q) == "index":
            assert "another rank" not in msg and "b_bounds" not in msg, msg
    check_good(c, [v[1] for v in out.values], "after the agreed error")


def test_bounds_not_ascending():
    """Every rank returns EINVAL before any round; the communicator stays usable."""
    c = error_case()
    ex = dk.Exchange(c.world)

    def fn(rank, ctx, dd):
        return failed_step(c, rank, ctx, dd, ex, b_bounds=[0, 21, 15, 25, 30]), good_step(c, rank, ctx, dd, ex)
    out = dk.run_ranks(c.world, fn, exchange=ex)
    out.raise_first()
    for q, ((code, msg, ncalls), _) in enumerate(out.values):
        assert (code, ncalls) == (EINVAL, 0) and "ascending" in msg, "rank %d: %d, %d calls (%s)" % (q, code, ncalls, msg)
    check_good(c, [v[1] for v in out.values], "after the rejected bounds")


def test_world_size_limit():
    from spsparse_amd import capi
    ctx = capi.Context(0)
    try:
        with pytest.raises(capi.SpsamdError) as e:
            capi.Dist(ctx, 0, dr.MAX_WORLD + 1, transport=lambda *a: None)
        assert e.value.code == EINVAL
        capi.Dist(ctx, dr.MAX_WORLD - 1, dr.MAX_WORLD, transport=lambda *a: None).close()
        with pytest.raises(capi.SpsamdError):
            capi.Dist(ctx, dr.MAX_WORLD, dr.MAX_WORLD, transport=lambda *a: None)
    finally:
        ctx.close()


def test_transport_failure_in_round_one():
    """The transport fails on rank 2 in the mask segment of round 1: every rank returns EHIP; the next step on those objects
    is refused with EPEER before any round; fresh spsamd_dist objects on the same contexts work."""
    from spsparse_amd import capi
    c = error_case()
    ex = dk.Exchange(c.world, fail=lambda rank, call: (rank, call) == (2, 1))
    ex2 = dk.Exchange(c.world)

    def fn(rank, ctx, dd):
        first = failed_step(c, rank, ctx, dd, ex)
        second = failed_step(c, rank, ctx, dd, ex)
        fresh = capi.Dist(ctx, rank, c.world, transport=ex2.transport(rank, ctx.memcpy, lambda src, n: ctx.to_host(src, n, np.uint8).tobytes()))
        try:
            return first, second, good_step(c, rank, ctx, fresh, ex2)
        finally:
            fresh.close()
    out = dk.run_ranks(c.world, fn, exchange=ex, also_abort=[ex2])
    out.raise_first()
    assert isinstance(ex.errors[2][0], dk.PlantedFailure)
    for q, (first, second, _) in enumerate(out.values):
        assert first[0] == EHIP and first[2] == 2, "rank %d: %r" % (q, first)
        assert second[0] == EPEER and second[2] == 0 and "create a new one" in second[1], "rank %d: %r" % (q, second)
    check_good(c, [v[2] for v in out.values], "fresh communicators")
