"""tests/emit_ref.py on the CPU: the restatement of hash_emit's dispatch pinned with literal values (and against the lines
of the sources it restates), the catalogue's records, its coverage of every feasible (kernel, table, ordering), and every
case through the oracle -- at 2^31 columns too, where the oracle must need neither time nor memory by the column."""
import os
import re
import resource
import time

import numpy as np
import pytest

from tests import emit_ref as er
from tests import tile_plan as tp
from tests.emit_ref import BITMAP, BITONIC, RADIX, Rec

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spsparse_amd", "csrc")

# (kernel, T) -> (widest colbits on the bitmap rank, widest on the radix sort); beyond: the bitonic network
TABLE = {("k_hash", 1024): (15, 23), ("k_few", 1024): (15, 23), ("k_hash", 3072): (16, 21), ("k_hash", 4096): (17, 21),
         ("k_few", 4096): (17, 21), ("k_hash", 8192): (None, 20), ("k_few", 8192): (18, 20), ("tiles", 4096): (17, 21)}


def test_threshold_table():
    for (kern, T), (bm, rx) in TABLE.items():
        assert er.thresholds(kern, T) == (bm, rx), (kern, T)
        for b in range(1, 33):
            want = BITMAP if bm is not None and b <= bm else (RADIX if b <= rx else BITONIC)
            assert er.emit_path(kern, T, b) == want, (kern, T, b)
            # the knob only skips orderings
            assert er.emit_path(kern, T, b, 1) == (RADIX if b <= rx else BITONIC), (kern, T, b)
            assert er.emit_path(kern, T, b, 2) == BITONIC
    assert [er.pbits(T) for T in (1024, 3072, 4096, 8192)] == [9, 11, 11, 12]
    # at the last radix width the key (col - colbase) << PBITS | position fills all 32 bits
    assert all(rx + er.pbits(T) == 32 for (kern, T), (bm, rx) in TABLE.items())


def test_routing_literals():
    assert [er.colbits(n) for n in (1, 2, 3, 64, 65, 513, 1 << 15, (1 << 15) + 1, 1 << 26, 1 << 31)] == [1, 1, 2, 6, 7, 10, 15, 16, 26, 31]
    assert [er.table_class(P) for P in (0, 64, 65, 512, 513, 2048, 2049, 4096, 4097)] == [None, None, 1024, 1024, 4096, 4096, 8192, 8192, None]
    assert [er.kernel(L) for L in (1, 8, 9, 16)] == ["k_few", "k_few", "k_hash", "k_hash"]
    assert [er.kernel(L, 16) for L in (16, 17)] == ["k_few", "k_hash"] and er.kernel(17, 100) == "k_hash" and er.kernel(16, 100) == "k_few"
    assert er.kernel(1, -1) == "k_hash" and er.kernel(1, 0, ordered=True) == "k_hash" and er.kernel(2, 1) == "k_hash"


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restatement_against_the_sources():
    """The lines that emit_ref restates, as they stand in the sources: the two dispatch conditions and PBITS of hash_emit,
    the (T, NT) of every launch that reaches it, the classes and the routing.  A change to one of them -- say k_few's table of
    8192 no longer on the bitmap rank, which changes no result and which no GPU test can see -- fails here until the
    restatement, its pinned table and the coverage lists follow."""
    h = _source("spgemm_hash.h")
    assert "constexpr uint32_t PBITS = T <= 1024 ? 9 : (T <= 4096 ? 11 : 12);" in h
    assert "constexpr int NSB = T / 8;" in h
    assert "if (NSB <= NT && colrange <= (uint32_t)T * 32u && ep.emit_path < 1) {" in h
    assert "if (colbits + PBITS <= 32 && ep.emit_path < 2) {" in h
    assert "const uint32_t colrange = colbits >= 32 ? 0xFFFFFFFFu : (1u << colbits);" in h
    assert len(re.findall(r"ep\.emit_path", h)) == 2 and len(re.findall(r"\bNSB\b", h)) == 3
    few = _source("k_few.hip")
    assert {(int(t), int(n)) for t, n in re.findall(r"launch_few<(\d+), (\d+), MODE>", few)} == set(er.NT["k_few"].items())
    assert len(re.findall(r"hash_emit<", few)) == 1 and "hash_emit<T, NT, MODE, false>(" in few and "s_cnt, 0, ep.ncolbits, m," in few
    kh = _source("k_hash.hip")
    assert {(int(t), int(n)) for t, n in re.findall(r"launch_hash<(\d+), (\d+), MODE, (?:true|false)>", kh)} == set(er.NT["k_hash"].items())
    assert {int(t) for t in re.findall(r"launch_hash<(\d+), \d+, MODE, false>", kh)} == {T for T, lo, hi in er.CLASSES}
    assert "s_cnt, 0, ep.ncolbits, m, beg, end, pthr);" in kh
    dev = _source("spgemm_dev.h")
    assert "#define TILE_NT_V 512" in dev and "constexpr int TILE_T = TILE_NT * 8;" in dev and "#define MID_MAX_V 4096" in dev
    assert "constexpr int FEW_MAX_DEFAULT = 8;" in dev and "constexpr uint32_t FEW_LMAX = 16;" in dev
    sp = _source("spgemm.hip")
    assert "if (P <= 64) return 4;" in sp and "if (P <= 512) return 5;" in sp and "if (P <= 2048) return 6;" in sp and "if (P <= MID_MAX) return 7;" in sp
    assert "if (b >= 5 && b <= 7 && (int)La <= few_max) b += BIN_FEW - 5;" in sp
    assert "ncol > 1 ? (uint32_t)(64 - __builtin_clzll((unsigned long long)(ncol - 1))) : 1u" in sp


# ---- the mid rows' catalogue

# width -> the ordering of (k_hash and k_few at 1024, at 4096, k_hash at 8192, k_few at 8192)
B_, R_, N_ = BITMAP, RADIX, BITONIC
NATURAL = {1: (B_, B_, R_, B_), 2: (B_, B_, R_, B_), 64: (B_, B_, R_, B_), 65: (B_, B_, R_, B_), 513: (B_, B_, R_, B_),
           1 << 15: (B_, B_, R_, B_), (1 << 15) + 1: (R_, B_, R_, B_), 1 << 17: (R_, B_, R_, B_), (1 << 17) + 1: (R_, R_, R_, B_),
           1 << 18: (R_, R_, R_, B_), (1 << 18) + 1: (R_, R_, R_, R_), 1 << 20: (R_, R_, R_, R_), (1 << 20) + 1: (R_, R_, N_, N_),
           1 << 21: (R_, R_, N_, N_), (1 << 21) + 1: (R_, N_, N_, N_), 1 << 23: (R_, N_, N_, N_), (1 << 23) + 1: (N_, N_, N_, N_),
           1 << 31: (N_, N_, N_, N_)}


def test_widths():
    assert set(er.WIDTHS) == set(NATURAL) and len(er.WIDTHS) == 18
    assert er.TOP == 1 << 31 and er.SCALE_BELOW == 1 << 26


@pytest.mark.parametrize("ncol", er.WIDTHS)
def test_records(ncol):
    c = er.width_case(ncol)
    p1, p4, p8h, p8f = NATURAL[ncol]
    natural = {("k_hash", 1024): p1, ("k_few", 1024): p1, ("k_hash", 4096): p4, ("k_few", 4096): p4, ("k_hash", 8192): p8h, ("k_few", 8192): p8f}
    lo, hi = tp.row_tuples(c.A)
    blen = np.bincount(c.B.idx0, minlength=c.B.shape[0])
    assert len(c.rec) == c.A.shape[0] <= 48 and c.B.nnz <= 40000 and c.B.shape[1] == ncol
    for i, r in enumerate(c.rec):
        assert r.L == hi[i] - lo[i] and r.products == blen[c.A.idx1[lo[i]:hi[i]]].sum()
        assert 64 < r.products <= 4096 and r.T == er.table_class(r.products), "every row of the catalogue is a mid row"
        assert r.kernel == ("k_few" if r.L <= 8 else "k_hash") and r.path == natural[(r.kernel, r.T)]
        assert r.outputs <= c.hit[i] <= min(r.products, ncol, r.T // 2)
    # different rows of a kernel, different output counts (a narrow matrix leaves no choice: most rows fill it)
    for kern in ("k_few", "k_hash"):
        outs = [r.outputs for r in c.rec if r.kernel == kern]
        assert len(set(outs)) == len(outs) or ncol < 4096
    # both ends of the column range in every row
    for i in range(len(c.rec)):
        held = np.unique(c.B.idx1[np.isin(c.B.idx0, c.A.idx1[lo[i]:hi[i]])])
        assert held[0] == 0 and held[-1] == ncol - 1 and (ncol < 4 or (held[1] == 1 and held[-2] == ncol - 2))
    n = c.names
    if ncol >= 4096:
        # the rows by name: one A tuple at the class edges, tables filled to T / 2 in either kernel, sums, cancellations
        assert [c.rec[n[k]][:3] for k in ("lo1024", "lo4096", "lo8192")] == [(1, 65, 65), (1, 513, 513), (1, 2049, 2049)]
        for T in (1024, 4096, 8192):
            assert c.rec[n["full%d_few" % T]] == Rec(1, T // 2, T // 2, "k_few", T, natural[("k_few", T)])
            assert c.rec[n["full%d_hash" % T]] == Rec(9, T // 2, T // 2, "k_hash", T, natural[("k_hash", T)])
            assert c.hit[n["full%d_few" % T]] == c.hit[n["full%d_hash" % T]] == T // 2
            r = c.rec[n["few_max%d" % T]]
            assert r.L == 8 and r.kernel == "k_few" and r.T == T and r.outputs == c.hit[n["few_max%d" % T]] < r.products
        assert c.rec[n["repeat"]][:3] == (3, 300, 100) and c.hit[n["repeat"]] == 100
        assert c.rec[n["cancel_few"]][:2] == (4, 300) and c.hit[n["cancel_few"]] == 150 and c.rec[n["cancel_few"]].outputs == 147
        assert c.rec[n["cancel_hash"]][:2] == (12, 1020) and c.hit[n["cancel_hash"]] == 170 and c.rec[n["cancel_hash"]].outputs == 167
        # the special columns of the widest layout are there
        full = c.B.idx1[np.isin(c.B.idx0, c.A.idx1[lo[n["full8192_few"]]:hi[n["full8192_few"]]])]
        sp = [x for x in er.ends(ncol) + er.bitmap_edges(ncol) + er.bit_pairs(ncol) if 0 <= x < ncol]
        assert np.all(np.isin(sp, full))
        top = 1 << (c.colbits - 1)
        assert {63, 64, 255, 256, ((ncol - 1) >> 6) << 6, ncol - 1} <= set(sp) and any((x ^ top) in sp for x in sp)
        assert ncol <= (1 << 16) or {(1 << 15) - 3, (1 << 16) - 3} <= set(sp)
        assert ncol < (1 << 31) or {(1 << 30) - 3, (1 << 31) - 3, (1 << 31) - 1} <= set(sp)
    if ncol == 1:
        assert [r[:3] for r in c.rec] == [(65, 65, 1), (512, 512, 1), (513, 513, 1), (2048, 2048, 1), (2049, 2049, 1), (4096, 4096, 1),
                                          (70, 70, 1), (132, 66, 0)]
    # the planned cancellations: the middle columns of the row's range are not in the product
    for name in ("cancel_few", "cancel_hash"):
        if name not in n:
            assert ncol <= 2                                        # (one shape there: the row is taken once)
            continue
        i = n[name]
        held = np.unique(c.B.idx1[np.isin(c.B.idx0, c.A.idx1[lo[i]:hi[i]])])
        out = c.want[1][c.want[0] == i]
        gone = held[max(0, held.size // 2 - 1):held.size // 2 + 2]
        assert not np.any(np.isin(gone, out)) and (held.size < 8 or (out[0] == 0 and out[-1] == ncol - 1))


FEASIBLE = ([("k_hash", 1024, p) for p in (B_, R_, N_)] + [("k_hash", 4096, p) for p in (B_, R_, N_)] + [("k_hash", 8192, p) for p in (R_, N_)]
            + [("k_few", T, p) for T in (1024, 4096, 8192) for p in (B_, R_, N_)])


def test_coverage_of_the_mid_rows():
    """Every feasible (kernel, T, ordering) is reached with no knob set, on both sides of its thresholds; with every mid
    row on k_hash and under the knob's settings as well; the occupied list is full (position field at its largest) in
    every kernel and table, and at each table's last radix width with the top column present (a key of 32 one-bits'
    width)."""
    cases = [er.width_case(w) for w in er.WIDTHS]
    reached = set().union(*[c.paths() for c in cases])
    assert reached == set(FEASIBLE) and len(FEASIBLE) == 17
    assert set().union(*[c.paths(few_max=-1) for c in cases]) == {f for f in FEASIBLE if f[0] == "k_hash"}
    assert set().union(*[c.paths(knob=1) for c in cases]) == {f for f in FEASIBLE if f[2] != BITMAP}
    assert set().union(*[c.paths(knob=2) for c in cases]) == {f for f in FEASIBLE if f[2] == BITONIC}
    by_bits = {c.colbits: c for c in cases}
    for (kern, T), (bm, rx) in TABLE.items():
        if kern == "tiles" or T == 3072:
            continue
        # both sides of each threshold, at 2^k against 2^k + 1 columns
        for edge in ([bm] if bm else []) + [rx]:
            a, b = er.width_case(1 << edge), er.width_case((1 << edge) + 1)
            assert (a.colbits, b.colbits) == (edge, edge + 1)
            assert {p for k, t, p in a.paths() if (k, t) == (kern, T)} != {p for k, t, p in b.paths() if (k, t) == (kern, T)}
        c = by_bits[rx]
        full = [i for i, r in enumerate(c.rec) if (r.kernel, r.T, r.path) == (kern, T, RADIX) and c.hit[i] == T // 2]
        assert full and all(c.want[1][c.want[0] == i][-1] == c.ncol - 1 for i in full), (kern, T)
    for c in cases:
        if c.ncol >= 4096:
            assert {(r.kernel, r.T) for i, r in enumerate(c.rec) if c.hit[i] == r.T // 2} == {(k, T) for k in ("k_hash", "k_few") for T in (1024, 4096, 8192)}
        assert c.few_rows() == sum(1 for r in c.rec if r.L <= 8) and c.few_rows(-1) == 0 and c.few_rows(0, True) == 0
    top = er.width_case(er.TOP)
    assert top.paths() == {f for f in FEASIBLE if f[2] == BITONIC} and top.want[1].max() == (1 << 31) - 1


def _rss_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


@pytest.mark.parametrize("ncol", er.WIDTHS)
def test_oracle_gives_the_constructions_tuples(ncol):
    """The oracle's product equals the sums the builder itself formed, bit for bit and in order; per row the recorded
    output count.  At 2^31 columns: well under a second, and no memory by the column (2^31 bytes would be 2048 MB)."""
    c = er.width_case(ncol)
    before, dt = _rss_mb(), []
    for rep in range(3):                                            # (the quickest of three: a busy host is not the oracle's doing)
        t0 = time.perf_counter()
        wi, wj, wv = er.orc.multiply(c.A, c.B, rowwise=True, nthreads=1)[:3]
        dt.append(time.perf_counter() - t0)
    dt, grown = min(dt), _rss_mb() - before
    assert np.array_equal(wi, c.want[0]) and np.array_equal(wj, c.want[1]) and np.array_equal(wv.view(np.int64), c.want[2].view(np.int64))
    assert np.array_equal(np.bincount(wi, minlength=len(c.rec)), [r.outputs for r in c.rec])
    assert np.all(wv == np.round(wv)) and np.all(wv != 0)
    assert dt < 0.5 and grown < 256, "oracle at %d columns: %.2f s, %+.0f MB" % (ncol, dt, grown)
    got = er.oracle_tuples(c)
    assert np.array_equal(got[1], wj) and np.array_equal(got[2].view(np.int64), wv.view(np.int64))


@pytest.mark.parametrize("ncol", [w for w in er.WIDTHS if w < er.SCALE_BELOW])
def test_scaled_cases_stay_exact(ncol):
    """C, scalei and scalek are powers of two (sums stay integers over a power of two); scalek drops a fifth of the columns,
    scalei rows."""
    c = er.width_case(ncol)
    plain, (wi, wj, wv) = er.oracle_tuples(c), er.oracle_tuples(c, scaled=True)
    assert np.all(wv * 4 == np.round(wv * 4)) and 0 < wv.size < plain[2].size
    kw = er.scales(c)
    assert not np.any(np.isin(wi, [3, 4])) and np.all(np.isin(wj, kw["scalek"].idx))


# ---- the heavy rows' cells

@pytest.mark.parametrize("T,W,where", er.WINDOW_CASES)
def test_window_cells_are_cut_as_planned(T, W, where):
    p = er.window_case(T, W, where)
    spans = er.spans_of(T, W)
    assert p.A.shape[0] == len(spans) and p.B.shape[1] == 2048 * W and p.B.nnz <= 40000
    klass = {"hash1024": (1, 512), "hash3072": (513, 1536), "hash4096": (1537, 2048), "hash8192": (2049, 4096), "tile": (1537, 2048)}[p.kind]
    for scheme in p.schemes:
        cells = er.planned_cells(p, scheme, p.kind)
        cut = p.cut(scheme)
        assert cut.rows_heavy == len(spans) == cut.cells_dense and len(cells) == len(spans)
        assert (cut.tile_cells, cut.cells_windowed) == ((len(spans), 0) if T == "tiles" else (0, len(spans)))
        for span, (wa, wb, prods, colbase, cb, path), r in zip(spans, cells, range(len(spans))):
            assert wb - wa == span and wa == (0 if where == "low" else 2048 - span) and klass[0] <= prods <= klass[1]
            st = tp.cell_stats(p.A, p.B, r, wa, wb, W)
            assert st["products"] == prods and st["distinct"] < prods
            assert st["columns"][0] == colbase and st["columns"][-1] == wb * W - 1
            assert {colbase + x for x in (1, 63, 64, 255, 256)} <= set(st["columns"]) and wb * W - 64 in st["columns"]
            assert cb == {8192: 13, 16384: 14}[W] + {1: 0, 2: 1, 3: 2, 4: 2, 5: 3, 9: 4}[span]
            assert path == (RADIX if T == 8192 or cb > TABLE[("k_hash", T) if T != "tiles" else ("tiles", 4096)][0] else BITMAP)
        if T == 3072:
            assert all(tp.cell_stats(p.A, p.B, r, wa, wb, W)["distinct"] > 1024 for r, (wa, wb, *_) in enumerate(cells))
        assert len({tp.cell_stats(p.A, p.B, r, c[0], c[1], W)["distinct"] for r, c in enumerate(cells)}) == len(cells)
    if where == "high":
        assert p.B.idx1.max() == 2048 * W - 1


def test_coverage_of_the_window_cells():
    """Every windowed table and the hash tiles reach the bitmap rank and the radix sort (8192 with 512 threads: the radix
    sort alone) away from column 0, the last bitmap width and the first radix width of each among them; forced, all
    reach the bitonic network."""
    reached, edge = set(), set()
    for T, W, where in er.WINDOW_CASES:
        p = er.window_case(T, W, where)
        for scheme in p.schemes:
            for wa, wb, prods, colbase, cb, path in er.planned_cells(p, scheme, p.kind):
                reached.add((p.kind, path, colbase != 0))
                edge.add((p.kind, cb))
    want = {(k, path, far) for k in ("hash1024", "hash3072", "hash4096", "tile") for path in (BITMAP, RADIX) for far in (False, True)}
    want |= {("hash8192", RADIX, False), ("hash8192", RADIX, True)}
    assert reached == want
    assert {("hash1024", 15), ("hash1024", 16), ("hash3072", 16), ("hash3072", 17), ("hash4096", 17), ("hash4096", 18), ("tile", 17), ("tile", 18)} <= edge
