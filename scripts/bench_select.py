"""Measure spsamd_select (keep op(A)'s tuples by position, size or row top-k) against what a user does without it: composed
torch calls over the same device arrays.

    python scripts/bench_select.py [--only poisson,rmat,raw,galerkin,square] [--reps 7] [--warmup 2]

Workloads (device generators; operands consolidated and handed in as sort0 = 0 device operands unless noted):
  poisson_tril     Poisson 4096^2, TRIL(-1)
  rmat20_*         R-MAT scale 20, consolidated: TRIL(-1), ABS_GE at the median magnitude, ROW_REL 0.25, ROW_TOPK 8 and 32
  rmat20_raw_tril  the same matrix raw (unsorted, duplicates): the consolidation is part of both sides
  galerkin_rowrel  R A R^T on 256^3, the product read in place from the context's output set, ROW_REL 0.25
  square_topk32    A A of R-MAT scale 16, read in place, ROW_TOPK 32
Baseline: tuple-wise and row-relative predicates -- a boolean mask (scatter_reduce amax over the rows for the row maximum)
and boolean indexing of the three arrays; top-k -- two stable sorts (by -|v|, then by row), a rank from the row pointer, the
mask, and a sort back to (row, col) order.  Its tuples are compared with spsamd_select's once per workload.
Times: HIP events on the context's stream, median of --reps after --warmup, select and baseline alternating.
Byte model: 16 B per tuple of S for every pass that reads it (tuple-wise: flag + compact = 2; ROW_REL: row maximum, flag,
compact = 3; ROW_TOPK: row pointer, selection, compact = 3) + 16 B per kept tuple, against 8 TB/s: reported, not gated.
One JSON line per measurement, then a table with the ratio select / baseline (the gate: < 1 everywhere).
"""
import torch

import opbench as ob
from opbench import capi

PASSES = {capi.SELECT_TRIL: 2, capi.SELECT_ABS_GE: 2, capi.SELECT_ROW_REL: 3, capi.SELECT_ROW_TOPK: 3}


def torch_select(t, nrow, pred, ip, dp):
    """The composed-torch form of one predicate over (rows, cols, vals) sorted row-major."""
    r, c, v = t
    if pred == capi.SELECT_ROW_TOPK:
        n = r.numel()
        o1 = torch.sort(-v.abs(), stable=True).indices
        r1 = r[o1]
        o2 = torch.sort(r1, stable=True).indices
        perm, rs = o1[o2], r1[o2].long()
        counts = torch.bincount(r, minlength=nrow)
        start = torch.cumsum(counts, 0) - counts
        rank = torch.arange(n, device=r.device) - start[rs]
        kept = torch.sort(perm[rank < ip]).values
        return r[kept], c[kept], v[kept]
    if pred == capi.SELECT_TRIL:
        keep = (c - r) <= ip
    elif pred == capi.SELECT_ABS_GE:
        keep = v.abs() >= dp
    else:
        a, rl = v.abs(), r.long()
        m = torch.zeros(nrow, dtype=torch.float64, device=r.device).scatter_reduce(0, rl, a, "amax", include_self=True)
        keep = a >= dp * m[rl]
    return r[keep], c[keep], v[keep]


def main():
    a = ob.parser("poisson,rmat,raw,galerkin,square").parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def measure(name, A, t, nrow, pred, ip=0, dp=0.0, baseline=None):
        """A: the operand of spsamd_select; t: the same tuples as torch tensors for the baseline."""
        def sel():
            return ctx.select(A, pred, iparam=ip, dparam=dp)

        def base():
            with torch.cuda.stream(stream):
                return baseline() if baseline else torch_select(t, nrow, pred, ip, dp)
        (s, ms_s), (b, ms_b), res, out = ob.time_pair(stream, sel, base, a.reps, a.warmup)
        got = ob.copy_out(ctx, sel(), dev)           # (a baseline that consolidates writes the output set: select once more)
        same = ob.same(got, out)
        nin, nout = int(res.nnz_a), int(res.nnz)
        by = 16.0 * nin * PASSES[pred] + 16.0 * nout
        for impl, med, ms in (("spsamd_select", s, ms_s), ("torch", b, ms_b)):
            r = {"workload": name, "impl": impl, **ob.times(med, ms), "tuples_in": nin,
                 "tuples_out": nout, "same_tuples": bool(same)}
            if impl == "spsamd_select":
                r.update({"passes": PASSES[pred], "model_bytes": by, "model_ms_at_8TBps": round(by / ob.PEAK * 1e3, 4),
                          "of_model": round(by / ob.PEAK * 1e3 / med, 4), "ratio_to_torch": round(s / b, 4),
                          "rows_light": int(res.rows_light), "rows_mid": int(res.rows_mid), "rows_heavy": int(res.rows_heavy)})
            ob.record(rows, r)

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        measure("poisson_tril", A, t, int(A.shape0), capi.SELECT_TRIL, ip=-1)

    def rmat20():
        R, raw = ob.rmat(ctx, dev, 20)
        A, t = ob.consolidated(ctx, dev, R)
        n = int(A.shape0)
        if "rmat" in only:
            med = float(t[2].abs().median().item())
            measure("rmat20_tril", A, t, n, capi.SELECT_TRIL, ip=-1)
            measure("rmat20_absge", A, t, n, capi.SELECT_ABS_GE, dp=med)
            measure("rmat20_rowrel", A, t, n, capi.SELECT_ROW_REL, dp=0.25)
            measure("rmat20_topk8", A, t, n, capi.SELECT_ROW_TOPK, ip=8)
            measure("rmat20_topk32", A, t, n, capi.SELECT_ROW_TOPK, ip=32)
        if "raw" in only:
            def raw_base():
                c = ob.copy_out(ctx, ctx.consolidate(R, 0), dev)
                return torch_select(c, n, capi.SELECT_TRIL, -1, 0.0)
            measure("rmat20_raw_tril", R, None, n, capi.SELECT_TRIL, ip=-1, baseline=raw_base)

    def galerkin():
        (A, ta), (R, tr) = ob.laplace3d(ctx, dev), ob.aggregation3d(ctx, dev)
        G = ob.galerkin(ctx, A, R)
        t = ob.copy_out(ctx, G, dev)
        measure("galerkin_rowrel", capi.result_operand(G), t, int(R.shape0), capi.SELECT_ROW_REL, dp=0.25)

    def square():
        R, raw = ob.rmat(ctx, dev, 16)
        P = ob.square(ctx, R)
        t = ob.copy_out(ctx, P, dev)
        measure("square_topk32", capi.result_operand(P), t, int(R.shape0), capi.SELECT_ROW_TOPK, ip=32)

    ob.run(only, [("poisson", poisson), ("rmat raw", rmat20), ("galerkin", galerkin), ("square", square)])
    ob.table(rows, [("workload", -16, "%s", "workload"), ("impl", -14, "%s", "impl"), ("ms", 10, "%.3f", "ms"),
                    ("model ms", 10, "%.3f", "model_ms_at_8TBps"), ("of model", 9, "%.1f%%", ob.pct("of_model")),
                    ("ratio", 8, "%.3f", "ratio_to_torch"), ("same", 6, "%s", lambda r: r["same_tuples"] if "passes" in r else None)])
    ob.gate("select faster than torch, same tuples",
            [r["workload"] for r in rows if r["impl"] == "spsamd_select" and (r["ratio_to_torch"] >= 1 or not r["same_tuples"])])
    ctx.close()


if __name__ == "__main__":
    main()
