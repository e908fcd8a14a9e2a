"""Measure spsamd_reduce (row and column reductions of op(A) into a vector) against the only way the library offered before:
spsamd_multiply_dense with a device vector of ones, one right-hand side, into a zeroed Y, on the same operand.

    python scripts/bench_reduce.py [--only poisson,laplace,galerkin,rmat,raw,square] [--reps 7] [--warmup 2]

Workloads (device generators; trusted sort0 = 0 device operands unless noted):
  poisson      Poisson 4096^2
  laplace      Laplace 256^3
  galerkin     R A R^T on 256^3, read in place from the context's output set
  rmat20       R-MAT scale 20, consolidated
  rmat20_rawT  the same matrix raw (unsorted, duplicates) under 'T': the consolidation by columns is part of the call.  No
               baseline: multiply_dense does not consolidate, so its sums over the raw tuples are other numbers
  rmat20_prepT the same matrix prepared for 'T' (spsamd_operand_prepare), both sides reading the handle
  square       A A of R-MAT scale 16, read in place
For each: SUM, MAX_ABS and COUNT, dense and sparse form, into device tensors.  The baseline (multiply_dense) stands beside
SUM dense only -- its Y is compared with reduce's output bit for bit first -- and the gate is that reduce(SUM, dense) is the
faster of the two on every workload.
Times: HIP events on the context's stream, median of --reps after --warmup, reduce and baseline alternating.
Byte model at 8 TB/s: 8 B per tuple (COUNT: none) + 4 B per row of row pointer + 12 B per output entry (dense: 8 B per row):
reported, not gated.  For R-MAT 20 the longest row is also reduced alone (an operand of that one row): its length and the
call's numeric time give the per-tuple cost of one chain.
One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi

OPS = (("sum", capi.REDUCE_SUM), ("max_abs", capi.REDUCE_MAX_ABS), ("count", capi.REDUCE_COUNT))


def main():
    a = ob.parser("poisson,laplace,galerkin,rmat,raw,square").parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def measure(name, A, transpose='.', before=None, baseline=True):
        nrow = int(A.shape1 if transpose == 'T' else A.shape0)
        ncol = int(A.shape0 if transpose == 'T' else A.shape1)
        val = torch.empty(nrow, dtype=torch.float64, device=dev)
        idx = torch.empty(nrow, dtype=torch.int32, device=dev)
        ones = torch.ones(ncol, dtype=torch.float64, device=dev)
        Y = torch.zeros(nrow, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        res = capi.Result()

        def base():
            with torch.cuda.stream(stream):
                Y.zero_()
            return ctx.multiply_dense(A, ones, Y, transpose=transpose)

        for opname, op in OPS:
            for form in ("dense", "sparse"):
                def call():
                    return ctx.reduce(A, op, transpose=transpose, dense=form == "dense", out=val if form == "dense" else (idx, val),
                                      result=res)
                gated = baseline and op == capi.REDUCE_SUM and form == "dense"
                if gated:
                    (s, ms_s), (b, ms_b), cnt, _ = ob.time_pair(stream, call, base, a.reps, a.warmup, before)
                    call()
                    torch.cuda.synchronize()
                    same = torch.equal(val.view(torch.int64), Y.view(torch.int64))
                else:
                    if before:
                        before()
                    s, ms_s = ob.time_call(stream, call, a.reps, a.warmup)
                    cnt = call()
                n = int(res.nnz_a)
                by = (0.0 if op == capi.REDUCE_COUNT else 8.0 * n) + 4.0 * nrow + (8.0 * nrow if form == "dense" else 12.0 * cnt)
                r = {"workload": name, "op": opname, "form": form, "impl": "spsamd_reduce", **ob.times(s, ms_s), "tuples": n, "rows": nrow,
                     "entries": int(cnt), "model_bytes": by, "model_ms_at_8TBps": round(by / ob.PEAK * 1e3, 4),
                     "of_model": round(by / ob.PEAK * 1e3 / s, 4), "ms_consolidate": round(res.ms_consolidate, 4),
                     "ms_numeric": round(res.ms_numeric, 4), "rows_short": int(res.rows_light), "rows_long": int(res.rows_heavy),
                     "tuples_long": int(res.tuples_heavy)}
                if gated:
                    r.update({"ratio_to_multiply_dense": round(s / b, 4), "same_bits": bool(same)})
                ob.record(rows, r)
                if gated:
                    ob.record(rows, {"workload": name, "op": opname, "form": form, "impl": "multiply_dense", **ob.times(b, ms_b)})

    def longest_row(name, A, t):
        """The longest row of a consolidated operand alone: its length and the time of the call that folds it (one chain)."""
        counts = torch.bincount(t[0], minlength=int(A.shape0))
        r = int(counts.argmax().item())
        n = int(counts[r].item())
        keep = t[0] == r
        one = tuple(x[keep].contiguous() for x in t)
        torch.cuda.synchronize()
        B = capi.device_coo(*ob.ptrs(one), n, (int(A.shape0), int(A.shape1)), 0)
        val = torch.empty(int(A.shape0), dtype=torch.float64, device=dev)
        res = capi.Result()
        s, ms = ob.time_call(stream, lambda: ctx.reduce(B, capi.REDUCE_SUM, dense=True, out=val, result=res), a.reps, a.warmup)
        ob.record(rows, {"workload": name + "_longest_row", "op": "sum", "form": "dense", "impl": "spsamd_reduce", **ob.times(s, ms),
                         "tuples": n, "ms_numeric": round(res.ms_numeric, 4), "ns_per_tuple": round(res.ms_numeric * 1e6 / n, 3)})

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        measure("poisson", A)

    def laplace():
        A, t = ob.laplace3d(ctx, dev)
        measure("laplace", A)

    def rmat20():
        R, raw = ob.rmat(ctx, dev, 20)
        if "rmat" in only:
            A, t = ob.consolidated(ctx, dev, R)
            measure("rmat20", A)
            longest_row("rmat20", A, t)
        if "raw" in only:
            measure("rmat20_rawT", R, 'T', baseline=False)
            P = capi.Operand(ctx, R, 'T', capi.AS_A)
            measure("rmat20_prepT", P.coo, 'T')
            P.close()

    def galerkin():
        (A, ta), (R, tr) = ob.laplace3d(ctx, dev), ob.aggregation3d(ctx, dev)
        G = ob.galerkin(ctx, A, R)
        measure("galerkin", capi.result_operand(G))

    def square():
        R, raw = ob.rmat(ctx, dev, 16)
        P = ob.square(ctx, R)
        measure("square", capi.result_operand(P))

    ob.run(only, [("poisson", poisson), ("laplace", laplace), ("rmat raw", rmat20), ("galerkin", galerkin), ("square", square)])
    ob.table(rows, [("workload", -20, "%s", "workload"), ("op", -8, "%s", "op"), ("form", -7, "%s", "form"), ("impl", -15, "%s", "impl"),
                    ("ms", 10, "%.3f", "ms"), ("model ms", 10, "%.3f", "model_ms_at_8TBps"), ("of model", 9, "%.1f%%", ob.pct("of_model")),
                    ("ratio", 8, "%.3f", "ratio_to_multiply_dense"), ("same", 6, "%s", "same_bits"),
                    ("ns/tuple", 9, "%.2f", "ns_per_tuple")])
    ob.gate("reduce(SUM, dense) faster than multiply_dense with ones, same bits",
            [r["workload"] for r in rows if "ratio_to_multiply_dense" in r and (r["ratio_to_multiply_dense"] >= 1 or not r["same_bits"])])
    ctx.close()


if __name__ == "__main__":
    main()
