"""Measure spsamd_factor_ilu0 (ILU(0) by level schedule).

    python scripts/bench_factor.py [--only poisson,laplace,rmat,tridiag] [--reps 5] [--warmup 1] [--rmat-scale 16]
                                   [--tridiag-log2 20] [--sweep fuse|serial|lds] [--one]

Workloads (device generators):
  poisson  the 5-point Poisson matrix on 4096^2 points: 8191 levels of at most 4096 rows, every row serial-class
  laplace  the 7-point Laplacian on 256^3 points: 766 wide levels
  rmat     R-MAT at --rmat-scale, 16 edges per vertex, A + A^T (spsamd_add) plus a diagonal of 2^scale: rows of every class in
           one level; its lookups grow like its wedges, so the scale and the lookups are part of the record
  tridiag  a tridiagonal matrix of 2^tridiag-log2 rows: n levels of one row, one fused launch
For each:
  prepared / default   a prepared handle: the schedule is analysed by the first call and kept
  prepared / path1     the same under factor_path = 1: launches per level -- an ablation of this code, not a bar
  raw / default        the device operand as it is: analysed by every call
  solve_tri            the reference point: spsamd_solve_tri(LOWER, NONUNIT) on the same prepared handle with one right-hand
                       side.  Both calls are bound by levels x (launch or barrier); `ratio` is factor ms / solve ms.
Nothing outside the project runs here as a baseline.
--sweep fuse: factor_fuse_rows over the powers of two from 64 to 16384 on poisson and laplace; serial: factor_serial_work over
8 .. 4096 on laplace and rmat; lds: factor_lds_row over 128 .. 4096 on rmat.  All prepared.
--one: a single prepared factorisation of rmat after the analysis, for a kernel trace.
Times: HIP events on the context's stream, median of --reps after --warmup.
Byte model at 8 TB/s: 40 B per tuple (its keys and value copied into the result: 16 B read, 16 B written, and the column read
again by its row) + 12 B per lookup (a column and a value of the named row) + 16 B per update (the value read and written):
reported, not gated -- a level schedule is bound by its levels' latency wherever the levels are thin, and a skewed row by
its own serial chain of k.
One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi


def main():
    ap = ob.parser("poisson,laplace,rmat,tridiag", reps=5, warmup=1)
    ap.add_argument("--rmat-scale", type=int, default=16)
    ap.add_argument("--tridiag-log2", type=int, default=20)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--one", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def factor(op):
        return ctx.factor_ilu0(op, stats=True)

    def measure(name, A, extra=None):
        n = int(A.shape0)
        P = capi.Operand(ctx, A, '.', capi.AS_A)
        _, first = factor(P.coo)
        by = 40.0 * int(A.nnz) + 12.0 * first.lookups + 16.0 * first.updates
        base = dict({"workload": name, "rows": n, "tuples": int(A.nnz), "levels": int(first.levels), "max_level_rows": int(first.max_level_rows),
                     "lookups": int(first.lookups), "updates": int(first.updates), "zero_pivot": int(first.zero_pivot),
                     "rows_serial": int(first.rows_serial), "rows_wave": int(first.rows_wave), "rows_block": int(first.rows_block),
                     "model_bytes": by, "model_ms_at_8TBps": round(by / ob.PEAK * 1e3, 4)}, **(extra or {}))
        B = torch.rand((n, 1), dtype=torch.float64, device=dev) + 0.5
        X = torch.empty_like(B)
        torch.cuda.synchronize()
        ctx.solve_tri(P.coo, B, X=X)
        s_solve, ms_solve = ob.time_call(stream, lambda: ctx.solve_tri(P.coo, B, X=X), a.reps, a.warmup)
        _, sst = ctx.solve_tri(P.coo, B, X=X, stats=True)
        ob.record(rows, dict(base, operand="prepared", path="solve_tri", **ob.times(s_solve, ms_solve), launches=int(sst.launches),
                             fused_levels=int(sst.fused_levels)))
        for mode, op, path in (("prepared", P.coo, 0), ("prepared", P.coo, 1), ("raw", A, 0)):
            ctx.set_tuning("factor_path", path)
            try:
                s, ms = ob.time_call(stream, lambda: ctx.factor_ilu0(op), a.reps, a.warmup)
                _, st = factor(op)
            finally:
                ctx.set_tuning("factor_path", 0)
            ob.record(rows, dict(base, operand=mode, path="path1" if path else "default", **ob.times(s, ms), launches=int(st.launches),
                                 fused_levels=int(st.fused_levels), ms_analysis=round(st.ms_analysis, 4), ms_factor=round(st.ms_factor, 4),
                                 analysis_reused=int(st.analysis_reused), ratio=round(s / s_solve, 3), of_model=round(by / ob.PEAK * 1e3 / s, 5)))
        P.close()

    def sweep(name, A, knob, values):
        P = capi.Operand(ctx, A, '.', capi.AS_A)
        factor(P.coo)
        for v in values:
            ctx.set_tuning(knob, v)
            try:
                s, ms = ob.time_call(stream, lambda: ctx.factor_ilu0(P.coo), a.reps, a.warmup)
                _, st = factor(P.coo)
            finally:
                ctx.set_tuning(knob, 0)
            ob.record(rows, {"workload": name + "_sweep", knob: v, "operand": "prepared", "path": "%s %d" % (knob, v), **ob.times(s, ms),
                             "launches": int(st.launches), "fused_levels": int(st.fused_levels), "levels": int(st.levels),
                             "rows_serial": int(st.rows_serial), "rows_wave": int(st.rows_wave), "rows_block": int(st.rows_block),
                             "ms_factor": round(st.ms_factor, 4)})
        P.close()

    def run_or_sweep(name, A, extra=None):
        pows = lambda lo, hi: [lo << k for k in range((hi // lo).bit_length())]      # noqa: E731
        if a.sweep == "fuse" and name in ("poisson", "laplace"):
            sweep(name, A, "factor_fuse_rows", pows(64, 16384))
        elif a.sweep == "serial" and name != "poisson" and not name.startswith("tridiag"):
            sweep(name, A, "factor_serial_work", pows(8, 4096))
        elif a.sweep == "lds" and name.startswith("rmat"):
            sweep(name, A, "factor_lds_row", pows(128, 4096))
        elif not a.sweep:
            measure(name, A, extra)

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        run_or_sweep("poisson", A)

    def laplace():
        A, t = ob.laplace3d(ctx, dev)
        run_or_sweep("laplace", A)

    def rmat():
        scale = a.rmat_scale
        n = 1 << scale
        R, raw = ob.rmat(ctx, dev, scale)
        sym = ctx.add(R, R, tB='T')
        i = torch.arange(n, dtype=torch.int32, device=dev)
        d = torch.full((n,), float(n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        D = capi.device_coo(i.data_ptr(), i.data_ptr(), d.data_ptr(), n, (n, n), 0)
        t = ob.copy_out(ctx, ctx.add(capi.result_operand(sym), D), dev)
        A = capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0)
        if a.one:
            P = capi.Operand(ctx, A, '.', capi.AS_A)
            for _ in range(2):
                _, st = factor(P.coo)
            ob.record(rows, {"workload": "rmat%d_one" % scale, "operand": "prepared", "path": "default", "ms": round(st.ms_factor, 4),
                             "launches": int(st.launches), "fused_levels": int(st.fused_levels), "levels": int(st.levels)})
            P.close()
            return
        run_or_sweep("rmat%d_sym" % scale, A, {"rmat_scale": scale})

    def tridiag():
        n = 1 << a.tridiag_log2
        i = torch.arange(n, dtype=torch.int32, device=dev)
        r, c = torch.cat([i, i[1:], i[:-1]]), torch.cat([i, i[1:] - 1, i[:-1] + 1])
        v = torch.cat([torch.full((n,), 2.0, dtype=torch.float64, device=dev), torch.full((2 * n - 2,), -0.5, dtype=torch.float64, device=dev)])
        o = torch.argsort(r.long() * n + c.long())
        t = (r[o].contiguous(), c[o].contiguous(), v[o].contiguous())
        torch.cuda.synchronize()
        A = capi.device_coo(*ob.ptrs(t), 3 * n - 2, (n, n), 0)
        run_or_sweep("tridiag_2^%d" % a.tridiag_log2, A)

    ob.run(only, [("poisson", poisson), ("laplace", laplace), ("rmat", rmat), ("tridiag", tridiag)])
    ob.table(rows, [("workload", -16, "%s", "workload"), ("operand", -9, "%s", "operand"), ("path", -24, "%s", "path"),
                    ("ms", 11, "%.3f", "ms"), ("ratio", 7, "%.2f", "ratio"), ("analysis", 10, "%.3f", "ms_analysis"),
                    ("levels", 8, "%d", "levels"), ("launches", 9, "%d", "launches"), ("fused", 8, "%d", "fused_levels"),
                    ("lookups", 12, "%d", "lookups"), ("updates", 11, "%d", "updates"),
                    ("model ms", 9, "%.3f", "model_ms_at_8TBps"), ("of model", 9, "%.2f%%", ob.pct("of_model"))])
    ctx.close()


if __name__ == "__main__":
    main()
