"""Measure spsamd_solve_tri (sparse triangular solves by level schedule).

    python scripts/bench_solve.py [--only poisson,laplace,rmat,chain] [--reps 7] [--warmup 2] [--nrhs 1,8,64]
                                  [--chain-log2 20] [--chain-reps 3] [--sweep] [--one] [--torch-ref]

Workloads (device generators):
  poisson  the whole Poisson 4096^2 matrix under LOWER (its tril by the fill-mode rule): 8191 levels of at most 4096 rows
  laplace  the whole 7-point Laplacian on 256^3 under LOWER: 766 wide levels
  rmat     R-MAT scale 20, consolidated, under LOWER | UNIT
  chain    a bidiagonal matrix, n = 2^chain-log2: n levels of one row (--chain-reps repetitions after one warm-up)
For each and each nrhs, B and X device arrays, out of place:
  prepared / default   a prepared handle: the schedule is analysed by the first solve and kept
  prepared / path1     the same under solve_path = 1: one launch per level -- an ablation of this code, not a bar
  raw / default        the device operand as it is: analysed by every call (nrhs 1 only for the chain)
and once per workload the analysis time (stats.ms_analysis of a raw call) beside one spsamd_consolidate of the operand.
--sweep: solve_fuse_rows over the powers of two from 64 to 16384 on poisson, prepared.
--one: a single prepared solve of poisson at nrhs 8 after the analysis, for a kernel trace.
Times: HIP events on the context's stream, median of --reps after --warmup.
Byte model at 8 TB/s: 12 B per used tuple + 8 nrhs per dependency (X read) + 16 nrhs per row (B read, X written): reported,
not gated -- a level schedule is bound by its levels' latency, not by bytes, wherever the levels are thin.
--torch-ref: torch has no sparse triangular solve whose summation order is fixed; torch.triangular_solve on a sparse CSR
matrix is tried on poisson at nrhs 1 and reported if this build has it -- a reference point, not a bar.
One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi


def main():
    ap = ob.parser("poisson,laplace,rmat,chain")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--chain-log2", type=int, default=20)
    ap.add_argument("--chain-reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--torch-ref", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")
    nrhs_list = [int(x) for x in a.nrhs.split(",")]

    def one_call(A, B, X, uplo, diag):
        _, st = ctx.solve_tri(A, B, uplo, diag, X=X, stats=True)
        return st

    def measure(name, A, uplo=capi.TRI_LOWER, diag=capi.DIAG_NONUNIT, reps=None, warmup=None, raw_nrhs=None):
        reps = a.reps if reps is None else reps
        warmup = a.warmup if warmup is None else warmup
        n = int(A.shape0)
        ms_c, _ = ob.time_call(stream, lambda: ctx.consolidate(A, 0), min(reps, 3), 1)
        P = capi.Operand(ctx, A, '.', capi.AS_A)
        for nrhs in nrhs_list:
            B = torch.rand((n, nrhs), dtype=torch.float64, device=dev) + 0.5
            X = torch.empty_like(B)
            torch.cuda.synchronize()
            first = one_call(P.coo, B, X, uplo, diag)                   # (analyses on the first nrhs, reuses after)
            deps = int(first.tuples_used) - (0 if diag == capi.DIAG_UNIT else n)
            by = 12.0 * first.tuples_used + 8.0 * nrhs * deps + 16.0 * nrhs * n
            base = {"workload": name, "nrhs": nrhs, "rows": n, "levels": int(first.levels), "max_level_rows": int(first.max_level_rows),
                    "tuples_used": int(first.tuples_used), "model_bytes": by, "model_ms_at_8TBps": round(by / ob.PEAK * 1e3, 4)}
            for mode, op, path in (("prepared", P.coo, 0), ("prepared", P.coo, 1), ("raw", A, 0)):
                if mode == "raw" and raw_nrhs is not None and nrhs not in raw_nrhs:
                    continue
                ctx.set_tuning("solve_path", path)
                try:
                    s, ms = ob.time_call(stream, lambda: ctx.solve_tri(op, B, uplo, diag, X=X), reps, warmup)
                    st = one_call(op, B, X, uplo, diag)
                finally:
                    ctx.set_tuning("solve_path", 0)
                r = dict(base, operand=mode, path="path1" if path else "default", **ob.times(s, ms), launches=int(st.launches),
                         fused_levels=int(st.fused_levels), ms_analysis=round(st.ms_analysis, 4), ms_solve=round(st.ms_solve, 4),
                         analysis_reused=int(st.analysis_reused), of_model=round(by / ob.PEAK * 1e3 / s, 5))
                if mode == "raw":
                    r["ms_consolidate_call"] = round(ms_c, 4)
                ob.record(rows, r)
            del B, X
            torch.cuda.empty_cache()
        P.close()

    def sweep(A):
        n = int(A.shape0)
        P = capi.Operand(ctx, A, '.', capi.AS_A)
        for nrhs in (1, 8):
            B = torch.rand((n, nrhs), dtype=torch.float64, device=dev) + 0.5
            X = torch.empty_like(B)
            torch.cuda.synchronize()
            for fr in [64 << k for k in range(9)]:
                ctx.set_tuning("solve_fuse_rows", fr)
                try:
                    s, ms = ob.time_call(stream, lambda: ctx.solve_tri(P.coo, B, X=X), a.reps, a.warmup)
                    st = one_call(P.coo, B, X, capi.TRI_LOWER, capi.DIAG_NONUNIT)
                finally:
                    ctx.set_tuning("solve_fuse_rows", 0)
                ob.record(rows, {"workload": "poisson_sweep", "nrhs": nrhs, "solve_fuse_rows": fr, "operand": "prepared", "path": "fuse %d" % fr,
                                 **ob.times(s, ms), "launches": int(st.launches), "fused_levels": int(st.fused_levels), "levels": int(st.levels)})
        P.close()

    def torch_reference(t, n):
        try:
            keep = t[1] <= t[0]
            crow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            crow[1:] = torch.cumsum(torch.bincount(t[0][keep].long(), minlength=n), 0)
            M = torch.sparse_csr_tensor(crow, t[1][keep].long(), t[2][keep], size=(n, n))
            b = torch.rand((n, 1), dtype=torch.float64, device=dev) + 0.5
            fn = lambda: torch.triangular_solve(b, M, upper=False)      # noqa: E731
            fn()
            torch.cuda.synchronize()
            s, ms = ob.time_call(torch.cuda.current_stream(), fn, min(a.reps, 3), 1)
            ob.record(rows, {"workload": "poisson", "nrhs": 1, "operand": "torch CSR", "path": "triangular_solve", **ob.times(s, ms)})
        except Exception as e:                                          # this build has no sparse triangular solve
            ob.record(rows, {"workload": "poisson", "nrhs": 1, "operand": "torch CSR", "path": "triangular_solve",
                             "unavailable": "%s: %s" % (type(e).__name__, str(e)[:160])})

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        if a.one:
            n = int(A.shape0)
            P = capi.Operand(ctx, A, '.', capi.AS_A)
            B = torch.rand((n, 8), dtype=torch.float64, device=dev) + 0.5
            X = torch.empty_like(B)
            torch.cuda.synchronize()
            for _ in range(2):
                st = one_call(P.coo, B, X, capi.TRI_LOWER, capi.DIAG_NONUNIT)
            ob.record(rows, {"workload": "poisson_one", "nrhs": 8, "operand": "prepared", "path": "default", "ms": round(st.ms_solve, 4),
                             "launches": int(st.launches), "fused_levels": int(st.fused_levels), "levels": int(st.levels)})
            P.close()
            return
        if a.sweep:
            sweep(A)
            return
        if a.torch_ref:
            torch_reference(t, int(A.shape0))
            return
        measure("poisson", A)

    def laplace():
        A, t = ob.laplace3d(ctx, dev)
        measure("laplace", A)

    def rmat():
        R, raw = ob.rmat(ctx, dev, 20)
        A, t = ob.consolidated(ctx, dev, R)
        measure("rmat20_unit", A, diag=capi.DIAG_UNIT)

    def chain():
        n = 1 << a.chain_log2
        i = torch.arange(n, dtype=torch.int32, device=dev)
        t = (torch.cat([i, i[1:]]), torch.cat([i, i[1:] - 1]),
             torch.cat([torch.full((n,), 2.0, dtype=torch.float64, device=dev), torch.full((n - 1,), -0.5, dtype=torch.float64, device=dev)]))
        torch.cuda.synchronize()
        A = capi.device_coo(*ob.ptrs(t), 2 * n - 1, (n, n), -1)
        measure("chain_2^%d" % a.chain_log2, A, reps=a.chain_reps, warmup=1, raw_nrhs=(1,))

    ob.run(only, [("poisson", poisson), ("laplace", laplace), ("rmat", rmat), ("chain", chain)])
    ob.table(rows, [("workload", -14, "%s", "workload"), ("nrhs", 5, "%d", "nrhs"), ("operand", -10, "%s", "operand"), ("path", -16, "%s", "path"),
                    ("ms", 11, "%.3f", "ms"), ("analysis", 10, "%.3f", "ms_analysis"), ("consol.", 9, "%.3f", "ms_consolidate_call"),
                    ("levels", 9, "%d", "levels"), ("launches", 9, "%d", "launches"), ("fused", 9, "%d", "fused_levels"),
                    ("model ms", 9, "%.3f", "model_ms_at_8TBps"), ("of model", 9, "%.2f%%", ob.pct("of_model"))])
    ctx.close()


if __name__ == "__main__":
    main()
