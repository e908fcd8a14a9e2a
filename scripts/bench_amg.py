"""Measure spsamd_solve_pcg_amg against the unpreconditioned spsamd_solve_pcg of the same process.

    python scripts/bench_amg.py [--only poisson,poisson_small,laplace] [--poisson-n 4096] [--small-n 1024] [--laplace-g 256]
                                [--tol 1e-8] [--max-iter 30000] [--sweep fuse|path] [--one V11|V22|none --iters K]

Workloads (device generators), b = A * 1, x0 = 0:
  poisson        the 5-point Poisson matrix on N^2 points (--poisson-n)
  poisson_small  the same at --small-n
  laplace        the 7-point Laplacian on g^3 points
The hierarchy is capi.Hierarchy (spsamd_aggregate in hash order with the SYMMETRIC flag, the tentative prolongator, two
spsamd_multiply calls a level, prepared operands); omega = 2/3, 4 coarse sweeps, V(1,1) and V(2,2).
Per configuration: levels and their orders, the operator complexity, the set-up split into aggregate, products and prepare
(host wall time, each stage synchronised), iterations to --tol, the stop reason, ms_setup and ms_iterate of the call (HIP
events), ms per iteration, launches per cycle, and the true relative residual ||b - A x|| / ||b|| by spsamd_multiply_dense
and torch.  Beside them `none`: spsamd_solve_pcg without a preconditioner, the fastest call of section 23 -- the yardstick,
on code this feature does not change.  `speedup` is its ms_iterate over the configuration's (set-up not counted).
Byte model at 8 TB/s for k_amg_smooth and k_amg_residual on level 0: 12 bytes per tuple plus three vector passes.
--sweep fuse: amg_fuse_rows over 64 .. 65536 (V(1,1)); --sweep path: amg_path 1 against 0.
--one CONFIG --iters K: that configuration alone on poisson with max_iter = K -- the run to put under a kernel trace;
scripts/bench_amg.py never starts a profiler itself.
One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi

REASONS = {0: "converged", 1: "maxiter", 2: "breakdown"}
CONFIGS = {"V11": (1, 1, 4, 2.0 / 3.0), "V22": (2, 2, 4, 2.0 / 3.0)}


def main():
    ap = ob.parser("poisson,poisson_small,laplace", reps=1, warmup=None)
    ap.add_argument("--poisson-n", type=int, default=4096)
    ap.add_argument("--small-n", type=int, default=1024)
    ap.add_argument("--laplace-g", type=int, default=256)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=30000)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--one", default="")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def ones_rhs(A, n):
        x = torch.ones((n, 1), dtype=torch.float64, device=dev)
        b = torch.zeros((n, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.multiply_dense(A, x, b)
        return b.reshape(n).contiguous()

    def residual(A, n, b, x):
        q = torch.zeros((n, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.multiply_dense(A, x.reshape(n, 1), q)
        return float(torch.linalg.norm(b - q.reshape(n)) / torch.linalg.norm(b))

    def plain(A, n, b, base, max_iter):
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        _, _hist, st = ctx.solve_pcg(A, b, x, capi.PRECOND_NONE, tol=a.tol, max_iter=max_iter, hist_capacity=1)
        it = max(int(st.iterations), 1)
        r = dict(base, what="none", iterations=int(st.iterations), reason=REASONS[int(st.reason)], ms_setup=round(st.ms_setup, 3),
                 ms=round(st.ms_iterate, 3), ms_per_iter=round(st.ms_iterate / it, 5), rel_residual=residual(A, n, b, x))
        ob.record(rows, r)
        return st.ms_iterate

    def amg(A, n, b, h, config, base, max_iter, ms_plain=None, extra=None):
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        res = capi.Result()
        _, _hist, st, ast = ctx.solve_pcg_amg(h, CONFIGS[config], b, x, tol=a.tol, max_iter=max_iter, hist_capacity=1, result=res)
        it = max(int(st.iterations), 1)
        nnz0 = int(ast.nnz[0])
        r = dict(base, what=config, iterations=int(st.iterations), reason=REASONS[int(st.reason)], ms_setup=round(st.ms_setup, 3),
                 ms=round(st.ms_iterate, 3), ms_per_iter=round(st.ms_iterate / it, 5), rel_residual=residual(A, n, b, x),
                 levels=int(ast.levels), fused_levels=int(ast.fused_levels), level_rows=[int(v) for v in ast.rows[:ast.levels]],
                 operator_complexity=round(ast.operator_complexity, 4), launches_per_cycle=int(ast.launches_per_cycle),
                 launches_per_iter=round(st.launches / it, 2), long_rows=int(ast.long_rows),
                 s_aggregate=round(h.seconds["aggregate"], 4), s_products=round(h.seconds["products"], 4),
                 s_prepare=round(h.seconds["prepare"], 4), workspace_GB=round(res.workspace_bytes / 1e9, 3),
                 model_ms_smooth_at_8TBps=round((12.0 * nnz0 + 24.0 * n) / ob.PEAK * 1e3, 4))
        if ms_plain is not None:
            r["speedup_iterate"] = round(ms_plain / st.ms_iterate, 3)
        if extra:
            r.update(extra)
        ob.record(rows, r)

    def workload(name, A, t, n):
        base = {"workload": name, "rows": n, "tuples": int(A.nnz)}
        b = ones_rhs(A, n)
        if a.one == "none":
            plain(A, n, b, base, a.iters)
            return
        h = capi.Hierarchy(ctx, A, flags=capi.AGG_SYMMETRIC)
        try:
            if a.one:
                amg(A, n, b, h, a.one, base, a.iters)
            elif a.sweep == "fuse":
                for rows_max in (64, 256, 1024, 4096, 16384, 65536):
                    ctx.set_tuning("amg_fuse_rows", rows_max)
                    try:
                        amg(A, n, b, h, "V11", base, a.max_iter, extra={"amg_fuse_rows": rows_max})
                    finally:
                        ctx.set_tuning("amg_fuse_rows", 0)
            elif a.sweep == "path":
                for path in (0, 1):
                    ctx.set_tuning("amg_path", path)
                    try:
                        amg(A, n, b, h, "V11", base, a.max_iter, extra={"amg_path": path})
                    finally:
                        ctx.set_tuning("amg_path", 0)
            else:
                ms_plain = plain(A, n, b, base, a.max_iter)
                for config in ("V11", "V22"):
                    amg(A, n, b, h, config, base, a.max_iter, ms_plain)
        finally:
            h.close()

    def poisson():
        A, t = ob.poisson2d(ctx, dev, a.poisson_n)
        workload("poisson_%d" % a.poisson_n, A, t, a.poisson_n ** 2)

    def poisson_small():
        if a.one:
            return
        A, t = ob.poisson2d(ctx, dev, a.small_n)
        workload("poisson_%d" % a.small_n, A, t, a.small_n ** 2)

    def laplace():
        if a.one:
            return
        A, t = ob.laplace3d(ctx, dev, a.laplace_g)
        workload("laplace_%d" % a.laplace_g, A, t, a.laplace_g ** 3)

    workloads = [("poisson", poisson), ("poisson_small", poisson_small), ("laplace", laplace)]
    for key, fn in workloads:                       # ("poisson" is a prefix of "poisson_small": match whole names)
        if key in only:
            fn()
            torch.cuda.empty_cache()
    ob.table(rows, [("workload", -14, "%s", "workload"), ("what", -5, "%s", "what"), ("fuse", 6, "%d", "amg_fuse_rows"),
                    ("path", 4, "%d", "amg_path"), ("levels", 6, "%d", "levels"), ("fused", 5, "%d", "fused_levels"),
                    ("op cx", 6, "%.3f", "operator_complexity"), ("iterations", 10, "%d", "iterations"),
                    ("reason", 10, "%s", "reason"), ("setup ms", 9, "%.2f", "ms_setup"), ("iterate ms", 11, "%.2f", "ms"),
                    ("ms / it", 9, "%.4f", "ms_per_iter"), ("launches / cycle", 16, "%d", "launches_per_cycle"),
                    ("residual", 10, "%.2e", "rel_residual"), ("speedup", 8, "%.2f", "speedup_iterate"),
                    ("agg s", 7, "%.3f", "s_aggregate"), ("prod s", 7, "%.3f", "s_products"), ("prep s", 7, "%.3f", "s_prepare"),
                    ("smooth model ms", 15, "%.4f", "model_ms_smooth_at_8TBps")])
    ctx.close()


if __name__ == "__main__":
    main()
