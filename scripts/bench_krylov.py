"""Measure spsamd_solve_pcg, and with it what the colouring's fewer levels cost in Krylov iterations.

    python scripts/bench_krylov.py [--only poisson,laplace] [--poisson-n 4096] [--natural-n 1024] [--laplace-g 256]
                                   [--tol 1e-8] [--max-iter 30000] [--host-iters 20] [--sweep every] [--one CONFIG --iters K]

Workloads (device generators), b = A * 1, x0 = 0:
  poisson  the 5-point Poisson matrix on N^2 points (--poisson-n); the ILU(0) of the natural ordering has 2 N - 1 levels
           and costs minutes at N = 4096, so that one configuration runs at --natural-n, beside the others at that size
  laplace  the 7-point Laplacian on g^3 points
Configurations: none, jacobi, ilu_natural, ilu_degree, ilu_hash (the ILU(0) of P A P^T for spsamd_color's two orders; the
colouring, the extract and the factorisation are set-up and are timed apart).  M is a prepared handle, so that the call's
own analyses are reported separately from the iterations (`analyses`, ms_setup).
Per configuration: iterations to --tol, the stop reason, ms_setup, ms_iterate, ms per iteration, launches per iteration,
readbacks; the true relative residual ||b - A x|| / ||b|| by spsamd_multiply_dense and torch.
The reference point for time is the same loop driven from the host through the public calls -- spsamd_multiply_dense for
q = A p, spsamd_solve_tri twice on the prepared F (or a torch division for Jacobi), torch for the vector updates and the
dot products (each a host round trip) -- run for --host-iters iterations: `host_ms_per_iter` and the ratio.  Nothing
outside the project runs here as a baseline, and the host loop's bits are not compared: torch's dots are not the fold.
Byte model at 8 TB/s for the vector kernels of one iteration (8 n bytes per vector pass): the fused update reads x, p, r, q
and writes x, r (6 passes); the direction reads z, p and writes p (3); the fused SpMV's dot costs nothing beyond the SpMV;
under Jacobi the division reads r, d and writes z (3); the stand-alone dot of the LU path reads r, z (2).
--sweep every: pcg_check_every over 1 .. 64 on poisson with ilu_hash.
--one CONFIG --iters K: that configuration alone on poisson with max_iter = K and nothing else -- the run to put under a
kernel trace; scripts/bench_krylov.py never starts a profiler itself.
Times: the call's own HIP events (ms_setup, ms_iterate).  One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi

REASONS = {0: "converged", 1: "maxiter", 2: "breakdown"}


def main():
    ap = ob.parser("poisson,laplace", reps=1, warmup=None)
    ap.add_argument("--poisson-n", type=int, default=4096)
    ap.add_argument("--natural-n", type=int, default=1024)
    ap.add_argument("--laplace-g", type=int, default=256)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=30000)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--one", default="")
    ap.add_argument("--iters", type=int, default=200)
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

    def reordered(A, n, order):
        """(P A P^T as an operand, its tensors, perm, ms of colour + extract)."""
        out = tuple(torch.empty(m, dtype=torch.int32, device=dev) for m in (n, n, n + 1))
        ms_c, _ = ob.timed(stream, lambda: ctx.color(A, order, 1, capi.COLOR_SYMMETRIC, out=out))
        ms_e, res = ob.timed(stream, lambda: ctx.extract(A, out[1], out[1]))
        t = ob.copy_out(ctx, res, dev)
        return capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0), t, out[1], ms_c + ms_e

    def factor(A):
        """(the prepared ILU(0) of A, its tensors, ms of the factorisation)."""
        ms_f, res = ob.timed(stream, lambda: ctx.factor_ilu0(A))
        t = ob.copy_out(ctx, res, dev)
        n = int(A.shape0)
        F = capi.Operand(ctx, capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0), '.', capi.AS_A)
        return F, t, ms_f

    def host_loop(A, n, b, precond, F, d, iters):
        """The same loop through the public calls, `iters` iterations: ms per iteration."""
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        r, p = b.clone(), torch.zeros(n, dtype=torch.float64, device=dev)
        q, z, y = (torch.zeros((n, 1), dtype=torch.float64, device=dev) for _ in range(3))
        rz = 0.0

        def body():
            nonlocal rz, p
            for k in range(iters):
                if precond == capi.PRECOND_NONE:
                    zz = r
                elif precond == capi.PRECOND_JACOBI:
                    zz = r / d
                else:
                    ctx.solve_tri(F.coo, r.reshape(n, 1), capi.TRI_LOWER, capi.DIAG_UNIT, X=y)
                    ctx.solve_tri(F.coo, y, capi.TRI_UPPER, capi.DIAG_NONUNIT, X=z)
                    zz = z.reshape(n)
                rz1 = float(torch.dot(r, zz))
                p = zz.clone() if k == 0 else zz + (rz1 / rz) * p
                rz = rz1
                q.zero_()
                ctx.multiply_dense(A, p.reshape(n, 1), q)
                alpha = rz / float(torch.dot(p, q.reshape(n)))
                x.add_(p, alpha=alpha)
                r.sub_(q.reshape(n), alpha=alpha)
                float(torch.dot(r, r))
        with torch.cuda.stream(stream):
            ms, _ = ob.timed(stream, body)
        return ms / iters

    def model_ms(n, precond):
        passes = 6 + 3 + (3 if precond == capi.PRECOND_JACOBI else 2 if precond == capi.PRECOND_LU else 0)
        return passes * 8.0 * n / ob.PEAK * 1e3

    def solve(name, config, A, t, n, b, precond, F, base, max_iter, host=True):
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        res = capi.Result()
        _, hist, st = ctx.solve_pcg(A, b, x, precond, None if F is None else F.coo, tol=a.tol, max_iter=max_iter, hist_capacity=1,
                                    result=res)
        it = max(int(st.iterations), 1)
        r = dict(base, what=config, iterations=int(st.iterations), reason=REASONS[int(st.reason)], analyses=int(st.analyses),
                 ms_setup=round(st.ms_setup, 3), ms=round(st.ms_iterate, 3), ms_per_iter=round(st.ms_iterate / it, 5),
                 launches_per_iter=round(st.launches / it, 2), readbacks=int(st.readbacks),
                 rel_residual=residual(A, n, b, x), model_ms_at_8TBps=round(model_ms(n, precond), 4),
                 workspace_GB=round(res.workspace_bytes / 1e9, 3))
        if host and a.host_iters:
            d = None
            if precond == capi.PRECOND_JACOBI:                          # (the generators store every key once)
                on = t[0] == t[1]
                d = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, t[0][on].long(), t[2][on])
                torch.cuda.synchronize()
            h = host_loop(A, n, b, precond, F, d, a.host_iters)
            r.update(host_ms_per_iter=round(h, 5), host_over_device=round(h / (st.ms_iterate / it), 3))
        ob.record(rows, r)
        return st

    def configs(name, A, t, n, which, max_iter, host=True):
        base = {"workload": name, "rows": n, "tuples": int(A.nnz)}
        b = ones_rhs(A, n)
        for config in which:
            if config == "none":
                solve(name, config, A, t, n, b, capi.PRECOND_NONE, None, base, max_iter, host)
            elif config == "jacobi":
                solve(name, config, A, t, n, b, capi.PRECOND_JACOBI, None, base, max_iter, host)
            elif config == "ilu_natural":
                F, tf, ms_f = factor(A)
                solve(name, config, A, t, n, b, capi.PRECOND_LU, F, dict(base, ms_factor=round(ms_f, 3)), max_iter, host)
                F.close()
            else:
                order = capi.COLOR_ORDER_DEGREE if config == "ilu_degree" else capi.COLOR_ORDER_HASH
                PA, tp, perm, ms_r = reordered(A, n, order)
                F, tf, ms_f = factor(PA)
                bp = b[perm.long()].contiguous()
                solve(name, config, PA, tp, n, bp, capi.PRECOND_LU, F, dict(base, ms_reorder=round(ms_r, 3), ms_factor=round(ms_f, 3)),
                      max_iter, host)
                F.close()
            torch.cuda.empty_cache()

    ALL = ["none", "jacobi", "ilu_degree", "ilu_hash"]

    def poisson():
        if a.one:
            A, t = ob.poisson2d(ctx, dev, a.poisson_n)
            configs("poisson_%d" % a.poisson_n, A, t, a.poisson_n ** 2, [a.one], a.iters, host=False)
            return
        if a.sweep == "every":
            A, t = ob.poisson2d(ctx, dev, a.poisson_n)
            n = a.poisson_n ** 2
            b = ones_rhs(A, n)
            PA, tp, perm, _ = reordered(A, n, capi.COLOR_ORDER_HASH)
            F, tf, _ = factor(PA)
            bp = b[perm.long()].contiguous()
            for every in (1, 2, 4, 8, 16, 32, 64):
                ctx.set_tuning("pcg_check_every", every)
                try:
                    solve("poisson_%d_sweep" % a.poisson_n, "pcg_check_every %d" % every, PA, tp, n, bp, capi.PRECOND_LU, F,
                          {"workload": "poisson_%d_sweep" % a.poisson_n, "pcg_check_every": every}, a.max_iter, host=False)
                finally:
                    ctx.set_tuning("pcg_check_every", 0)
            F.close()
            return
        A, t = ob.poisson2d(ctx, dev, a.poisson_n)
        configs("poisson_%d" % a.poisson_n, A, t, a.poisson_n ** 2, ALL, a.max_iter)
        del A, t
        torch.cuda.empty_cache()
        A, t = ob.poisson2d(ctx, dev, a.natural_n)
        configs("poisson_%d" % a.natural_n, A, t, a.natural_n ** 2, ["ilu_natural"] + ALL, a.max_iter)

    def laplace():
        if a.one or a.sweep:
            return
        A, t = ob.laplace3d(ctx, dev, a.laplace_g)
        configs("laplace_%d" % a.laplace_g, A, t, a.laplace_g ** 3, ALL, a.max_iter)

    ob.run(only, [("poisson", poisson), ("laplace", laplace)])
    ob.table(rows, [("workload", -18, "%s", "workload"), ("what", -20, "%s", "what"), ("iterations", 10, "%d", "iterations"),
                    ("reason", 10, "%s", "reason"), ("setup ms", 10, "%.2f", "ms_setup"), ("iterate ms", 11, "%.2f", "ms"),
                    ("ms / it", 9, "%.4f", "ms_per_iter"), ("launches / it", 13, "%.1f", "launches_per_iter"),
                    ("reads", 6, "%d", "readbacks"), ("residual", 10, "%.2e", "rel_residual"),
                    ("host ms / it", 12, "%.4f", "host_ms_per_iter"), ("host / device", 13, "%.2f", "host_over_device"),
                    ("vector model ms", 15, "%.4f", "model_ms_at_8TBps")])
    ctx.close()


if __name__ == "__main__":
    main()
