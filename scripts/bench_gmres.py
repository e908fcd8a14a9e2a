"""Measure spsamd_solve_gmres.

    python scripts/bench_gmres.py [--only convdiff,poisson] [--n 4096,1024] [--poisson-n 4096] [--cx 2] [--cy 1]
                                  [--tol 1e-8] [--restart 30] [--max-iter 3000] [--step-cycles 2] [--configs none,jacobi,ilu_hash]
                                  [--no-bicgstab] [--one CONFIG --iters K [--path 1]]

Workloads (made on the device), b = A * 1, x0 = 0: those of scripts/bench_bicgstab.py -- upwind convection-diffusion on N^2
points (--n, one run per size) and the 5-point Poisson matrix (--poisson-n).  Configurations: none, jacobi, ilu_hash (the
ILU(0) of P A P^T for spsamd_color's hashed order, M a prepared handle).
Per configuration, GMRES(--restart) to --tol within --max-iter steps: steps, cycles (readbacks - 1), the stop reason,
ms_iterate, ms per step, launches per step, and the true relative residual ||b - A x|| / ||b|| by spsamd_multiply_dense
and torch; beside it spsamd_solve_bicgstab on the same operands (iterations, reason, ms, true residual) unless
--no-bicgstab.
Per step, over --step-cycles whole cycles (max_iter = cycles x restart, tol = 0): gmres_path 0 against gmres_path 1 and
against the same loop driven from the host through the public calls -- spsamd_multiply_dense for the product,
spsamd_solve_tri twice per preconditioner application (a torch division for Jacobi), torch.mv for the two Gram-Schmidt
passes over the stored block, one host round trip per step for the Hessenberg column -- after one untimed cycle.  The host
loop's bits are not compared: torch's reductions are not the fold.  The gate: path 0 is not slower per step than either.
Byte model at 8 TB/s, 8 n bytes per vector pass: a step at inner index j moves 4 j + 10 passes in the two Gram-Schmidt
passes (each projection j + 2, each subtraction j + 3) and 2 in the scale; PASSES below, kernel by kernel, summed over the
j of one cycle.  The SpMV's own traffic is not in the model.
--one CONFIG --iters K: that configuration alone on the first convdiff size with max_iter = K, tol = 0 and nothing else --
the run to put under a kernel trace; this script never starts a profiler itself.
Times: the call's own HIP events (ms_setup, ms_iterate).  One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi

REASONS = {0: "converged", 1: "maxiter", 2: "breakdown"}


def PASSES(precond, m):
    """[(kernel, vector passes summed over the m steps of one full cycle and its end)]: what each vector kernel of the block
    path reads and writes (k_gmres.hip; the k_pcg_ ones are the shared kernels of k_krylov.hip)."""
    js = range(m)
    k = [("k_gmres_project x2 (w, v_0..v_j in)", sum(2 * (j + 2) for j in js)),
         ("k_gmres_subtract<0> (w, v_0..v_j in; w out)", sum(j + 3 for j in js)),
         ("k_gmres_subtract<1> (w, v_0..v_j in; w out)", sum(j + 3 for j in js)),
         ("k_gmres_scale (w in; v out)", 2 * m),
         ("k_gmres_combine (v_0..v_{m-1} in; x in and out, or u out)", m + 2 if precond == capi.PRECOND_NONE else m + 1)]
    if precond == capi.PRECOND_JACOBI:
        k += [("k_pcg_jacobi<plain> (v, d in; z out)", 3 * (m + 1)), ("k_gmres_addx (x, z in; x out)", 3)]
    k += [("k_pcg_residual<dot> (b, q in; r out)", 3)]
    return k


def main():
    ap = ob.parser("convdiff,poisson", reps=1, warmup=None)
    ap.add_argument("--n", default="4096,1024")
    ap.add_argument("--poisson-n", type=int, default=4096)
    ap.add_argument("--cx", type=float, default=2.0)
    ap.add_argument("--cy", type=float, default=1.0)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--max-iter", type=int, default=3000)
    ap.add_argument("--step-cycles", type=int, default=2)
    ap.add_argument("--configs", default="none,jacobi,ilu_hash")
    ap.add_argument("--no-bicgstab", action="store_true")
    ap.add_argument("--one", default="")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--path", type=int, default=0)
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows, missed = [], []
    only = a.only.split(",")
    m = a.restart

    def convdiff2d(N):
        A, t = ob.poisson2d(ctx, dev, N)
        off = t[1] - t[0]
        t[2][off == 0] = 4.0 + a.cx + a.cy
        t[2][off == -1] = -1.0 - a.cx
        t[2][off == -N] = -1.0 - a.cy
        torch.cuda.synchronize()
        return A, t

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
        out = tuple(torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n, n + 1))
        ctx.color(A, order, 1, capi.COLOR_SYMMETRIC, out=out)
        t = ob.copy_out(ctx, ctx.extract(A, out[1], out[1]), dev)
        return capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0), t, out[1]

    def factor(A):
        t = ob.copy_out(ctx, ctx.factor_ilu0(A), dev)
        n = int(A.shape0)
        return capi.Operand(ctx, capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0), '.', capi.AS_A), t

    def host_loop(A, n, b, precond, F, d, cycles):
        """The loop of the header through the public calls, `cycles` full cycles: ms per step."""
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        V = torch.empty((m + 1, n), dtype=torch.float64, device=dev)
        w, t1, z = (torch.zeros((n, 1), dtype=torch.float64, device=dev) for _ in range(3))

        def apply_m(u):
            if precond == capi.PRECOND_NONE:
                return u
            if precond == capi.PRECOND_JACOBI:
                return u / d
            ctx.solve_tri(F.coo, u.reshape(n, 1), capi.TRI_LOWER, capi.DIAG_UNIT, X=t1)
            ctx.solve_tri(F.coo, t1, capi.TRI_UPPER, capi.DIAG_NONUNIT, X=z)
            return z.reshape(n)

        def body():
            r = b.clone()
            for _ in range(cycles):
                beta = float(torch.linalg.norm(r))
                V[0] = r / beta
                H = torch.zeros((m + 1, m), dtype=torch.float64)
                for j in range(m):
                    w.zero_()
                    ctx.multiply_dense(A, apply_m(V[j]).reshape(n, 1), w)
                    ww = w.reshape(n)
                    h = torch.mv(V[:j + 1], ww)
                    ww -= torch.mv(V[:j + 1].t(), h)
                    h2 = torch.mv(V[:j + 1], ww)
                    ww -= torch.mv(V[:j + 1].t(), h2)
                    hn = torch.linalg.norm(ww)
                    H[:j + 1, j] = (h + h2).cpu()                      # the step's round trip: the Hessenberg column on the host
                    H[j + 1, j] = float(hn)
                    V[j + 1] = ww / hn
                e = torch.zeros(m + 1, dtype=torch.float64)
                e[0] = beta
                y = torch.linalg.lstsq(H, e.reshape(-1, 1)).solution.reshape(m).to(dev)
                x.add_(apply_m(torch.mv(V[:m].t(), y)))
                w.zero_()
                ctx.multiply_dense(A, x.reshape(n, 1), w)
                r = b - w.reshape(n)
        with torch.cuda.stream(stream):
            ms, _ = ob.timed(stream, body)
        return ms / (cycles * m)

    def model_ms(n, precond):
        return sum(p for _, p in PASSES(precond, m)) * 8.0 * n / ob.PEAK * 1e3 / m

    def call(A, n, b, precond, F, max_iter, tol, path=0, bicgstab=False):
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        res = capi.Result()
        ctx.set_tuning("gmres_path", path)
        try:
            if bicgstab:
                _, _, st = ctx.solve_bicgstab(A, b, x, precond, None if F is None else F.coo, tol=tol, max_iter=max_iter, hist_capacity=1, result=res)
            else:
                _, _, st = ctx.solve_gmres(A, b, x, precond, None if F is None else F.coo, tol=tol, max_iter=max_iter, restart=m,
                                           hist_capacity=1, result=res)
        finally:
            ctx.set_tuning("gmres_path", 0)
        return st, res, x

    def solve(config, A, t, n, b, precond, F, base, max_iter, tol, compare=True):
        st, res, x = call(A, n, b, precond, F, max_iter, tol, a.path if a.one else 0)
        it = max(int(st.iterations), 1)
        r = dict(base, what=config, restart=m, steps=int(st.iterations), cycles=int(st.readbacks) - 1, reason=REASONS[int(st.reason)],
                 analyses=int(st.analyses), ms_setup=round(st.ms_setup, 3), ms=round(st.ms_iterate, 3),
                 ms_per_step=round(st.ms_iterate / it, 5), launches_per_step=round(st.launches / it, 2),
                 rel_residual=residual(A, n, b, x), workspace_GB=round(res.workspace_bytes / 1e9, 3),
                 model_passes_per_step=round(sum(p for _, p in PASSES(precond, m)) / m, 2), model_ms_at_8TBps=round(model_ms(n, precond), 4))
        if compare:
            steps = a.step_cycles * m
            s0, _, _ = call(A, n, b, precond, F, steps, 0.0, 0)
            s1, _, _ = call(A, n, b, precond, F, steps, 0.0, 1)
            d = None
            if precond == capi.PRECOND_JACOBI:                          # (the generator stores every key once)
                on = t[0] == t[1]
                d = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, t[0][on].long(), t[2][on])
                torch.cuda.synchronize()
            host_loop(A, n, b, precond, F, d, 1)                         # (untimed: torch loads its kernels on first use)
            h = host_loop(A, n, b, precond, F, d, a.step_cycles)
            p0, p1 = s0.ms_iterate / max(int(s0.iterations), 1), s1.ms_iterate / max(int(s1.iterations), 1)
            r.update(step_ms_path0=round(p0, 5), step_ms_path1=round(p1, 5), step_ms_host=round(h, 5),
                     path1_over_path0=round(p1 / p0, 3), host_over_path0=round(h / p0, 3))
            if n >= 4096 * 4096 and (p1 < p0 or h < p0):
                missed.append("%s %s" % (base["workload"], config))
            if not a.no_bicgstab:
                sb, _, xb = call(A, n, b, precond, F, 30000, tol, bicgstab=True)
                r.update(bicgstab_iterations=int(sb.iterations), bicgstab_reason=REASONS[int(sb.reason)], bicgstab_ms=round(sb.ms_iterate, 3),
                         bicgstab_rel_residual=residual(A, n, b, xb))
        ob.record(rows, r)

    def configs(name, A, t, n, which, max_iter, tol, compare=True):
        base = {"workload": name, "rows": n, "tuples": int(A.nnz)}
        b = ones_rhs(A, n)
        for config in which:
            if config == "none":
                solve(config, A, t, n, b, capi.PRECOND_NONE, None, base, max_iter, tol, compare)
            elif config == "jacobi":
                solve(config, A, t, n, b, capi.PRECOND_JACOBI, None, base, max_iter, tol, compare)
            elif config == "ilu_hash":
                PA, tp, perm = reordered(A, n, capi.COLOR_ORDER_HASH)
                F, tf = factor(PA)
                solve(config, PA, tp, n, b[perm.long()].contiguous(), capi.PRECOND_LU, F, base, max_iter, tol, compare)
                F.close()
            else:
                raise SystemExit("unknown configuration %r" % config)
            torch.cuda.empty_cache()

    which = a.configs.split(",")
    sizes = [int(s) for s in a.n.split(",")]

    def convdiff():
        if a.one:
            N = sizes[0]
            A, t = convdiff2d(N)
            configs("convdiff_%d" % N, A, t, N * N, [a.one], a.iters, 0.0, compare=False)
            precond = {"none": capi.PRECOND_NONE, "jacobi": capi.PRECOND_JACOBI}.get(a.one, capi.PRECOND_LU)
            for kernel, passes in PASSES(precond, m):
                print("model: %-50s %5d passes a cycle, %.3f ms" % (kernel, passes, passes * 8.0 * N * N / ob.PEAK * 1e3))
            return
        for N in sizes:
            A, t = convdiff2d(N)
            configs("convdiff_%d" % N, A, t, N * N, which, a.max_iter, a.tol)
            del A, t
            torch.cuda.empty_cache()

    def poisson():
        if a.one:
            return
        N = a.poisson_n
        A, t = ob.poisson2d(ctx, dev, N)
        configs("poisson_%d" % N, A, t, N * N, which, a.max_iter, a.tol)

    ob.run(only, [("convdiff", convdiff), ("poisson", poisson)])
    ob.table(rows, [("workload", -14, "%s", "workload"), ("what", -9, "%s", "what"), ("steps", 6, "%d", "steps"), ("cycles", 6, "%d", "cycles"),
                    ("reason", 10, "%s", "reason"), ("ms", 10, "%.1f", "ms"), ("ms / step", 9, "%.4f", "ms_per_step"),
                    ("residual", 9, "%.1e", "rel_residual"), ("path 0", 8, "%.4f", "step_ms_path0"), ("path 1", 8, "%.4f", "step_ms_path1"),
                    ("host", 8, "%.4f", "step_ms_host"), ("p1 / p0", 7, "%.2f", "path1_over_path0"), ("host / p0", 9, "%.2f", "host_over_path0"),
                    ("model ms", 8, "%.4f", "model_ms_at_8TBps"), ("bicg its", 8, "%d", "bicgstab_iterations"),
                    ("bicg ms", 9, "%.1f", "bicgstab_ms"), ("bicg residual", 13, "%.1e", "bicgstab_rel_residual")])
    if not a.one:
        ob.gate("gmres_path 0 no slower per step than path 1 and than the host loop at 4096^2", missed)
    ctx.close()


if __name__ == "__main__":
    main()
