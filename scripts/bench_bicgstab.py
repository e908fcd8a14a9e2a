"""Measure spsamd_solve_bicgstab.

    python scripts/bench_bicgstab.py [--only convdiff,poisson] [--n 4096,1024] [--poisson-n 4096] [--cx 2] [--cy 1]
                                     [--tol 1e-8] [--max-iter 30000] [--host-iters 20] [--configs none,jacobi,ilu_hash]
                                     [--one CONFIG --iters K [--unfused]]

Workloads (made on the device), b = A * 1, x0 = 0:
  convdiff  upwind convection-diffusion on N^2 points (--n, one run per size): spsamd_gen_poisson2d's tuples with the
            diagonal set to 4 + cx + cy, the col - row = -1 tuples to -1 - cx and the col - row = -N tuples to -1 - cy
  poisson   the 5-point Poisson matrix on N^2 points (--poisson-n): a BiCGStab iteration beside section 23's PCG iteration
            on the same operator
Configurations: none, jacobi, ilu_hash (the ILU(0) of P A P^T for spsamd_color's hashed order; the colouring, the extract
and the factorisation are set-up and are timed apart).  M is a prepared handle, so that the call's own analyses are
reported separately from the iterations (`analyses`, ms_setup).
Per configuration: iterations to --tol, the stop reason, ms_setup, ms_iterate, ms per iteration, launches per iteration,
readbacks; the true relative residual ||b - A x|| / ||b|| by spsamd_multiply_dense and torch.
The reference point for time is the same loop driven from the host through the public calls -- spsamd_multiply_dense for
the two products, spsamd_solve_tri twice per preconditioner application on the prepared F (or a torch division for Jacobi),
torch for the vector updates and the dot products (each a host round trip) -- run for --host-iters iterations after two untimed:
`host_ms_per_iter` and the ratio.  Nothing outside the project runs here as a baseline, and the host loop's bits are not
compared: torch's dots are not the fold.
Byte model at 8 TB/s for the vector kernels of one iteration, 8 n bytes per vector pass: PASSES below, kernel by kernel,
for the fused and the unfused iteration; every row prints its sum, and --one prints the list.
--one CONFIG --iters K: that configuration alone on the first convdiff size with max_iter = K, tol = 0 and nothing else --
the run to put under a kernel trace; this script never starts a profiler itself.
Times: the call's own HIP events (ms_setup, ms_iterate).  One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi

REASONS = {0: "converged", 1: "maxiter", 2: "breakdown"}


def PASSES(precond, unfused):
    """[(kernel, vector passes)] of one iteration after the first: what each vector kernel of the loop reads and writes
    (k_bicgstab.hip; the k_pcg_ ones are the shared kernels of k_krylov.hip), a vector read twice by one kernel counted
    once.  Without a preconditioner y is p and z is s.  The SpMVs' own traffic (S, the gathers, the product) is not in
    the model: a fused dot costs the SpMV one more vector where its partner is not the SpMV's input."""
    none = precond == capi.PRECOND_NONE
    k = [("k_bicg_direction (r, p, v in; p out)", 4)]
    if precond == capi.PRECOND_JACOBI:
        k += [("k_pcg_jacobi<plain> y (p, d in; y out)", 3), ("k_pcg_jacobi<plain> z (s, d in; z out)", 3)]
    if unfused:
        k += [("k_pcg_dot (rhat, v)", 2), ("k_bicg_half<plain> (r, v in; s out)", 3), ("k_pcg_dot (s, s)", 1),
              ("k_pcg_dot (t, s)", 2), ("k_pcg_dot (t, t)", 1),
              ("k_bicg_update<1> (x, y, z in; x out)", 4), ("k_bicg_update<2> (s, t in; r out)", 3),
              ("k_pcg_dot (r, r)", 1), ("k_pcg_dot (rhat, r)", 2)]
    else:
        k += [("k_pcg_spmv<1>: rhat beside v = A y", 1), ("k_bicg_half<dot> (r, v in; s out)", 3),
              ("k_pcg_spmv<2>: s beside t = A z", 0 if none else 1),
              ("k_bicg_update<0> (x, y, z, s, t, rhat in; x, r out)", 7 if none else 8)]
    return k


def main():
    ap = ob.parser("convdiff,poisson", reps=1, warmup=None)
    ap.add_argument("--n", default="4096,1024")
    ap.add_argument("--poisson-n", type=int, default=4096)
    ap.add_argument("--cx", type=float, default=2.0)
    ap.add_argument("--cy", type=float, default=1.0)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=30000)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--configs", default="none,jacobi,ilu_hash")
    ap.add_argument("--one", default="")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--unfused", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")
    if a.unfused:
        ctx.set_tuning("pcg_fuse", 1)

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
        """(P A P^T as an operand, its tensors, perm, ms of colour + extract)."""
        out = tuple(torch.empty(m, dtype=torch.int32, device=dev) for m in (n, n, n + 1))
        ms_c, _ = ob.timed(stream, lambda: ctx.color(A, order, 1, capi.COLOR_SYMMETRIC, out=out))   # (the stencil's pattern is symmetric)
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
        """The loop of the header through the public calls, `iters` iterations: ms per iteration."""
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        r = b.clone()
        rhat = r.clone()
        p = torch.zeros(n, dtype=torch.float64, device=dev)
        v, t, w, y, z = (torch.zeros((n, 1), dtype=torch.float64, device=dev) for _ in range(5))

        def apply_m(u, out):
            if precond == capi.PRECOND_NONE:
                return u
            if precond == capi.PRECOND_JACOBI:
                return u / d
            ctx.solve_tri(F.coo, u.reshape(n, 1), capi.TRI_LOWER, capi.DIAG_UNIT, X=w)
            ctx.solve_tri(F.coo, w, capi.TRI_UPPER, capi.DIAG_NONUNIT, X=out)
            return out.reshape(n)

        def body():
            nonlocal p, r
            rho1 = float(torch.dot(r, r))
            rho = alpha = omega = 1.0
            for k in range(iters):
                p = r.clone() if k == 0 else r + (rho1 / rho) * (alpha / omega) * (p - omega * v.reshape(n))
                rho = rho1
                yy = apply_m(p, y)
                v.zero_()
                ctx.multiply_dense(A, yy.reshape(n, 1), v)
                alpha = rho / float(torch.dot(rhat, v.reshape(n)))
                s = r - alpha * v.reshape(n)
                float(torch.dot(s, s))                                   # the half-step test
                zz = apply_m(s, z)
                t.zero_()
                ctx.multiply_dense(A, zz.reshape(n, 1), t)
                tt = t.reshape(n)
                omega = float(torch.dot(tt, s)) / float(torch.dot(tt, tt))
                x.add_(yy, alpha=alpha).add_(zz, alpha=omega)
                r = s - omega * tt
                float(torch.dot(r, r))
                rho1 = float(torch.dot(rhat, r))
        with torch.cuda.stream(stream):
            ms, _ = ob.timed(stream, body)
        return ms / iters

    def model_ms(n, precond):
        return sum(p for _, p in PASSES(precond, a.unfused)) * 8.0 * n / ob.PEAK * 1e3

    def solve(config, A, t, n, b, precond, F, base, max_iter, tol, host=True, pcg=False):
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        res = capi.Result()
        call = ctx.solve_pcg if pcg else ctx.solve_bicgstab
        _, hist, st = call(A, b, x, precond, None if F is None else F.coo, tol=tol, max_iter=max_iter, hist_capacity=1, result=res)
        it = max(int(st.iterations), 1)
        r = dict(base, what=config + (" (pcg)" if pcg else ""), iterations=int(st.iterations), reason=REASONS[int(st.reason)],
                 analyses=int(st.analyses), ms_setup=round(st.ms_setup, 3), ms=round(st.ms_iterate, 3),
                 ms_per_iter=round(st.ms_iterate / it, 5), launches_per_iter=round(st.launches / it, 2),
                 readbacks=int(st.readbacks), rel_residual=residual(A, n, b, x), workspace_GB=round(res.workspace_bytes / 1e9, 3))
        if not pcg:
            r.update(model_passes=sum(p for _, p in PASSES(precond, a.unfused)), model_ms_at_8TBps=round(model_ms(n, precond), 4))
        if host and a.host_iters:
            d = None
            if precond == capi.PRECOND_JACOBI:                          # (the generator stores every key once)
                on = t[0] == t[1]
                d = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, t[0][on].long(), t[2][on])
                torch.cuda.synchronize()
            host_loop(A, n, b, precond, F, d, 2)                         # (untimed: torch loads its kernels on first use)
            h = host_loop(A, n, b, precond, F, d, a.host_iters)
            r.update(host_ms_per_iter=round(h, 5), host_over_device=round(h / (st.ms_iterate / it), 3))
        ob.record(rows, r)
        return st

    def configs(name, A, t, n, which, max_iter, tol, host=True):
        base = {"workload": name, "rows": n, "tuples": int(A.nnz)}
        b = ones_rhs(A, n)
        for config in which:
            if config == "none":
                solve(config, A, t, n, b, capi.PRECOND_NONE, None, base, max_iter, tol, host)
            elif config == "jacobi":
                solve(config, A, t, n, b, capi.PRECOND_JACOBI, None, base, max_iter, tol, host)
            elif config == "ilu_hash":
                PA, tp, perm, ms_r = reordered(A, n, capi.COLOR_ORDER_HASH)
                F, tf, ms_f = factor(PA)
                bp = b[perm.long()].contiguous()
                solve(config, PA, tp, n, bp, capi.PRECOND_LU, F, dict(base, ms_reorder=round(ms_r, 3), ms_factor=round(ms_f, 3)),
                      max_iter, tol, host)
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
            configs("convdiff_%d" % N, A, t, N * N, [a.one], a.iters, 0.0, host=False)
            precond = {"none": capi.PRECOND_NONE, "jacobi": capi.PRECOND_JACOBI}.get(a.one, capi.PRECOND_LU)
            for kernel, passes in PASSES(precond, a.unfused):
                print("model: %-55s %d passes, %.4f ms" % (kernel, passes, passes * 8.0 * N * N / ob.PEAK * 1e3))
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
    ob.table(rows, [("workload", -18, "%s", "workload"), ("what", -12, "%s", "what"), ("iterations", 10, "%d", "iterations"),
                    ("reason", 10, "%s", "reason"), ("setup ms", 10, "%.2f", "ms_setup"), ("iterate ms", 11, "%.2f", "ms"),
                    ("ms / it", 9, "%.4f", "ms_per_iter"), ("launches / it", 13, "%.1f", "launches_per_iter"),
                    ("reads", 6, "%d", "readbacks"), ("residual", 10, "%.2e", "rel_residual"),
                    ("host ms / it", 12, "%.4f", "host_ms_per_iter"), ("host / device", 13, "%.2f", "host_over_device"),
                    ("passes", 7, "%d", "model_passes"), ("vector model ms", 15, "%.4f", "model_ms_at_8TBps")])
    ctx.close()


if __name__ == "__main__":
    main()
