"""Measure spsamd_extract (the submatrix op(A)(I, J) by index lists) against the only way to get it without the call: two
sparse products with selection matrices, S_I * A * S_J^T, through spsamd_multiply.

    python scripts/bench_extract.py [--only block,principal,perm,redblack,afc,square] [--reps 7] [--warmup 2]

Workloads (device generators; operands consolidated and handed in as sort0 = 0 device operands unless noted):
  rmat20_block      R-MAT scale 20, the row block [n/4, n/2) with all columns
  rmat20_principal  the principal submatrix on a sorted random half of the vertices
  rmat20_perm       a symmetric random permutation P A P^T
  poisson_redblack  Poisson 4096^2, I = J = reds ++ blacks
  laplace_afc       Laplace 256^3, A_FC: the C points of the 2x2x2 aggregation as columns, the other points as rows
  square_principal  A A of R-MAT scale 16 read in place from the context's output set, then a principal submatrix
Baseline: T = multiply(S_I, A), G = multiply(T, S_J, tB='T') with S_L = {(k, L[k], 1.0)} already on the device, sort0 = 0,
T chained in place.  Its tuples are compared with spsamd_extract's once per workload (bit for bit: every sum has one term).
Times: HIP events on the context's stream, median of --reps after --warmup, extract and baseline alternating.
Byte model at 8 TB/s: 16 B per tuple of the source rows per pass (count and emit: 2), 4 B per column-map lookup per pass (none
where J is ALL), 16 B per output tuple, and 32 B per output tuple more where the rows have to be ordered: reported, not gated.
One JSON line per measurement, then a table with the ratio extract / baseline (the gate: < 1 everywhere).
"""
import torch

import opbench as ob
from opbench import capi


def selection(L, dim, dev):
    """S_L on the device: (tensors, Coo) of the len(L) x dim matrix with a 1.0 at (k, L[k])."""
    k = L.numel()
    t = (torch.arange(k, dtype=torch.int32, device=dev), L.contiguous(), torch.ones(k, dtype=torch.float64, device=dev))
    return t, capi.device_coo(*ob.ptrs(t), k, (k, dim), 0)


def main():
    a = ob.parser("block,principal,perm,redblack,afc,square").parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def measure(name, A, t, shape, I, J, before=None, A_base=None):
        """A: the operand of spsamd_extract (a callable: made anew by `before` every repetition); t: its tuples as torch tensors
        (row-major) for the byte model; I, J: device int32 tensors or None; A_base: the baseline's operand (default A)."""
        nrow, ncol = shape
        Ii = I if I is not None else torch.arange(nrow, dtype=torch.int32, device=dev)
        Jj = J if J is not None else torch.arange(ncol, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        keep_i, SI = selection(Ii, nrow, dev)
        keep_j, SJ = selection(Jj, ncol, dev)
        torch.cuda.synchronize()

        def ext():
            return ctx.extract(A() if callable(A) else A, I, J)

        def base():
            T = ctx.multiply(SI, A_base if A_base is not None else A)
            return ctx.multiply(capi.result_operand(T), SJ, tB='T')
        (e, ms_e), (b, ms_b), res, G = ob.time_pair(stream, ext, base, a.reps, a.warmup, before)
        out = ob.copy_out(ctx, G, dev)
        if before:
            before()
        res = ext()
        # (a product is not bit-reproducible from run to run: the comparison reads the copy the baseline read)
        got = ob.copy_out(ctx, res if A_base is None else ctx.extract(A_base, I, J), dev)
        same = ob.same(got, out)
        rowlen = torch.bincount(t[0], minlength=nrow)
        nsrc, nout = int(rowlen[Ii.long()].sum().item()), int(res.nnz)
        ordered = int(res.rows_light + res.rows_mid + res.rows_heavy) > 0
        by = 2 * 16.0 * nsrc + (2 * 4.0 * nsrc if J is not None else 0.0) + 16.0 * nout + (32.0 * nout if ordered else 0.0)
        for impl, med, ms in (("spsamd_extract", e, ms_e), ("two_products", b, ms_b)):
            r = {"workload": name, "impl": impl, **ob.times(med, ms), "tuples_src": nsrc,
                 "tuples_out": nout, "same_tuples": bool(same)}
            if impl == "spsamd_extract":
                r.update({"path": "permuted" if ordered else "in order", "model_bytes": by, "model_ms_at_8TBps": round(by / ob.PEAK * 1e3, 4),
                          "of_model": round(by / ob.PEAK * 1e3 / e, 4), "ratio_to_products": round(e / b, 4),
                          "ms_consolidate": round(float(res.ms_consolidate), 4), "ms_symbolic": round(float(res.ms_symbolic), 4),
                          "ms_numeric": round(float(res.ms_numeric), 4),
                          "rows_light": int(res.rows_light), "rows_mid": int(res.rows_mid), "rows_heavy": int(res.rows_heavy)})
            ob.record(rows, r)

    def rmat20():
        R, raw = ob.rmat(ctx, dev, 20)
        A, t = ob.consolidated(ctx, dev, R)
        del raw
        n = int(A.shape0)
        g = torch.Generator(device="cpu").manual_seed(1)
        perm = torch.randperm(n, generator=g).to(torch.int32).to(dev)
        half = torch.sort(perm[: n // 2]).values.contiguous()
        if "block" in only:
            measure("rmat20_block", A, t, (n, n), torch.arange(n // 4, n // 2, dtype=torch.int32, device=dev), None)
        if "principal" in only:
            measure("rmat20_principal", A, t, (n, n), half, half)
        if "perm" in only:
            measure("rmat20_perm", A, t, (n, n), perm, perm)

    def redblack():
        N = 4096
        A, t = ob.poisson2d(ctx, dev, N)
        n = N * N
        i = torch.arange(n, dtype=torch.int64, device=dev)
        red = ((i // N + i % N) % 2) == 0
        rb = torch.cat([i[red], i[~red]]).to(torch.int32).contiguous()
        measure("poisson_redblack", A, t, (n, n), rb, rb)

    def afc():
        g = 256
        A, t = ob.laplace3d(ctx, dev, g)
        n = g ** 3
        i = torch.arange(n, dtype=torch.int64, device=dev)
        cpt = ((i % g) % 2 == 0) & (((i // g) % g) % 2 == 0) & ((i // (g * g)) % 2 == 0)      # one point of every 2x2x2 aggregate
        measure("laplace_afc", A, t, (n, n), i[~cpt].to(torch.int32).contiguous(), i[cpt].to(torch.int32).contiguous())

    def square():
        R, raw = ob.rmat(ctx, dev, 16)
        n = int(R.shape0)
        state = {}

        def again():
            state["P"] = ob.square(ctx, R)
        again()
        t = ob.copy_out(ctx, state["P"], dev)
        A_base = capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0)
        g = torch.Generator(device="cpu").manual_seed(2)
        half = torch.sort(torch.randperm(n, generator=g)[: n // 2]).values.to(torch.int32).to(dev).contiguous()
        measure("square_principal", lambda: capi.result_operand(state["P"]), t, (n, n), half, half, before=again, A_base=A_base)

    ob.run(only, [("block principal perm", rmat20), ("redblack", redblack), ("afc", afc), ("square", square)])
    ob.table(rows, [("workload", -17, "%s", "workload"), ("impl", -15, "%s", "impl"), ("path", -9, "%s", "path"),
                    ("ms", 10, "%.3f", "ms"), ("model ms", 10, "%.3f", "model_ms_at_8TBps"), ("of model", 9, "%.1f%%", ob.pct("of_model")),
                    ("ratio", 8, "%.3f", "ratio_to_products"), ("same", 6, "%s", lambda r: r["same_tuples"] if "path" in r else None)])
    ob.gate("extract faster than the two products, same tuples",
            [r["workload"] for r in rows if r["impl"] == "spsamd_extract" and (r["ratio_to_products"] >= 1 or not r["same_tuples"])])
    ctx.close()


if __name__ == "__main__":
    main()
