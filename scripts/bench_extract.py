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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spsparse_amd import capi  # noqa: E402

PEAK = 8.0e12


def dev_arrays(m, dev):
    return (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
            torch.empty(m, dtype=torch.float64, device=dev))


def ptrs(t):
    return [x.data_ptr() for x in t]


def copy_out(ctx, res, dev):
    """A SINK_COO result in torch tensors of its own."""
    n = int(res.nnz)
    t = dev_arrays(n, dev)
    for x, src, sz in zip(t, (res.idx0, res.idx1, res.val), (4, 4, 8)):
        if n:
            ctx.memcpy(x.data_ptr(), src, n * sz)
    return t


def selection(L, dim, dev):
    """S_L on the device: (tensors, Coo) of the len(L) x dim matrix with a 1.0 at (k, L[k])."""
    k = L.numel()
    t = (torch.arange(k, dtype=torch.int32, device=dev), L.contiguous(), torch.ones(k, dtype=torch.float64, device=dev))
    return t, capi.device_coo(*ptrs(t), k, (k, dim), 0)


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="block,principal,perm,redblack,afc,square")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx = capi.Context(0, stream.cuda_stream)
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
        ext = lambda: ctx.extract(A() if callable(A) else A, I, J)       # noqa: E731

        def base():
            T = ctx.multiply(SI, A_base if A_base is not None else A)
            return ctx.multiply(capi.result_operand(T), SJ, tB='T')
        ms_e, ms_b = [], []
        for rep in range(a.warmup + a.reps):
            if before:
                before()
            m1, res = timed(stream, ext)
            m2, G = timed(stream, base)
            if rep >= a.warmup:
                ms_e.append(m1); ms_b.append(m2)
        out = copy_out(ctx, G, dev)
        if before:
            before()
        res = ext()
        # (a product is not bit-reproducible from run to run: the comparison reads the copy the baseline read)
        got = copy_out(ctx, res if A_base is None else ctx.extract(A_base, I, J), dev)
        same = all(x.numel() == y.numel() for x, y in zip(got, out)) and torch.equal(got[0], out[0]) and \
            torch.equal(got[1], out[1]) and torch.equal(got[2].view(torch.int64), out[2].view(torch.int64))
        rowlen = torch.bincount(t[0], minlength=nrow)
        nsrc, nout = int(rowlen[Ii.long()].sum().item()), int(res.nnz)
        ordered = int(res.rows_light + res.rows_mid + res.rows_heavy) > 0
        by = 2 * 16.0 * nsrc + (2 * 4.0 * nsrc if J is not None else 0.0) + 16.0 * nout + (32.0 * nout if ordered else 0.0)
        e, b = float(np.median(ms_e)), float(np.median(ms_b))
        for impl, med, ms in (("spsamd_extract", e, ms_e), ("two_products", b, ms_b)):
            r = {"workload": name, "impl": impl, "ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "tuples_src": nsrc,
                 "tuples_out": nout, "same_tuples": bool(same)}
            if impl == "spsamd_extract":
                r.update({"path": "permuted" if ordered else "in order", "model_bytes": by, "model_ms_at_8TBps": round(by / PEAK * 1e3, 4),
                          "of_model": round(by / PEAK * 1e3 / e, 4), "ratio_to_products": round(e / b, 4),
                          "ms_consolidate": round(float(res.ms_consolidate), 4), "ms_symbolic": round(float(res.ms_symbolic), 4),
                          "ms_numeric": round(float(res.ms_numeric), 4),
                          "rows_light": int(res.rows_light), "rows_mid": int(res.rows_mid), "rows_heavy": int(res.rows_heavy)})
            print(json.dumps(r), flush=True)
            rows.append(r)
        del keep_i, keep_j

    if any(k in only for k in ("block", "principal", "perm")):
        scale = 20
        ne, n = 16 << scale, 1 << scale
        raw = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(raw))
        torch.cuda.synchronize()
        t = copy_out(ctx, ctx.consolidate(capi.device_coo(*ptrs(raw), ne, (n, n), -1), 0), dev)
        del raw
        A = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        g = torch.Generator(device="cpu").manual_seed(1)
        perm = torch.randperm(n, generator=g).to(torch.int32).to(dev)
        half = torch.sort(perm[: n // 2]).values.contiguous()
        if "block" in only:
            measure("rmat20_block", A, t, (n, n), torch.arange(n // 4, n // 2, dtype=torch.int32, device=dev), None)
        if "principal" in only:
            measure("rmat20_principal", A, t, (n, n), half, half)
        if "perm" in only:
            measure("rmat20_perm", A, t, (n, n), perm, perm)
        del t
        torch.cuda.empty_cache()
    if "redblack" in only:
        N = 4096
        n = N * N
        t = dev_arrays(5 * N * N - 4 * N, dev)
        ctx.gen_poisson2d(N, *ptrs(t))
        torch.cuda.synchronize()
        A = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        i = torch.arange(n, dtype=torch.int64, device=dev)
        red = ((i // N + i % N) % 2) == 0
        rb = torch.cat([i[red], i[~red]]).to(torch.int32).contiguous()
        measure("poisson_redblack", A, t, (n, n), rb, rb)
        del t
        torch.cuda.empty_cache()
    if "afc" in only:
        g = 256
        n = g ** 3
        t = dev_arrays(7 * g ** 3 - 6 * g * g, dev)
        ctx.gen_laplace3d(g, *ptrs(t))
        torch.cuda.synchronize()
        A = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        i = torch.arange(n, dtype=torch.int64, device=dev)
        cpt = ((i % g) % 2 == 0) & (((i // g) % g) % 2 == 0) & ((i // (g * g)) % 2 == 0)      # one point of every 2x2x2 aggregate
        measure("laplace_afc", A, t, (n, n), i[~cpt].to(torch.int32).contiguous(), i[cpt].to(torch.int32).contiguous())
        del t
        torch.cuda.empty_cache()
    if "square" in only:
        scale = 16
        ne, n = 16 << scale, 1 << scale
        raw = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(raw))
        torch.cuda.synchronize()
        R = capi.device_coo(*ptrs(raw), ne, (n, n), -1)
        state = {}

        def square():
            state["P"] = ctx.multiply(R, R)
        square()
        t = copy_out(ctx, state["P"], dev)
        A_base = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        g = torch.Generator(device="cpu").manual_seed(2)
        half = torch.sort(torch.randperm(n, generator=g)[: n // 2]).values.to(torch.int32).to(dev).contiguous()
        measure("square_principal", lambda: capi.result_operand(state["P"]), t, (n, n), half, half, before=square, A_base=A_base)
        del raw, t
        torch.cuda.empty_cache()

    print("%-17s %-15s %-9s %10s %10s %9s %8s %6s" % ("workload", "impl", "path", "ms", "model ms", "of model", "ratio", "same"))
    for r in rows:
        if r["impl"] == "spsamd_extract":
            print("%-17s %-15s %-9s %10.3f %10.3f %8.1f%% %8.3f %6s" % (r["workload"], r["impl"], r["path"], r["ms"], r["model_ms_at_8TBps"],
                                                                         100 * r["of_model"], r["ratio_to_products"], r["same_tuples"]))
        else:
            print("%-17s %-15s %-9s %10.3f" % (r["workload"], r["impl"], "", r["ms"]))
    bad = [r["workload"] for r in rows if r["impl"] == "spsamd_extract" and (r["ratio_to_products"] >= 1 or not r["same_tuples"])]
    print("gate (extract faster than the two products, same tuples):", "holds" if not bad else "MISSED by " + ", ".join(bad))
    ctx.close()


if __name__ == "__main__":
    main()
