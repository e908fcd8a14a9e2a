"""Measure spsamd_multiply_masked (op(A) op(B) on the keys of M only) against what a user does without it, and against
the unmasked product.

    python scripts/bench_masked.py [--only tri,poisson] [--reps 5] [--warmup 1] [--paths]

Workloads (device generators):
  rmat_tri      R-MAT scale 20, pattern symmetrised, values 1.0; L its strict lower triangle; (L L) o L into the DIGEST
                sink: result.sum is the triangle count
  poisson_AA_A  Poisson 4096^2, A A on A's own pattern
Three ways, each timed with HIP events on the context's stream (median of --reps after --warmup):
  masked        spsamd_multiply_masked (DIGEST for rmat_tri, COO for poisson_AA_A)
  coo+filter    what a user does today: spsamd_multiply into SINK_COO, then a torch filter of the tuples' keys against
                M's sorted keys on the device (searchsorted, in slices of 2^27 tuples)
  unmasked      spsamd_multiply into SINK_DIGEST: the whole product, reduced
--paths also times the masked call with every masked_path value forced (1 entry, 2 row, 3 wave).
Byte model of the masked call: per evaluated key its two lists (12 B per tuple of A_i and B_j, the k and the value) and
the key itself (8 B), against 8 TB/s -- an upper bound of the traffic (lists shared by neighbouring keys hit in cache).
One JSON line per measurement.
"""
import torch

import opbench as ob
from opbench import capi


def coo_filter(ctx, stream, A, B, mkeys, ncol):
    """spsamd_multiply to SINK_COO, then keep the tuples whose key i * ncol + j is in mkeys (sorted int64): the count,
    the sum and the kept tuples' positions, on the device."""
    r = ctx.multiply(A, B, sink=capi.SINK_COO)
    n = int(r.nnz)
    cnt, tot = 0, 0.0
    step = 1 << 27
    with torch.cuda.stream(stream):
        for o in range(0, n, step):
            m = min(step, n - o)
            i = torch.empty(m, dtype=torch.int32, device="cuda")
            j = torch.empty(m, dtype=torch.int32, device="cuda")
            v = torch.empty(m, dtype=torch.float64, device="cuda")
            ctx.memcpy(i.data_ptr(), r.idx0 + 4 * o, 4 * m)
            ctx.memcpy(j.data_ptr(), r.idx1 + 4 * o, 4 * m)
            ctx.memcpy(v.data_ptr(), r.val + 8 * o, 8 * m)
            k = i.to(torch.int64) * ncol + j.to(torch.int64)
            p = torch.searchsorted(mkeys, k).clamp_(max=mkeys.numel() - 1)
            hit = mkeys[p] == k
            cnt += int(hit.sum())
            tot += float(v[hit].sum())
    return cnt, tot, n


def record(rows, name, impl, med, ms, **extra):
    ob.record(rows, {"workload": name, "impl": impl, **ob.times(med, ms), **extra})


def bytes_model(la, lb):
    """12 B per tuple of A_i and B_j of every evaluated key, 8 B per key."""
    return 12.0 * (float(la.sum()) + float(lb.sum())) + 8.0 * la.numel()


def list_lengths(i, j, rowptr_a, colptr_b):
    la = (rowptr_a[i.long() + 1] - rowptr_a[i.long()]).double()
    lb = (colptr_b[j.long() + 1] - colptr_b[j.long()]).double()
    ok = (la > 0) & (lb > 0)
    return la[ok], lb[ok]


def run(ctx, stream, rows, name, A, B, M, mi, mj, ncol, sink, a, bytes_):
    med, ms = ob.time_call(stream, lambda: ctx.multiply_masked(A, B, M, sink=sink), a.reps, a.warmup)
    res = ctx.multiply_masked(A, B, M, sink=sink)
    out = dict(nnz=int(res.nnz), products=int(res.products), keys=int(mi.numel()), algo_bytes=bytes_,
               tbps=round(bytes_ / med / 1e9, 3), ms_numeric=round(res.ms_numeric, 4))
    if sink == capi.SINK_DIGEST:
        out["sum"] = res.sum
    record(rows, name, "masked", med, ms, **out)
    if a.paths:
        for p in (1, 2, 3):
            ctx.set_tuning("masked_path", p)
            med, ms = ob.time_call(stream, lambda: ctx.multiply_masked(A, B, M, sink=sink), a.reps, a.warmup)
            record(rows, name, "masked_path=%d" % p, med, ms, tbps=round(bytes_ / med / 1e9, 3))
        ctx.set_tuning("masked_path", 0)
    mkeys = mi.to(torch.int64) * ncol + mj.to(torch.int64)
    res_f = []
    med, ms = ob.time_call(stream, lambda: res_f.append(coo_filter(ctx, stream, A, B, mkeys, ncol)), a.reps, a.warmup)
    cnt, tot, nfull = res_f[-1]
    record(rows, name, "coo+filter", med, ms, nnz=cnt, sum=tot, nnz_full=nfull, coo_bytes=16 * nfull)
    med, ms = ob.time_call(stream, lambda: ctx.multiply(A, B, sink=capi.SINK_DIGEST), a.reps, a.warmup)
    d = ctx.multiply(A, B, sink=capi.SINK_DIGEST)
    record(rows, name, "unmasked digest", med, ms, nnz=int(d.nnz), products=int(d.products))


def rowptr(idx, n):
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=idx.device), torch.bincount(idx.long(), minlength=n).cumsum(0)])


def main():
    ap = ob.parser("tri,poisson", reps=5, warmup=1)
    ap.add_argument("--paths", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []

    def tri():
        R, t = ob.rmat(ctx, dev, 20)
        n = int(R.shape0)
        u, v = t[0].long(), t[1].long()
        hi, lo = torch.maximum(u, v), torch.minimum(u, v)
        off = hi != lo
        k = torch.unique(hi[off] * n + lo[off])                   # sorted: L row-major, each key once
        del off
        li, lj = (k // n).to(torch.int32), (k % n).to(torch.int32)
        lv = torch.ones(li.numel(), dtype=torch.float64, device=dev)
        del R, t, u, v, hi, lo, k
        torch.cuda.synchronize()
        L = capi.device_coo(li.data_ptr(), lj.data_ptr(), lv.data_ptr(), li.numel(), (n, n), 0)
        rp = rowptr(li, n)
        cp = rowptr(lj, n)                                         # columns of L (op(B) = L)
        la, lb = list_lengths(li, lj, rp, cp)
        run(ctx, stream, rows, "rmat_tri", L, L, L, li, lj, n, capi.SINK_DIGEST, a, bytes_model(la, lb))

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        n = int(A.shape0)
        rp = rowptr(t[0], n)
        cp = rowptr(t[1], n)
        la, lb = list_lengths(t[0], t[1], rp, cp)
        run(ctx, stream, rows, "poisson_AA_A", A, A, A, t[0], t[1], n, capi.SINK_COO, a, bytes_model(la, lb))

    ob.run(a.only.split(","), [("tri", tri), ("poisson", poisson)])
    ob.table(rows, [("workload", -14, "%s", "workload"), ("impl", -18, "%s", "impl"), ("ms", 10, "%.3f", "ms")])
    ctx.close()


if __name__ == "__main__":
    main()
