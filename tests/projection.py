"""Oracle-free value checks of a product at any size, by linearity (test helper, not a conftest).

For C = c diag(si) op(A) diag(sj) op(B) and a weight vector w over its columns, (C w)_i = c si_i (op(A) (sj * (op(B) w)))_i
and (u^T C)_j = c ((u si)^T op(A) diag(sj)) op(B))_j: two sparse matrix-vector products on the host, O(nnz(A) + nnz(B)),
with duplicates in raw tuples summed (the ADD policy is linear).  A value at the wrong column moves the row's weighted sum,
a value at the wrong row moves the column's.

Error bound.  Every computed value here is a sum of scalar terms, each a product of at most d roundings, so its error is at
most gamma_d * (the same sum over |terms|) (Higham, Accuracy and Stability, Lemma 3.1/3.3).  For a row i with P_i raw scalar
products (sum over its raw A tuples of the raw length of B's row k) and n_i raw A tuples, no term passes through more than
2 P_i + n_i + 6 roundings on the device (consolidating A and B, the cell's sum, the row's sum, the scalings), P_i + n_i + 4
in the host reference and P_i + 1 in the reducer below.  The row bound is gamma_m * S_i with m = 5 (P_i + n_i) + 64 and S_i
the reference evaluated on |values|: the three evaluations together, with room for the bound's own rounding.  The column
bound is the same with Q_j (raw scalar products landing in column j) and the raw tuple count of B's column j.  Such a bound
resolves a change of one value v only above about m u S / |v w|: it catches any misplaced value and any relative value
error of a short row, not a 1e-12 relative error in a hub row.

COO reducer.  reduce_coo() walks a COO result in chunks (torch, CPU or device) and returns what it takes to check the whole
result without ever holding it on the host: counts, strict ascending (i, j) order across chunk boundaries, index bounds,
NaNs, per-row sums, the row and column projections and the index hash of the digest sink (orc_mix64 summed mod 2^64).
"""
import numpy as np

from spsparse_amd import workloads as wl

U = 2.0 ** -53
MASK64 = (1 << 64) - 1
MIX_K = 0x9E3779B97F4A7C15 - (1 << 64)          # orc_mix64's multiplier as a signed int64
WEIGHT_STREAM = 0x5EED


def weights(n, seed, kind="real"):
    """Deterministic weights, a pure function of (n, seed, kind): 'real' in [1, 2), 'int' the integers 1 .. 2^16
    (every projection of an integer stencil product is then exact in fp64)."""
    r = wl.draw(seed, WEIGHT_STREAM, np.arange(n, dtype=np.uint64))
    if kind == "real":
        return 1.0 + (r >> np.uint64(11)).astype(np.float64) * U
    if kind == "int":
        return ((r >> np.uint64(32)) % np.uint64(1 << 16) + np.uint64(1)).astype(np.float64)
    raise ValueError(kind)


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def sign_of(i, j):
    """+-1 from a hash of (i, j): duplicates of one index pair share their sign."""
    from oracle import binding as orc
    return np.where((orc.mix64(i, j) >> np.uint64(40)) & np.uint64(1), -1.0, 1.0)


def _op(x, t):
    i, j, v, shape = x[:4]
    if t == 'T':
        return np.asarray(j), np.asarray(i), np.asarray(v, dtype=np.float64), (int(shape[1]), int(shape[0]))
    return np.asarray(i), np.asarray(j), np.asarray(v, dtype=np.float64), (int(shape[0]), int(shape[1]))


def mv(x, vec, t='.'):
    """op(X) vec from raw tuples (duplicates summed)."""
    i, j, v, (n, _) = _op(x, t)
    return np.bincount(i, weights=v * vec[j], minlength=n)


def row_sums_by_linearity(a, b, n_rows, n_inner):
    """(A B) 1 = A (B 1): per-row sums of C from O(nnz) host arithmetic."""
    b1 = np.bincount(b[0], weights=b[2], minlength=n_inner)
    return np.bincount(a[0], weights=a[2] * b1[a[1]], minlength=n_rows)


def vm(vec, x, t='.'):
    """vec^T op(X) from raw tuples."""
    i, j, v, (_, m) = _op(x, t)
    return np.bincount(j, weights=v * vec[i], minlength=m)


class Reference:
    """Row and column projections of C = c diag(si) op(A) diag(sj) op(B) diag(sk) from raw host tuples, with their
    rigorous bounds.  si, sj, sk: dense vectors (0 where the scale vector has no entry: that row, term or column is
    skipped, as spsparse does) or None."""

    def __init__(self, a, b, C_=1.0, si=None, sj=None, sk=None, tA='.', tB='.'):
        self.a0, self.a1, av, (self.n, self.ni) = _op(a, tA)
        self.b0, self.b1, self.bv, (nb, self.m) = _op(b, tB)
        assert nb == self.ni, (nb, self.ni)
        self.C = float(C_)
        self.si = np.ones(self.n) if si is None else np.asarray(si, dtype=np.float64)
        self.sk = np.ones(self.m) if sk is None else np.asarray(sk, dtype=np.float64)
        self.av = av if sj is None else av * np.asarray(sj, dtype=np.float64)[self.a1]
        blen = np.bincount(self.b0, minlength=self.ni).astype(np.float64)
        alen = np.bincount(self.a1, minlength=self.ni).astype(np.float64)
        self.m_row = 5.0 * (np.bincount(self.a0, weights=blen[self.a1], minlength=self.n) +
                            np.bincount(self.a0, minlength=self.n)) + 64
        self.m_col = 5.0 * (np.bincount(self.b1, weights=alen[self.b0], minlength=self.m) +
                            np.bincount(self.b1, minlength=self.m)) + 64

    def rows(self, w):
        """(C w, bound) per row."""
        ws = self.sk * np.asarray(w, dtype=np.float64)
        bw = np.bincount(self.b0, weights=self.bv * ws[self.b1], minlength=self.ni)
        babs = np.bincount(self.b0, weights=np.abs(self.bv * ws[self.b1]), minlength=self.ni)
        val = self.C * self.si * np.bincount(self.a0, weights=self.av * bw[self.a1], minlength=self.n)
        s = abs(self.C) * np.abs(self.si) * np.bincount(self.a0, weights=np.abs(self.av) * babs[self.a1], minlength=self.n)
        return val, gamma(self.m_row) * s

    def cols(self, u):
        """(u^T C, bound) per column."""
        us = self.si * np.asarray(u, dtype=np.float64)
        ua = np.bincount(self.a1, weights=self.av * us[self.a0], minlength=self.ni)
        uabs = np.bincount(self.a1, weights=np.abs(self.av * us[self.a0]), minlength=self.ni)
        val = self.C * self.sk * np.bincount(self.b1, weights=self.bv * ua[self.b0], minlength=self.m)
        s = abs(self.C) * np.abs(self.sk) * np.bincount(self.b1, weights=np.abs(self.bv) * uabs[self.b0], minlength=self.m)
        return val, gamma(self.m_col) * s


def within(got, want, bound):
    """(ok, largest |got - want| / bound): every entry inside its bound; where the bound is 0 (an empty row or column)
    the value must be exactly the reference."""
    got, want, bound = (np.asarray(x, dtype=np.float64) for x in (got, want, bound))
    err = np.abs(got - want)
    ok = bool(np.all(err <= bound)) and not np.any(np.isnan(got))
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0
    return ok, ratio


# ---------------------------------------------------------------------------------------------- the COO reducer

class CooSummary:
    """What reduce_coo() found.  Arrays are numpy; `complete` is False when an index out of bounds stopped the walk
    (the weights are not indexed with it)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def mix64_t(i64, j64):
    """orc_mix64 on int64 torch tensors: (i << 32 | j) * K mod 2^64, then x ^ (x >>> 29) by a masked arithmetic shift."""
    x = ((i64 << 32) | j64) * MIX_K
    return x ^ ((x >> 29) & ((1 << 35) - 1))


def host_source(i, j, v):
    """Chunk reader over host arrays (CPU tensors, no copy)."""
    import torch
    ti, tj, tv = (torch.from_numpy(np.ascontiguousarray(x)) for x in (i, j, v))
    return lambda lo, cnt: (ti[lo:lo + cnt], tj[lo:lo + cnt], tv[lo:lo + cnt])


def device_source(ctx, res, chunk):
    """Chunk reader over a SINK_COO result in device memory: each chunk is copied (spsamd_memcpy) into preallocated
    device tensors, so the result is never copied whole."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n = min(int(chunk), max(1, int(res.nnz)))
    bi = torch.empty(n, dtype=torch.int32, device=dev)
    bj = torch.empty(n, dtype=torch.int32, device=dev)
    bv = torch.empty(n, dtype=torch.float64, device=dev)

    def read(lo, cnt):
        torch.cuda.synchronize()                   # the previous chunk's readers are done with the buffers
        ctx.memcpy(bi.data_ptr(), res.idx0 + 4 * lo, 4 * cnt)
        ctx.memcpy(bj.data_ptr(), res.idx1 + 4 * lo, 4 * cnt)
        ctx.memcpy(bv.data_ptr(), res.val + 8 * lo, 8 * cnt)     # synchronous on the library's stream
        return bi[:cnt], bj[:cnt], bv[:cnt]
    return read


def reduce_coo(source, nnz, shape, w=None, u=None, chunk=1 << 27, device="cpu"):
    """Walk nnz tuples of a shape-(n, m) COO result, `chunk` at a time (source(lo, cnt) -> int32 i, int32 j, float64 v
    tensors on `device`).  w: weights over columns (row projection sum_j w_j v_ij), u: weights over rows (column
    projection sum_i u_i v_ij); None: not computed."""
    import torch
    n, m = int(shape[0]), int(shape[1])
    nnz, chunk = int(nnz), int(chunk)
    f64 = dict(dtype=torch.float64, device=device)
    row_nnz = torch.zeros(n, dtype=torch.int64, device=device)
    row_sum = torch.zeros(n, **f64)
    row_w = torch.zeros(n, **f64) if w is not None else None
    col_u = torch.zeros(m, **f64) if u is not None else None
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64), device=device) if w is not None else None
    ut = torch.as_tensor(np.asarray(u, dtype=np.float64), device=device) if u is not None else None
    h, prev, seen = 0, -1, 0
    first_disorder, nan, vmin, vmax = None, 0, np.inf, -np.inf
    in_bounds = True
    for lo in range(0, nnz, chunk):
        cnt = min(chunk, nnz - lo)
        i, j, v = source(lo, cnt)
        i64, j64 = i.long(), j.long()
        lim = torch.stack([i64.min(), i64.max(), j64.min(), j64.max()]).tolist()
        if lim[0] < 0 or lim[1] >= n or lim[2] < 0 or lim[3] >= m:
            in_bounds = False
            break
        key = i64 * m + j64
        if cnt > 1:
            bad = torch.nonzero(key[1:] <= key[:-1])
            if bad.numel() and first_disorder is None:
                first_disorder = lo + 1 + int(bad[0, 0])
        if int(key[0]) <= prev and first_disorder is None:
            first_disorder = lo
        prev = int(key[-1])
        nan += int(torch.isnan(v).sum())
        vr = torch.stack([v.min(), v.max()]).tolist()
        vmin, vmax = min(vmin, vr[0]), max(vmax, vr[1])
        # per run of equal rows (one per row when ordered): one segment sum each, then one add per run -- an
        # index_add_ per tuple would serialise a hub row's atomics on one address
        rows, runs = torch.unique_consecutive(i64, return_counts=True)
        row_nnz.index_add_(0, rows, runs)
        row_sum.index_add_(0, rows, torch.segment_reduce(v, "sum", lengths=runs))
        if row_w is not None:
            row_w.index_add_(0, rows, torch.segment_reduce(v * wt[j64], "sum", lengths=runs))
        if col_u is not None:
            col_u.index_add_(0, j64, v * ut[i64])
        h = (h + int(mix64_t(i64, j64).sum())) & MASK64
        seen += cnt
        del i64, j64, key, rows, runs
    cpu = (lambda t: None if t is None else t.cpu().numpy())
    return CooSummary(nnz=seen, complete=in_bounds and seen == nnz, ordered=first_disorder is None,
                      first_disorder=first_disorder, nan=nan, vmin=vmin, vmax=vmax, hash=h,
                      row_nnz=cpu(row_nnz), row_sum=cpu(row_sum), row_w=cpu(row_w), col_u=cpu(col_u))


def failures(s, ref=None, w=None, u=None, want=None, exact=False):
    """Names of the checks summary `s` fails; [] when it passes them all.
    ref: a Reference (row projections with 1 and w, column projection with u, against their bounds; bit for bit when
    `exact`); want: (nnz, row_nnz, hash) of the index set, e.g. from the oracle's streaming digest."""
    bad = []
    if not s.complete:
        return ["bounds"]
    if s.nan:
        bad.append("nan")
    if not s.ordered:
        bad.append("order")
    if want is not None:
        nnz, rn, h = want
        if s.nnz != nnz:
            bad.append("count")
        if rn is not None and not np.array_equal(s.row_nnz, rn):
            bad.append("row_nnz")
        if h is not None and s.hash != h:
            bad.append("hash")
    if ref is not None:
        checks = [("row_sum", s.row_sum, ref.rows(np.ones(ref.m)))]
        if w is not None:
            checks.append(("row_w", s.row_w, ref.rows(w)))
        if u is not None:
            checks.append(("col_u", s.col_u, ref.cols(u)))
        for name, got, (val, bound) in checks:
            ok = np.array_equal(got, val) if exact else within(got, val, bound)[0]
            if not ok:
                bad.append(name)
    return bad
