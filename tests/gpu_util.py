"""What the GPU test files (tests/test_gpu_*.py, tests/test_*_cpp.py, tests/test_abi.py) share: the context fixture, operands
as C structs, the bit-for-bit tuple check, the exact digest check, the path-knob wrappers, the solve wrapper and its bit check, the memory sampler
and the g++ line of the C++ tests.
Importing it needs no GPU.  The seeded input makers stay with their tests: no two of them draw the same random stream."""
import contextlib
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from tests import add_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    """One context on device 0 for the module (import the name into the module to use it)."""
    from spsparse_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def dev(arrs, keep):
    """numpy arrays as torch device copies, kept alive in `keep` for as long as a struct points at them."""
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
    torch.cuda.synchronize()
    keep.append(t)
    return t


def coo(X, shape, sort0=-1, device=False, keep=None, no_val=False):
    """Coo struct of (idx0, idx1, val): host numpy arrays or torch device copies (kept alive in `keep`); no_val: val NULL."""
    from spsparse_amd import capi
    if device:
        t = dev((np.asarray(X[0], np.int32), np.asarray(X[1], np.int32), np.asarray(X[2], np.float64)), keep)
        s = capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(X[2]), shape, sort0)
    else:
        s, k = capi.host_coo(X[0], X[1], X[2], shape, sort0)
        keep.append(k)
    if no_val:
        s.val = None
    return s


def device_operand(ctx, gen, n_tuples, shape, sort0=-1):
    """(Coo, tensors) of n_tuples written on the device by gen(ptr0, ptr1, ptrv), one of the context's generators."""
    import torch
    from spsparse_amd import capi
    d = torch.device("cuda:0")
    t = (torch.empty(n_tuples, dtype=torch.int32, device=d), torch.empty(n_tuples, dtype=torch.int32, device=d),
         torch.empty(n_tuples, dtype=torch.float64, device=d))
    gen(*[x.data_ptr() for x in t])
    torch.cuda.synchronize()
    return capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n_tuples, shape, sort0), t


def bits_differ(gv, wv):
    return gv.view(np.int64) != wv.view(np.int64)


def check_tuples(got, want, what, same=ar.same_tuples, differ=bits_differ):
    """Raise unless same(got, want); the message counts the tuples that differ (an index, or differ(values)) and shows the
    first of them."""
    if same(got, want):
        return
    gi, gj, gv = (np.asarray(x) for x in got)
    wi, wj, wv = (np.asarray(x) for x in want)
    if gi.shape != wi.shape:
        raise AssertionError("%s: %d tuples, want %d" % (what, gi.size, wi.size))
    bad = np.flatnonzero((gi != wi) | (gj != wj) | differ(gv, wv))
    k = bad[0]
    raise AssertionError("%s: %d tuples differ, first at %d: (%d, %d, %r) vs (%d, %d, %r)" % (
        what, bad.size, k, gi[k], gj[k], gv[k], wi[k], wj[k], wv[k]))


@contextlib.contextmanager
def forced(ctx, knob, value):
    """Set a path knob for the calls inside; always back to 0 (auto) after them."""
    ctx.set_tuning(knob, value)
    try:
        yield
    finally:
        ctx.set_tuning(knob, 0)


class Knobs:
    """Several tuning knobs for the calls inside; all of them back to 0 (their defaults) afterwards."""

    def __init__(self, ctx, knobs):
        self.ctx, self.knobs = ctx, knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            self.ctx.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            self.ctx.set_tuning(k, 0)


def check_digest(res, want, what):
    """A digest result against the digest of the oracle's tuples: count, hash and value sum, all exact (for values whose
    sums are exact in any order)."""
    from oracle import binding as orc
    cnt, vsum, h = orc.digest(*want[:3])
    assert (res.nnz, res.hash) == (cnt, h), "%s: digest sink: nnz %d hash %x, want %d %x" % (what, res.nnz, res.hash, cnt, h)
    assert res.sum == vsum, "%s: digest sink: sum %r, want %r" % (what, res.sum, vsum)


# ---- planned operands (tests/test_gpu_tile_shapes.py, tests/test_gpu_dense_cells.py)

def sink_flags(flag):
    from spsparse_amd import capi
    return {"plain": 0, "exact": capi.SINK_EXACT_PATTERN, "ordered": capi.SINK_ORDERED}[flag]


def operands(p, emit, keep):
    """(a, b, C, scalei, scalek) as C structs over the host arrays of a plan of tests/tile_plan.py."""
    from spsparse_amd import capi
    from tests import tile_plan as tp

    def vec(x):
        if x is None:
            return None
        s, k = capi.host_vec(x.idx, x.val, x.shape0)
        keep.append(k)
        return s
    a, ka = capi.host_coo(p.A.idx0, p.A.idx1, p.A.val, p.A.shape, p.A.sort0)
    b, kb = capi.host_coo(p.B.idx0, p.B.idx1, p.B.val, p.B.shape, p.B.sort0)
    keep += [ka, kb]
    C_, scalei, scalek = tp.emit_args(p.A, p.B, emit)
    return a, b, C_, vec(scalei), vec(scalek)


# ---- spsamd_solve_tri (tests/test_gpu_solve.py, tests/test_gpu_solve_wide.py)

SENT = -7.5          # what solve() fills X and the padding of B and X with


def bits_same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, "%s: %d values differ, first at %r: %r (%#x) vs %r (%#x)" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], got.view(np.uint64)[tuple(bad[0])],
        want[tuple(bad[0])], want.view(np.uint64)[tuple(bad[0])])


def solve(ctx, a, B, uplo=0, diag=0, t='.', pol=ar.ADD, zn=False, device=False, in_place=False, pad=1):
    """One solve through padded buffers (ld = nrhs + pad, the padding sentinel-filled and checked untouched).
    Returns (X as a host array, stats)."""
    B = np.ascontiguousarray(B, np.float64)
    n, nrhs = B.shape
    ld = nrhs + pad
    hb = np.full((n, ld), SENT)
    hb[:, :nrhs] = B
    hx = hb if in_place else np.full((n, ld), SENT)
    if device:
        import torch
        tb = torch.from_numpy(hb).cuda()
        tx = tb if in_place else torch.from_numpy(hx).cuda()
        torch.cuda.synchronize()
        _, st = ctx.solve_tri(a, tb[:, :nrhs], uplo, diag, t, X=tx[:, :nrhs], duplicate_policy=pol, zero_nan=zn, stats=True)
        gx, gb = tx.cpu().numpy(), tb.cpu().numpy()
    else:
        _, st = ctx.solve_tri(a, hb[:, :nrhs], uplo, diag, t, X=hx[:, :nrhs], duplicate_policy=pol, zero_nan=zn, stats=True)
        gx, gb = hx, hb
    assert np.all(gx[:, nrhs:] == SENT), "the padding of X was written"
    if not in_place:
        assert np.all(gb[:, nrhs:] == SENT) and np.array_equal(gb[:, :nrhs].view(np.int64), B.view(np.int64)), "B was written"
    return gx[:, :nrhs].copy(), st


def rhs(rng, n, nrhs, special=0.05):
    return ar._values(rng, n * nrhs, special).reshape(n, nrhs)


class PeakMemory:
    """Device memory in use (hipMemGetInfo, the whole device), sampled every millisecond on a thread."""

    def __enter__(self):
        import torch
        free, total = torch.cuda.mem_get_info(0)
        self.base = self.peak = total - free
        self.total, self.stop = total, False

        def poll():
            while not self.stop:
                free, total = torch.cuda.mem_get_info(0)
                self.peak = max(self.peak, total - free)
                time.sleep(0.001)
        self.t = threading.Thread(target=poll, daemon=True)
        self.t.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.t.join()


def threads():
    """Host threads for the oracle's full-size runs."""
    from oracle import binding as orc
    return max(1, min(orc.host_threads(), int(os.environ.get("OMP_NUM_THREADS") or 16)))


def build_cpp_test(name, tmp_path, opt="-O1"):
    """tests/cpp/test_<name>.cpp compiled and linked against the built library; returns the executable."""
    from spsparse_amd import build
    libdir = os.path.dirname(build.build())
    exe = os.path.join(str(tmp_path), "test_" + name)
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_%s.cpp" % name), "-o", exe, "-L" + libdir,
                           "-lspsparse_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe
