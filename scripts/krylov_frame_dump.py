"""One dump of what spsamd_solve_pcg, spsamd_solve_bicgstab and spsamd_solve_pcg_amg return, to compare two checkouts:

    cd CHECKOUT && python PATH/TO/scripts/krylov_frame_dump.py OUT

loads the package and tests/ of the current directory (the checkout needs tests/test_gpu_krylov_frame.py for its systems).
The cases of that test, then Poisson 256^2 (tol 1e-8, at most 400 iterations, defaults) under every preconditioner, both
loops and both pcg_fuse values.  Per case one line: the sha256 (32 hex digits) of x's and the history's bytes, the first
eight history entries and bb, rr0, rr as hex words, every stats field but the times, nnz_a / nnz_b and workspace_bytes.
profiles/krylov_frame/ has two of them and their diff."""
import hashlib
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

from spsparse_amd import capi  # noqa: E402
from tests import krylov_ref as kr  # noqa: E402
from tests.gpu_util import Knobs, coo as _coo  # noqa: E402
from tests.test_gpu_krylov_frame import HOOK, LU, ORDERS, OWN, PARAMS, _system, _two_levels  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()[:32]


def hexes(a):
    return ",".join("%016x" % w for w in np.atleast_1d(np.asarray(a, np.float64)).view(np.uint64))


def main():
    out = open(sys.argv[1], "w")
    ctx = capi.Context(0)
    print("library", capi.__file__, file=sys.stderr)

    def case(name, a, f, levels, n, b, x0, loop, precond, tol, max_iter, cap):
        res, x = capi.Result(), np.array(x0, np.float64)
        if precond == HOOK:
            _, hist, st, ast = ctx.solve_pcg_amg(levels, PARAMS, b, x, tol, max_iter, cap, result=res)
            extra = " cycle %d" % ast.launches_per_cycle
        else:
            call = ctx.solve_pcg if loop == "pcg" else ctx.solve_bicgstab
            _, hist, st = call(a, b, x, precond, f if precond == LU else None, tol=tol, max_iter=max_iter, hist_capacity=cap, result=res)
            extra = ""
        out.write("%s | x %s hist %s [%s] | it %d reason %d bb %s rr0 %s rr %s launches %d readbacks %d analyses %d | nnz_a %d nnz_b %d workspace %d%s\n" % (
            name, sha(x), sha(hist), hexes(hist[:8]), st.iterations, st.reason, hexes(st.bb), hexes(st.rr0), hexes(st.rr), st.launches,
            st.readbacks, st.analyses, res.nnz_a, res.nnz_b, res.workspace_bytes, extra))
        out.flush()

    def operands(S, n, keep):
        a = _coo(S, (n, n), keep=keep)
        f = _coo(ctx.fetch(ctx.factor_ilu0(a)), (n, n), keep=keep)
        A0, P0, R0, A1 = (_coo(X, shape, keep=keep) for X, shape in _two_levels(S, n))
        return a, f, [(A0, '.', P0, '.', R0, '.'), (A1, '.', None, '.', None, '.')]

    for n in ORDERS:                                                     # the cases of tests/test_gpu_krylov_frame.py
        S, b = _system(n)
        keep = []
        a, f, levels = operands(S, n, keep)
        for (loop, precond) in OWN:
            for fuse in (0, 1):
                for max_iter in (3, 1):
                    with Knobs(ctx, {"pcg_check_every": 1, "pcg_fuse": fuse}):
                        case("n %d %s precond %d fuse %d max_iter %d" % (n, loop, precond, fuse, max_iter), a, f, levels, n, b, np.zeros(n),
                             loop, precond, 0.0, max_iter, 2)
    S, n = kr.poisson2d(256)                                             # Poisson 256^2, defaults, to convergence or 400 iterations
    b = np.bincount(S[0], weights=S[2], minlength=n)                      # A 1: small integers, exact in any order
    keep = []
    a, f, levels = operands(S, n, keep)
    for (loop, precond) in OWN:
        for fuse in (0, 1):
            with Knobs(ctx, {"pcg_fuse": fuse}):
                case("poisson256 %s precond %d fuse %d" % (loop, precond, fuse), a, f, levels, n, b, np.zeros(n), loop, precond, 1e-8, 400, None)
    ctx.close()
    out.close()


if __name__ == "__main__":
    main()
