"""All ranks of one communicator in ONE process: a thread per rank, each with a context and an spsamd_dist of its own on
device 0, and a live all-to-allv between the threads as the step's transport callback.  ctypes releases the GIL inside
spsamd_dist_multiply and takes it back in the callback, so the ranks' steps really interleave: every rank runs the C
code a multi-GPU run executes, at any world size up to MAX_WORLD, and the transport sees -- and records -- what each
rank sends.  `copy` is a parameter: with ctypes.memmove the same exchange runs on host memory (tests/test_dist_host.py).

One call of the transport (one segment of a round), on every rank:
    publish (send, sendb, recvb); wait for all ranks;
    check the size agreement sendb_p[me] == recvb_me[p] for every peer p (RCCL would hang on a mismatch);
    copy every peer's buffer for this rank into its receive buffer; wait for all ranks (send buffers may be reused).
An exception on any rank aborts the barrier: every rank's callback then fails, the step ends with SPSAMD_EHIP everywhere.

TIMEOUT is a guard against a hang, three orders above a step's milliseconds -- not a measurement.  A thread that does
not come back is an error, and nothing more is started by this module afterwards.
Importing it needs no GPU."""
import threading
import time

import numpy as np

TIMEOUT = 60.0

_hung = []          # names of rank threads that never came back: run_ranks refuses from then on


class SizeMismatch(RuntimeError):
    """Two ranks disagree on the bytes of one buffer."""


class PlantedFailure(RuntimeError):
    """Raised by the transport where a test asked for it (Exchange(fail=...))."""


class RankHung(RuntimeError):
    """A rank's thread did not come back within the timeout."""


class Exchange:
    """The shared state of one communicator's transport.  log[rank][call][peer]: a host copy (bytes) of what `rank`
    handed to the transport for `peer` in its call number `call`.  fail(rank, call) -> True: the transport raises there."""

    def __init__(self, world, fail=None, timeout=TIMEOUT):
        self.world, self.fail, self.timeout = world, fail, timeout
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.log = [[] for _ in range(world)]
        self.errors = [[] for _ in range(world)]

    def abort(self):
        self.barrier.abort()

    def transport(self, rank, copy, to_host):
        """The callable capi.Dist takes for `rank`.  copy(dst, src, nbytes) moves a buffer; to_host(src, nbytes) -> bytes."""
        W = self.world

        def xfer(send, sendb, recv, recvb, _stream=None):
            call = len(self.log[rank])
            try:
                sendb_, recvb_ = [int(x) for x in sendb], [int(x) for x in recvb]
                self.log[rank].append([to_host(send[p], sendb_[p]) if sendb_[p] else b"" for p in range(W)])
                if self.fail is not None and self.fail(rank, call):
                    raise PlantedFailure("rank %d, call %d" % (rank, call))
                self.slots[rank] = (list(send), sendb_, recvb_)
                self.barrier.wait(self.timeout)
                for p in range(W):
                    if self.slots[p][1][rank] != recvb_[p]:
                        raise SizeMismatch("call %d: rank %d sends %d bytes to rank %d, which expects %d"
                                           % (call, p, self.slots[p][1][rank], rank, recvb_[p]))
                for p in range(W):
                    if recvb_[p]:
                        copy(recv[p], self.slots[p][0][rank], recvb_[p])
                self.barrier.wait(self.timeout)
            except BaseException as e:
                self.errors[rank].append(e)
                self.barrier.abort()
                raise
        return xfer


class Ranks:
    """What run_ranks returns: values[rank] (fn's return value, None where it raised) and errors[rank] (the exception, or
    None)."""

    def __init__(self, world):
        self.values, self.errors = [None] * world, [None] * world

    def raise_first(self):
        """Re-raise the most telling error: one that is no broken barrier or transport failure if there is any."""
        errs = [(r, e) for r, e in enumerate(self.errors) if e is not None]
        if not errs:
            return
        errs.sort(key=lambda re: (isinstance(re[1], threading.BrokenBarrierError) or "transport failed" in str(re[1]), re[0]))
        r, e = errs[0]
        raise AssertionError("rank %d of %d failed (%d ranks in all): %s: %s" % (r, len(self.errors), len(errs), type(e).__name__, e)) from e


def run_ranks(world, fn, timeout=TIMEOUT, copy=None, exchange=None, also_abort=()):
    """fn(rank, ctx, dd) on `world` threads; returns a Ranks.
    copy=None: every thread makes its own capi.Context(0) and capi.Dist(ctx, rank, world, transport=...), buffers are device
    memory moved with ctx.memcpy, and both are closed when fn returns.  copy given (ctypes.memmove): host memory, no GPU --
    ctx is None and dd is the rank's transport callable itself.
    exchange: an Exchange made by the caller (to plant a failure or read its log); also_abort: further Exchange objects fn
    uses, aborted with the first one when a rank fails outside the transport, so that no peer waits for it."""
    if _hung:
        raise RankHung("an earlier run left threads behind (%s): nothing more is started" % ", ".join(_hung))
    ex = exchange if exchange is not None else Exchange(world, timeout=timeout)
    out = Ranks(world)
    if copy is None:
        from spsparse_amd import capi
        capi.load()                                         # once, before the threads race for it

    def host_bytes(src, n):
        import ctypes
        return ctypes.string_at(src, n)

    def body(rank):
        ctx = dd = None
        try:
            if copy is None:
                from spsparse_amd import capi
                ctx = capi.Context(0)
                dd = capi.Dist(ctx, rank, world, transport=ex.transport(
                    rank, ctx.memcpy, lambda src, n, c=ctx: c.to_host(src, n, np.uint8).tobytes()))
            else:
                dd = ex.transport(rank, copy, host_bytes)
            out.values[rank] = fn(rank, ctx, dd)
        except BaseException as e:
            out.errors[rank] = e
            ex.abort()
            for x in also_abort:
                x.abort()
        finally:
            try:
                if copy is None and dd is not None:
                    dd.close()
                if ctx is not None:
                    ctx.close()
            except BaseException as e:                      # (a close that fails after a failed step)
                out.errors[rank] = out.errors[rank] or e

    threads = [threading.Thread(target=body, args=(r,), name="rank%d" % r, daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    left = [t.name for t in threads if t.is_alive()]
    if left:
        ex.abort()
        _hung.extend(left)
        raise RankHung("threads %s did not come back within %g s" % (", ".join(left), timeout))
    return out
