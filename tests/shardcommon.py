"""Ranks as threads (shared by the sharded GPU tests): `world` threads of the test process, one Engine each on the same GPU, in the
window-sharded mode of include/arkbp.h bp_ctx_set_window_shard / bp_ctx_set_shard_allgather through
parallel.enable_window_sharding, their two collectives served by a barrier over a shared slot array.

What run_ranks adds to the copies in tests/test_gpu_prove.py:
  * every barrier wait is bounded (WAIT_S: a cap, not a measurement — the legs finish in seconds).  Ranks that make different
    collectives, or a rank that returns while another still waits for it, fail the test instead of hanging the suite: the wait
    raises inside the Python callback, Engine.set_window_shard / set_shard_allgather turn that into a non-zero return to the
    library, the call fails on that rank and the barrier is aborted for the others;
  * a log per rank of every collective, ("point", 8) for a point-reduce (8 words) and ("vector", nbytes) for the vector gather of
    the index-cyclic inner-product argument; all ranks must have logged the same sequence.  (A gathered block is never 64 bytes: a
    rank sends at least one element of a and b, 32 bytes each, and of G and H, 64 bytes each.)  Blocks that differ in shape between
    the ranks are an error, never padded;
  * sharding is switched off before the ctx is destroyed, on the error path too."""
import threading
import time

import numpy as np

WAIT_S = 120
TUNE_IPA_FREEZE_LEN, TUNE_CYCLIC_MIN = 2, 4          # include/arkbp.h BP_TUNE_IPA_FREEZE_LEN, BP_TUNE_CYCLIC_MIN
DEFAULT_KNOBS = {TUNE_CYCLIC_MIN: 16, TUNE_IPA_FREEZE_LEN: 4}   # the inner-product arguments of 16- to 128-element statements go cyclic
_DONE = "done"


class Run(list):
    """body's result per rank; .log: the collectives every rank made, in order (one list: the ranks' logs are equal); .logs: per rank"""


def points(log):
    return sum(1 for kind, _ in log if kind == "point")


def vectors(log):
    return sum(1 for kind, _ in log if kind == "vector")


def run_ranks(world, curve, body, gens=128, knobs=None, setup=None, share_from=None):
    """Runs body(rank, engine) on `world` rank threads and returns a Run of its results.  Each engine derives `gens` generators (or
    shares those of `share_from`, tables included), runs setup(rank, engine) if given — still unsharded —, is sharded as rank `rank`
    of `world` and takes DEFAULT_KNOBS overlaid with `knobs` ({knob: value}).  engine.shard_log is the rank's log so far: a body
    reads its length to count the collectives of one call.  Raises the first error of any rank."""
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd import parallel as P

    bar = threading.Barrier(world)
    slots, out, errors = [None] * world, [None] * world, []
    logs = [[] for _ in range(world)]
    tune = dict(DEFAULT_KNOBS)
    tune.update(knobs or {})

    def exchange(rank, item):
        """every rank deposits item; returns all of them once all have (two bounded waits: the slots are read between them)"""
        slots[rank] = item
        t0 = time.monotonic()
        try:
            bar.wait(WAIT_S)
            got = list(slots)
            bar.wait(WAIT_S)
        except threading.BrokenBarrierError:
            if time.monotonic() - t0 >= WAIT_S - 1:
                raise TimeoutError("rank %d waited %d s for the other ranks (%r): the ranks' collectives have diverged" % (rank, WAIT_S, item if isinstance(item, str) else logs[rank][-1]))
            raise
        return got

    def run(rank):
        e = None
        try:
            e = A.Engine(curve=curve)
            if share_from is not None:
                e.share_gens_from(share_from)
            else:
                e.gens_derive(gens)
            if setup is not None:
                setup(rank, e)
            e.shard_log = logs[rank]

            def allgather(arr):
                a = np.array(arr, copy=True)
                logs[rank].append(("point", 8) if a.size == 8 else ("vector", int(a.nbytes)))
                got = exchange(rank, a)
                if any(isinstance(g, str) for g in got):
                    raise RuntimeError("rank %d is in a collective (%r) while another rank has finished" % (rank, logs[rank][-1]))
                if any(g.shape != a.shape for g in got):
                    raise RuntimeError("the ranks' blocks differ in shape: %r" % ([g.shape for g in got],))
                return np.stack(got)

            P.enable_window_sharding(e, curve, E.host_points_sum, rank, world, allgather=allgather)
            for knob, value in sorted(tune.items()):
                e.set_tuning(knob, value)
            out[rank] = body(rank, e)
            if not all(isinstance(g, str) for g in exchange(rank, _DONE)):
                raise RuntimeError("rank %d has finished while another rank is in a collective" % rank)
        except BaseException as ex:   # (an assertion of the body included)
            cb = (getattr(e, "_shard_errors", None) or []) + (getattr(e, "_gather_errors", None) or []) if e is not None else []
            errors.append((rank, ex, cb))
            bar.abort()
        finally:
            if e is not None:
                try:
                    P.enable_window_sharding(e, curve, E.host_points_sum, 0, 1)
                finally:
                    e.close()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errors:
        # the cause first: a rank whose barrier was broken by another rank's failure only followed it
        errors.sort(key=lambda x: (isinstance(x[1], threading.BrokenBarrierError) or any(isinstance(c, threading.BrokenBarrierError) for c in x[2]), x[0]))
        rank, ex, cb = errors[0]
        raise AssertionError("rank %d of %d: %r (in its callbacks: %r); all: %r" % (rank, world, ex, cb, [(r, repr(x)) for r, x, _ in errors])) from ex
    for r in range(1, world):
        assert logs[r] == logs[0], "rank %d made other collectives than rank 0: %r vs %r" % (r, logs[r][:40], logs[0][:40])
    res = Run(out)
    res.log, res.logs = logs[0], logs
    return res
