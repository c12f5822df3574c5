"""Many variable-base MSMs per call, resident operands, wall time per call in ms: (a) a loop of bp_msm_dev, (b) k_ve_tail on every job
(bp_msm_batch_dev with the short route forced: bp_debug_msm_each itself takes host operands, which would make this leg a PCIe test),
(c) bp_msm_batch_dev at the default knobs, (d) bp_msm_batch_dev with the bucketed route forced for every job (default slice
cap); and the slice sweep of (d).  (b) and (d) form groups whatever the job count; (c) is the call as a caller gets it.  Inputs
come from a seed (derived generators, random scalars below 2^254 as Montgomery words).  Every variant runs once untimed; then
REPS rounds in which the variants alternate, a host clock around each call (every call ends in a host wait for the GPU).  Reported as median [min .. max].  One more call per variant with profiling on gives the HIP-event time of k_ve_tail and of
k_msb_accum + k_msb_combine.  Not part of the product and not run by the tests.

  python tools/exp_msm_batch.py [curve ...]                 the table (default: curves 0 1), one JSON line per shape
  python tools/exp_msm_batch.py --shape COUNT TERMS [curve] one shape
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd import engine as E  # noqa: E402

REPS, SEED, POOL = 5, 20260818, 512
SHAPES = [(256, n) for n in (17, 64, 128, 300, 1024, 2081, 8192)] + [(8, n) for n in (300, 2081, 8192)] + [(1, 2081)]
# what the defaults of the short cap (256 short jobs), of the least job count (2 .. 6 jobs) and of the longest bucketed job rest on
EXTRA_SHAPES = [(256, n) for n in (2, 4, 8, 12)] + [(c, n) for c in (2, 4, 6) for n in (300, 2081)] + [(8, 4096), (256, 4096)]
SWEEP_SHAPES, SWEEP = [(256, 2081), (8, 2081)], (64, 128, 256, 512)
HUGE = 1 << 31
K_VE_TAIL = 15


def knobs(e, short, slice_terms, batch_max, min_jobs):
    e.set_tuning(E.TUNE_MSM_BATCH_SHORT, short)
    e.set_tuning(E.TUNE_MSM_BATCH_SLICE, slice_terms)
    e.set_tuning(E.TUNE_MSM_BATCH_MAX, batch_max)
    e.set_tuning(E.TUNE_MSM_BATCH_MIN_JOBS, min_jobs)


def fmt(ts):
    ms = sorted(1e3 * t for t in ts)
    return {"median": round(statistics.median(ms), 3), "min": round(ms[0], 3), "max": round(ms[-1], 3)}


def shape(e, pool, count, terms, sweep):
    rs = np.random.RandomState((SEED + 131 * count + terms) & 0x7FFFFFFF)
    n = count * terms
    bases = pool[rs.randint(0, len(pool), size=n)]
    scal = rs.randint(0, 1 << 62, size=(n, 4), dtype=np.uint64)   # < 2^254: below both moduli
    d_b, d_s = e.upload_points(bases), e.upload_scalars(scal)
    lengths = [terms] * count

    def loop():
        return [e.msm_dev(_View(d_b, 64 * j * terms), _View(d_s, 32 * j * terms), terms) for j in range(count)]

    def batch(short, slice_terms, batch_max, min_jobs=1):
        def run():
            knobs(e, short, slice_terms, batch_max, min_jobs)
            return e.msm_batch_dev(d_b, d_s, lengths)
        return run

    variants = [("a_msm_dev_loop", loop), ("b_ve_tail", batch(HUGE, 0, 0)), ("c_batch_default", batch(0, 0, 0, 0)), ("d_bucketed", batch(1, 0, HUGE))]
    if sweep:
        variants += [("d_slice_%d" % s, batch(1, s, HUGE)) for s in SWEEP]
    ref = np.stack(variants[0][1]())
    for name, fn in variants[1:]:   # untimed first run; all variants compute the same points
        assert (fn() == ref).all(), name
    times = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    row = {"curve": e.curve, "jobs": count, "terms": terms, "reps": REPS, "wall_ms": {name: fmt(ts) for name, ts in times.items()}}
    kt = {}
    e.set_profiling(True)
    for name, fn in variants[1:]:
        e.reset_profiling()
        fn()
        kt[name] = {"k_ve_tail": round(e.kernel_time(K_VE_TAIL)[0], 3), "k_msb": round(e.kernel_time(E.K_MSM_BATCH)[0], 3)}
    e.set_profiling(False)
    knobs(e, 0, 0, 0, 0)
    row["kernel_ms"] = kt
    d_b.free()
    d_s.free()
    return row


class _View:
    """a DeviceBuffer seen from a byte offset (for the bp_msm_dev loop over one resident array)"""

    def __init__(self, buf, off):
        import ctypes as C

        self.ptr = C.c_void_p(buf.ptr.value + off)


def main():
    args = sys.argv[1:]
    shapes, sweeps = SHAPES + EXTRA_SHAPES, SWEEP_SHAPES
    if args and args[0] == "--shape":
        shapes, sweeps = [(int(args[1]), int(args[2]))], []
        args = args[3:]
    print("# one run on one MI355X; wall ms per call, median [min .. max] of %d alternating repetitions; defaults %s" % (REPS, (E.MSM_BATCH_DEFAULTS,)), flush=True)
    for curve in [int(x) for x in args] or [0, 1]:
        e = A.Engine(curve=curve)
        pool = E.host_derive_generators(curve, 0, 0, POOL)
        for count, terms in shapes:
            row = shape(e, pool, count, terms, (count, terms) in sweeps)
            print(json.dumps(row), flush=True)
            for name, v in row["wall_ms"].items():
                k = row["kernel_ms"].get(name, {})
                print("#   curve %d  %4d x %-5d %-16s %9.3f [%9.3f .. %9.3f]   k_ve_tail %8.3f  k_msb %8.3f" % (
                    curve, count, terms, name, v["median"], v["min"], v["max"], k.get("k_ve_tail", 0.0), k.get("k_msb", 0.0)), flush=True)
        e.close()


if __name__ == "__main__":
    main()
