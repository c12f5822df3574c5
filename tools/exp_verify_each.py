"""Verdicts/s for many small proofs: (a) a bp_r1cs_verify_scenario loop on one ctx, (b) eight ctxs on eight threads sharing the
tables, (c) bp_r1cs_verify_each_scenarios (one call, a verdict per instance), (d) for scale only: bp_r1cs_batch_verify_scenarios of
the same all-valid batch (ONE verdict).  B distinct k-shuffle proofs per batch, proved before anything is timed; every ctx verifies
once first (tables, templates, first-use allocations).  Not part of the product and not run by the tests.

  python tools/exp_verify_each.py [curve] [k ...]          one JSON line per k: median verdicts/s of REPS batches and the spread
  python tools/exp_verify_each.py --only abd [curve] [k ..]   the legs that exist in a build without the new call (a parent build, for
                                                              alternating the two builds); --only c: the new call alone
  python tools/exp_verify_each.py --one CURVE K B           one call of (c) (for rocprofv3 --kernel-trace --stats, ARKBP_VFY_TRACE=1)
"""
import json
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd import engine as E  # noqa: E402

B, REPS = 256, 5
TIMING = ["total", "replay", "gpu_waits", "single_route", "decode"]


def gens_for(k):
    n = 2
    while n < max(2, 2 * (k - 1)):
        n *= 2
    return n


def pool(e, k, n):
    out = []
    for j in range(n):
        pr = e.prove_scenario(0, [k], bytes([0x5E, j & 255, j >> 8]) + bytes(29))
        out.append((0, [k], pr.proof, pr.commitments, pr.publics))
    return out


def rate(fn, n):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    r = sorted(n / t for t in ts)
    return {"median": round(statistics.median(r)), "min": round(r[0]), "max": round(r[-1])}


def table(curve, ks, only):
    for k in ks:
        g = max(gens_for(k), 16)
        e = A.Engine(curve=curve)
        e.gens_derive(g)
        e.gens_direct_tables(g)
        inst = pool(e, k, B)
        row = {"curve": curve, "k": k, "B": B, "reps": REPS}
        if "a" in only:
            e.verify_scenario(*inst[0])
            row["a_loop"] = rate(lambda: [e.verify_scenario(*i) for i in inst], B)
        if "b" in only:
            others = [A.Engine(curve=curve) for _ in range(7)]
            for o in others:
                o.share_gens_from(e)
            engs = [e] + others
            for x in engs:
                x.verify_scenario(*inst[0])
            per = B // 8

            def go():
                ths = [threading.Thread(target=lambda i=i, x=x: [x.verify_scenario(*q) for q in inst[i * per:(i + 1) * per]]) for i, x in enumerate(engs)]
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()

            row["b_8ctx"] = rate(go, 8 * per)
            for o in others:
                o.close()
        if "c" in only:
            pk = E.PackedInstances(inst)
            rc, st = e.verify_each_scenarios(pk)
            assert rc == 0 and st == [0] * B
            tm = [0.0] * 5
            row["c_each"] = rate(lambda: e.verify_each_scenarios(pk, timing=tm), B)
            row["c_last_call_ms"] = {n: round(1e3 * t, 3) for n, t in zip(TIMING, tm)}
            row["c_stats"] = list(e.verify_each_stats())
        if "d" in only:
            pk = E.PackedInstances(inst)
            seed = bytes([7]) * 32
            assert e.batch_verify(pk, seed)[0] == 0
            row["d_batch_one_verdict"] = rate(lambda: e.batch_verify(pk, seed), B)
        print(json.dumps(row), flush=True)
        e.close()


def one(curve, k, n):
    g = max(gens_for(k), 16)
    e = A.Engine(curve=curve)
    e.gens_derive(g)
    e.gens_direct_tables(g)
    pk = E.PackedInstances(pool(e, k, n))
    e.verify_each_scenarios(pk)
    tm = [0.0] * 5
    e.set_profiling(True)
    t0 = time.perf_counter()
    rc, st = e.verify_each_scenarios(pk, timing=tm)
    wall = time.perf_counter() - t0
    kt = {name: e.kernel_time(i) for name, i in (("k_vfy_tables", 11), ("k_vfy_batch", 5), ("table_sums", 0), ("k_ve_tail", 15))}
    print(json.dumps({"curve": curve, "k": k, "B": n, "rc": rc, "wall_ms": round(1e3 * wall, 3), "timing_ms": {a: round(1e3 * t, 3) for a, t in zip(TIMING, tm)},
                      "kernel_ms": {a: round(v[0], 3) for a, v in kt.items()}}), flush=True)
    e.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    only = "abcd"
    if "--only" in args:
        i = args.index("--only")
        only = args[i + 1]
        del args[i:i + 2]
    if args and args[0] == "--one":
        one(int(args[1]), int(args[2]), int(args[3]))
    else:
        table(int(args[0]) if args else 0, [int(x) for x in args[1:]] or [2, 16, 128, 1024], only)
