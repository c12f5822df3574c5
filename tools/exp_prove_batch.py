"""Proofs/s of small statements: (a) one at a time on one ctx, (b) eight ctxs in flight on threads, (c) Engine.prove_batch.
k-shuffles; every rate twice: statement construction outside the timed region ("out") and inside it ("in": Statement(.., engine),
i.e. bp_stmt_prover_create_dev — the scenario's commitments are one GPU batch per statement).  cpu = host CPU seconds per proof.
The direct window tables are built on the first ctx and shared before anything is timed, and every ctx proves once first.

  python tools/exp_prove_batch.py [curve] [k ...]      the table (one JSON line per k)
  python tools/exp_prove_batch.py --one CURVE K B      one batch of B (for rocprofv3 --kernel-trace --stats), prints its host timing
  --front 0|1 anywhere on the line sets BP_TUNE_PROVE_BATCH_FRONT on every ctx (default: the library's, 1): 0 runs the stages in front of
  the inner-product argument one instance at a time.  Each (c) row also carries the front counters (instances, groups, host waits).
"""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd.engine import Statement  # noqa: E402

FRONT = None   # --front: BP_TUNE_PROVE_BATCH_FRONT (knob 14) for every ctx
STAGES = ["total", "lockstep_ipa", "rng", "upload", "commit", "flatten", "poly", "ipa_single"]


def stmts(e, k, n, tag):
    return [Statement(e.curve, 0, [k], bytes([tag, j & 255, j >> 8]) + bytes(29), e) for j in range(n)]


def engine(curve, gens=4096):
    e = A.Engine(curve=curve)
    e.gens_derive(gens)
    e.gens_direct_tables(gens)   # built here, so that share_gens_from hands them over
    return front(e)


def front(e):
    if FRONT is not None:
        e.set_tuning(14, FRONT)
    return e


def timed(fn):
    c0, t0 = time.process_time(), time.perf_counter()
    fn()
    return time.perf_counter() - t0, time.process_time() - c0


def one_batch(curve, k, B):
    e = engine(curve)
    for s in stmts(e, k, 2, 1):
        s.prove(e)
    s = stmts(e, k, B, 2)
    tm = [0.0] * 8
    wall, cpu = timed(lambda: e.prove_batch(s, timing=tm))
    print(json.dumps({"curve": curve, "k": k, "B": B, "wall_s": wall, "cpu_s": cpu, "stages_s": dict(zip(STAGES, tm)), "front": list(e.prove_batch_front_stats())}), flush=True)
    e.close()


def table(curve, ks):
    e = engine(curve)
    others = [front(A.Engine(curve=curve)) for _ in range(7)]
    for o in others:
        o.share_gens_from(e)
    engs = [e] + others
    for k in ks:
        for i, g in enumerate(engs):   # warm-up: first-use allocations of every ctx
            for s in stmts(g, k, 1, 100 + i):
                s.prove(g)
        n_a = 64 if k <= 128 else 16
        row = {"curve": curve, "k": k}
        s = stmts(e, k, n_a, 2)
        w, c = timed(lambda: [x.prove(e) for x in s])
        row["a_out"] = [round(n_a / w), round(1e3 * c / n_a, 3)]
        w, c = timed(lambda: [x.prove(e) for x in stmts(e, k, n_a, 3)])
        row["a_in"] = [round(n_a / w), round(1e3 * c / n_a, 3)]
        for inside in (False, True):
            per_n = n_a // 8
            per = None if inside else [stmts(g, k, per_n, 4 + i) for i, g in enumerate(engs)]

            def run(i, g):
                ss = stmts(g, k, per_n, 20 + i) if inside else per[i]
                for x in ss:
                    x.prove(g)

            def go():
                ths = [threading.Thread(target=run, args=(i, g)) for i, g in enumerate(engs)]
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()

            w, c = timed(go)
            row["b_in" if inside else "b_out"] = [round(8 * per_n / w), round(1e3 * c / (8 * per_n), 3)]
        for B in (64, 256, 1024):
            if k == 1024 and B > 256:
                continue
            s = stmts(e, k, B, 40)
            tm = [0.0] * 8
            res = []
            f0 = e.prove_batch_front_stats()
            w, c = timed(lambda: res.extend(e.prove_batch(s, timing=tm)))
            assert all(st == 0 for st, _ in res)
            row["c%d_out" % B] = [round(B / w), round(1e3 * c / B, 3)]
            row["c%d_front" % B] = [b - a for a, b in zip(f0, e.prove_batch_front_stats())]
            row["c%d_stages_ms_per_proof" % B] = {n: round(1e3 * t / B, 4) for n, t in zip(STAGES, tm)}
            w, c = timed(lambda: e.prove_batch(stmts(e, k, B, 41)))
            row["c%d_in" % B] = [round(B / w), round(1e3 * c / B, 3)]
        print(json.dumps(row), flush=True)
    for o in others:
        o.close()
    e.close()


if __name__ == "__main__":
    if "--front" in sys.argv:
        i = sys.argv.index("--front")
        FRONT = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one_batch(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 0, [int(x) for x in sys.argv[2:]] or [2, 16, 128, 1024])
