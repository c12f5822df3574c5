"""What naming the failing proofs costs at the bench's verify shape (secq256k1, 256 x 64-bit range proofs per statement: 2^14
multipliers, B statements per batch built from a few distinct proofs round-robin, proved before anything is timed):
  (a) bp_r1cs_batch_verify_scenarios on the all-valid batch (ONE verdict),
  (b) bp_r1cs_batch_verify_locate_scenarios on the all-valid batch,
  (c) the same with 1, 8 and 64 bad proofs at random positions (one byte of t_x changed), with the passes and the instances in them,
      at BP_TUNE_VERIFY_LOCATE_LEAF = 1, 8 and 64,
  (d) a bp_r1cs_verify_scenario loop (bp_verifier_verify for scenario statements) over 256 of the instances, scaled to the batch.
Five batches per figure: median [min .. max], milliseconds per batch.  Not part of the product and not run by the tests.

  python tools/exp_verify_locate.py [--only abcd] [--batch B] [--tag NAME]     one JSON line per figure
  (--only ad: the legs that exist in a build without the new call — a parent build, for alternating the two builds)
"""
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd import engine as E  # noqa: E402

REPS, DISTINCT, NVAL, NBITS = 5, 4, 256, 64
T_X = 11 * 33
TUNE_VERIFY_LOCATE_LEAF = 22


def ms(fn):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(ts[0], 2), "max_ms": round(ts[-1], 2)}


def main():
    args = sys.argv[1:]
    only, B, tag = "abcd", 512, "this build"
    for flag in ("--only", "--batch", "--tag"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            if flag == "--only":
                only = v
            elif flag == "--batch":
                B = int(v)
            else:
                tag = v
    e = A.Engine(curve=0)
    e.gens_derive(NVAL * NBITS)
    prm = [NVAL, NBITS, 0]
    distinct = []
    for i in range(DISTINCT):
        pr = e.prove_scenario(E.SC_MULTI_RANGE, prm, bytes([0x4C, i]) + bytes(30), m_cap=NVAL + 8)
        distinct.append((E.SC_MULTI_RANGE, prm, pr.proof, pr.commitments, pr.publics))
    valid = [distinct[i % DISTINCT] for i in range(B)]
    seed = bytes([5]) * 32
    head = {"build": tag, "batch": B, "reps": REPS}
    pk = E.pack_instances(valid)
    assert e.batch_verify(pk, seed)[0] == 0           # warm: templates, first-use allocations
    if "a" in only:
        print(json.dumps(dict(head, figure="a batch_verify, all valid", **ms(lambda: e.batch_verify(pk, seed)))), flush=True)
    if "b" in only:
        rc, st = e.batch_verify_locate(pk, seed)
        assert rc == 0 and st == [0] * B
        tm = [0.0] * 4
        row = ms(lambda: e.batch_verify_locate(pk, seed, timing=tm))
        print(json.dumps(dict(head, figure="b locate, all valid", last_call_ms=[round(1e3 * t, 2) for t in tm], **row)), flush=True)
    if "c" in only:
        rnd = random.Random(2011)
        for nbad in (1, 8, 64):
            bad = sorted(rnd.sample(range(B), nbad))
            inst = list(valid)
            for j in bad:
                sc, p, proof, cm, pb = inst[j]
                b = bytearray(proof)
                b[T_X] ^= 1 + (j % 7)
                inst[j] = (sc, p, bytes(b), cm, pb)
            pkb = E.pack_instances(inst)
            want = [-4 if j in set(bad) else 0 for j in range(B)]
            for leaf in (1, 8, 64):
                e.set_tuning(TUNE_VERIFY_LOCATE_LEAF, leaf)
                s0 = e.verify_locate_stats()
                rc, st = e.batch_verify_locate(pkb, seed)
                s1 = e.verify_locate_stats()
                assert st == want and rc == -4
                tm = [0.0] * 4
                row = ms(lambda: e.batch_verify_locate(pkb, seed, timing=tm))
                print(json.dumps(dict(head, figure="c locate, %d bad" % nbad, leaf=leaf, passes=s1[1] - s0[1], instances_in_passes=s1[2] - s0[2],
                                      exact=s1[3] - s0[3], last_call_ms=[round(1e3 * t, 2) for t in tm], **row)), flush=True)
            e.set_tuning(TUNE_VERIFY_LOCATE_LEAF, 0)
    if "d" in only:
        n = min(256, B)
        assert e.verify_scenario(*valid[0]) == 0
        row = ms(lambda: [e.verify_scenario(*i) for i in valid[:n]])
        row = {k: round(v * B / n, 1) for k, v in row.items()}
        print(json.dumps(dict(head, figure="d verify loop over %d, scaled to the batch" % n, **row)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
