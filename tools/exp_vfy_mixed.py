"""What a batch of several gadgets costs at the bench's verify shape (secq256k1, 256 x 64-bit range proofs per statement: 2^14
multipliers; a "class" is that statement under another third parameter, which the verifier ignores: its own recording, the same
template; a few distinct proofs per class round-robin, proved before anything is timed):
  x  the crossover for BP_TUNE_VFY_CLASS_MIN: two interleaved classes of S members each, S = 8 .. 512, with the knob at 1 (both on
     the device) and at 65535 (the host replay of the same members), alternating;
  m  4096 instances as 2 and as 4 interleaved classes, without and with an 8-instance remainder (8 one-off statements), knob at 64
     and at 65535 (the host replay: what a build without the class path does with the batch);
  l  a like-instance batch of 4096;
  f  the like-instance batch with one malformed proof (both flag bits of A_I1 set).
Each figure: REPS batches, median [min .. max], milliseconds per batch.  Not part of the product and not run by the tests.

  python tools/exp_vfy_mixed.py [--only xmlf] [--tag NAME]     one JSON line per figure
  (--only lf and, with the host replay only, m: the legs that exist in a build without the class path — alternate the two builds)
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd import engine as E  # noqa: E402

REPS, DISTINCT, NVAL, NBITS = 7, 2, 256, 64
TUNE_VFY_CLASS_MIN = 24
SEED = bytes([5]) * 32


def ms(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(ts[0], 2), "max_ms": round(ts[-1], 2)}


def main():
    args = sys.argv[1:]
    only, tag = "xmlf", "this build"
    for flag in ("--only", "--tag"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            if flag == "--only":
                only = v
            else:
                tag = v
    e = A.Engine(curve=0)
    e.gens_derive(NVAL * NBITS)
    try:                                                   # (a library without the class path, loaded through ARKBP_LIB_PATH, lacks the symbol)
        e.vfe_class_stats()
        has_classes = True
    except AttributeError:
        has_classes = False

    def knob(v):
        if has_classes:
            e.set_tuning(TUNE_VFY_CLASS_MIN, v)

    def proved(third, n=DISTINCT):
        out = []
        for i in range(n):
            prm = [NVAL, NBITS, third]
            pr = e.prove_scenario(E.SC_MULTI_RANGE, prm, bytes([0x4D, third & 255, i]) + bytes(29), m_cap=NVAL + 8)
            out.append((E.SC_MULTI_RANGE, prm, pr.proof, pr.commitments, pr.publics))
        return out

    classes = [proved(c) for c in range(4)]
    oneoff = [proved(100 + j, 1)[0] for j in range(8)] if "m" in only else []
    head = {"build": tag, "reps": REPS}

    def interleaved(ncls, per_class, extra=()):
        inst = [classes[i % ncls][(i // ncls) % DISTINCT] for i in range(ncls * per_class)]
        step = max(1, len(inst) // (len(extra) + 1))
        for j, x in enumerate(extra):
            inst.insert((j + 1) * step, x)
        return inst

    def timed(inst, k):
        pk = E.pack_instances(inst)
        knob(k)
        c0 = e.vfe_class_stats() if has_classes else None
        assert e.batch_verify(pk, SEED)[0] == 0           # warm: sources, templates, class constants, allocations
        c1 = e.vfe_class_stats() if has_classes else None
        row = ms(lambda: e.batch_verify(pk, SEED))
        if has_classes:
            row["class_stats_of_one_call"] = [b - a for a, b in zip(c0, c1)]
        return row

    if "x" in only and has_classes:
        for S in (8, 16, 32, 64, 128, 256, 512):
            inst = interleaved(2, S)
            for rnd in range(2):                           # device, host, device, host
                for k, what in ((1, "device classes"), (65535, "host replay")):
                    print(json.dumps(dict(head, figure="x two classes of %d" % S, path=what, round=rnd, **timed(inst, k))), flush=True)
    if "m" in only:
        for ncls in (2, 4):
            for extra in ((), oneoff):
                inst = interleaved(ncls, 4096 // ncls, extra)
                for rnd in range(2):
                    for k, what in ((64, "device classes (knob 64)"), (65535, "host replay")):
                        if k == 64 and not has_classes:
                            continue
                        print(json.dumps(dict(head, figure="m 4096 as %d classes + %d one-off" % (ncls, len(extra)), path=what, round=rnd, **timed(inst, k))), flush=True)
    like = [classes[0][i % DISTINCT] for i in range(4096)]
    if "l" in only:
        for rnd in range(3):
            print(json.dumps(dict(head, figure="l 4096 like-instances", round=rnd, **timed(like, 0))), flush=True)
    if "f" in only:
        sc, prm, proof, cm, pb = like[1234]
        b = bytearray(proof)
        b[32] = 0xC0
        bad = list(like)
        bad[1234] = (sc, prm, bytes(b), cm, pb)
        pk = E.pack_instances(bad)
        knob(0)
        assert e.batch_verify(pk, SEED)[0] == -6
        for rnd in range(2):
            print(json.dumps(dict(head, figure="f 4096 like-instances, one malformed", round=rnd, **ms(lambda: e.batch_verify(pk, SEED)))), flush=True)
    e.close()


if __name__ == "__main__":
    main()
