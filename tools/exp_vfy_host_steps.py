"""Batch verification's host-replay route, for comparing two builds of the library (the other one through ARKBP_LIB_PATH):
  trace-host   a warm-up batch, then ONE mixed batch of 40 instances of three shapes (a multi-range, a range proof, a two-phase
               shuffle) with the device front end off: the process to put under rocprofv3 --kernel-trace --stats
  trace-dev    the same with 40 like-instances of the multi-range and the device front end on
  trace-2phase the same with 40 like-instances of the two-phase shuffle and BP_TUNE_VFY_DEVICE = 2
  trace-classes  the same with 40 interleaved instances of three single-phase shapes and BP_TUNE_VFY_CLASS_MIN = 1: three device classes
  replay       verifies per second of a 4096-instance batch of four interleaved gadgets at the bench's verify shape (256 x 64-bit range
               proofs per statement) with the device classes off: the host replay of every instance.  Median of 3 batches after a
               warm-up one; one JSON line with the median batch's timing[0..4].
  classes      the same batch with BP_TUNE_VFY_CLASS_MIN = 1: four device classes of 1024 members
Not part of the product and not run by the tests.

  python tools/exp_vfy_host_steps.py trace-host|trace-dev|trace-2phase|trace-classes|replay|classes [--tag NAME]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd import engine as E  # noqa: E402

TUNE_VFY_DEVICE, TUNE_VFY_CLASS_MIN = 11, 24
SEED = bytes([5]) * 32


def proved(e, sc, prm, n, m_cap=64):
    out = []
    for i in range(n):
        pr = e.prove_scenario(sc, prm, bytes([0x56, sc, i]) + bytes(29), m_cap=m_cap)
        out.append((sc, prm, pr.proof, pr.commitments, pr.publics))
    return out


def trace(e, mode):
    e.gens_derive(256)
    e.set_tuning(TUNE_VFY_DEVICE, {"trace-host": 0, "trace-2phase": 2}.get(mode, 1))
    if mode == "trace-classes":
        e.set_tuning(TUNE_VFY_CLASS_MIN, 1)
    multi = proved(e, E.SC_MULTI_RANGE, [3, 8, 0], 4)
    if mode == "trace-dev":
        inst = [multi[i % 4] for i in range(40)]
    elif mode == "trace-2phase":
        shuf = proved(e, E.SC_SHUFFLE, [4], 4)
        inst = [shuf[i % 4] for i in range(40)]
    elif mode == "trace-classes":
        two, rng = proved(e, E.SC_MULTI_RANGE, [2, 8, 0], 2), proved(e, E.SC_RANGE, [16, 77], 2)
        inst = [(multi[i % 4], two[i % 2], rng[i % 2], multi[i % 4])[i % 4] for i in range(40)]
    else:
        rng, shuf = proved(e, E.SC_RANGE, [16, 77], 2), proved(e, E.SC_SHUFFLE, [4], 2)
        inst = [multi[i % 4] for i in range(20)] + [rng[i % 2] for i in range(10)] + [shuf[i % 2] for i in range(10)]
    pk = E.pack_instances(inst)
    stats = lambda: list(e.vfe_stats()) + list(e.vfe_class_stats()) + list(e.commit_wire_stats())   # noqa: E731
    before = stats()
    for _ in range(2):   # warm-up, then the batch that is compared
        rc, tm, pt = e.batch_verify(pk, SEED, want_point=True)
        assert rc == 0, rc
    print(json.dumps({"mode": mode, "instances": len(inst), "vfe_class_wire_stats_delta": [int(b - a) for a, b in zip(before, stats())],
                      "check_point": [int(x) for x in pt]}))


def replay(e, tag, class_min=65535):
    nval, nbits = 256, 64
    e.gens_derive(nval * nbits)
    e.set_tuning(TUNE_VFY_CLASS_MIN, class_min)
    classes = [proved(e, E.SC_MULTI_RANGE, [nval, nbits, c], 2, m_cap=nval + 8) for c in range(4)]
    inst = [classes[i % 4][(i // 4) % 2] for i in range(4096)]
    pk = E.pack_instances(inst)
    assert e.batch_verify(pk, SEED)[0] == 0   # warm: sources, templates, allocations
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        rc, tm = e.batch_verify(pk, SEED)
        runs.append((time.perf_counter() - t0, list(tm)))
        assert rc == 0, rc
    runs.sort()
    wall, tm = runs[1]
    after = e.vfe_class_stats()
    print(json.dumps({"build": tag, "figure": ("host replay" if class_min == 65535 else "device classes") + ", 4096 instances of 4 gadgets", "vfe_class_stats": [int(x) for x in after], "verifies_per_s": 4096 / wall, "wall_s": [r[0] for r in runs],
                      "timing_of_median": {"total": tm[0], "host_busy": tm[1], "drain": tm[2], "msm": tm[3], "first_decode": tm[4]}}), flush=True)


def main():
    args = sys.argv[1:]
    tag = args[args.index("--tag") + 1] if "--tag" in args else "this build"
    e = A.Engine(curve=0)
    if args[0] in ("replay", "classes"):
        replay(e, tag, 65535 if args[0] == "replay" else 1)
    else:
        trace(e, args[0])
    e.close()


if __name__ == "__main__":
    main()
