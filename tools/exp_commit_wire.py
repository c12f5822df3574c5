"""What the commitments cost a verifying service that receives them as 33-byte encodings (secq256k1, the bench's verify statement:
256 x 64-bit range proofs, m = 256 commitments, 2^14 multipliers; B like-instances through bp_verifier_new_like, built from a few
distinct proofs round-robin and proved before anything is timed; one more verifier with m = 1 through bp_verifier_verify, which
always takes the prologue).

  parent path   decode every commitment on the CPU with the oracle's restatement of the reference (point_deser_compressed), on one
                core and on --threads worker processes (started before the GPU is opened; they never touch it); then
                bp_verifier_commit per verifier; then bp_r1cs_batch_verify (twice, on fresh handles: the spread between the two
                calls is the noise of the comparison below)
  new path      bp_verifier_commit_compressed_batch(defer = 1); then bp_r1cs_batch_verify (twice as well)

Per stage: wall seconds and host CPU seconds (user + system time of the process, all its threads, and of the workers it has
reaped — what tools/thread_cpu.py samples per thread from outside).  The counters of bp_ctx_commit_wire_stats show which route
decoded.  One JSON line per figure.  Not part of the product and not run by the tests.

  python tools/exp_commit_wire.py [--batch B] [--threads T]
"""
import json
import os
import sys
import time
import multiprocessing

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_bulletproofs_amd as A  # noqa: E402
from ark_bulletproofs_amd import engine as E  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

CV, DISTINCT, NVAL, NBITS = 0, 4, 256, 64
LABEL = b"MultiRangeBenchmark"       # the scenario's transcript label: the proofs come from the scenario prover
K_VFE_POINTS, K_VFE_SPONGE = 12, 13   # BP_K_VFE_POINTS, BP_K_VFE_SPONGE (include/arkbp.h)
ONE_VAR = (4, 0)


def staged(fn):
    w0, c0 = time.perf_counter(), sum(os.times()[:4])
    out = fn()
    return out, {"wall_s": round(time.perf_counter() - w0, 4), "host_cpu_s": round(sum(os.times()[:4]) - c0, 4)}


def decode_chunk(chunk):
    return sum(O.point_deser_compressed(CV, chunk[i:i + 33]) is not None for i in range(0, len(chunk), 33))


def record_range(v, words, vars_, nbits):
    """the scenario's range gadget per committed value (host_proto.hpp range_gadget), through the bulk recording calls"""
    one, mone, mpow = words
    for var in vars_:
        first = v.allocate_multipliers(count=nbits)
        vv, cc, off = [], [], [0]
        for i in range(nbits):
            vv += [(3, first + i)]; cc += [one]; off.append(len(vv))
            vv += [(1, first + i), (2, first + i), ONE_VAR]; cc += [one, one, mone]; off.append(len(vv))
        vv += [var] + [(2, first + i) for i in range(nbits)]
        cc += [one] + [mpow[i] for i in range(nbits)]
        off.append(len(vv))
        v.constrain_many(np.array(vv, dtype=np.uint32), np.stack(cc), off)


def main():
    args = sys.argv[1:]
    B, threads = 4096, 16
    for flag in ("--batch", "--threads"):
        if flag in args:
            i = args.index(flag)
            val = int(args[i + 1])
            del args[i:i + 2]
            if flag == "--batch":
                B = val
            else:
                threads = val
    fr = O.fid(CV, True)
    p = O.modulus(fr)
    words = (O.fe_from_int(fr, 1), O.fe_from_int(fr, p - 1), [O.fe_from_int(fr, p - (1 << i)) for i in range(NBITS)])
    workers = multiprocessing.get_context("spawn").Pool(threads)
    workers.map(decode_chunk, [b""] * threads)     # started and imported before anything is timed
    e = A.Engine(curve=CV)
    e.gens_derive(NVAL * NBITS)
    distinct, small = [], None
    for i in range(DISTINCT):
        pr = e.prove_scenario(E.SC_MULTI_RANGE, [NVAL, NBITS, 0], bytes([0x57, i]) + bytes(30), m_cap=NVAL + 8)
        V = np.asarray(pr.commitments, dtype=np.uint64).reshape(-1, 8)
        distinct.append((pr.proof, V, E.points_compress(CV, V)))
    pr = e.prove_scenario(E.SC_MULTI_RANGE, [1, NBITS, 0], bytes([0x58]) * 32, m_cap=16)
    V1 = np.asarray(pr.commitments, dtype=np.uint64).reshape(-1, 8)
    small = (pr.proof, V1, E.points_compress(CV, V1))
    proofs = [distinct[k % DISTINCT][0] for k in range(B)]
    blobs = [distinct[k % DISTINCT][2] for k in range(B)]
    alphas = O.fe_rand(fr, bytes([6]) * 32, B)
    head = {"batch": B, "m": NVAL, "threads": threads}

    def handles(commit):
        """v0 records the gadget, the rest are like-instances; commit(list of verifiers) gives every one its commitments"""
        v0 = E.VerifierCS(CV, E.HostTranscript(LABEL))
        commit([v0], 0)
        record_range(v0, words, [(0, j) for j in range(NVAL)], NBITS)
        rest = [E.VerifierCS(CV, E.HostTranscript(LABEL), like=v0) for _ in range(B - 1)]
        _, row = staged(lambda: commit(rest, 1))
        return [v0] + rest, row

    def verify(vs, what):
        e.reset_profiling(); e.set_profiling(True)
        d0, c0 = e.vfe_stats(), e.commit_wire_stats()
        (rc, pt), row = staged(lambda: E.batch_verify_cs(e, vs, proofs, alphas, want_point=True))
        d1, c1 = e.vfe_stats(), e.commit_wire_stats()
        e.set_profiling(False)
        assert rc == 0 and not pt.any(), (what, rc)
        kms = {"k_vfe_points_ms": round(e.kernel_time(K_VFE_POINTS)[0], 3), "k_vfe_sponge_ms": round(e.kernel_time(K_VFE_SPONGE)[0], 3)}
        print(json.dumps(dict(head, figure=what, device_batches=d1[0] - d0[0], fallbacks=d1[1] - d0[1], **kms, wire_by_front_end=c1[0] - c0[0], wire_by_prologue_gpu=c1[1] - c0[1], wire_on_host=c1[2] - c0[2], **row)), flush=True)
        return row["wall_s"]

    # ---- parent path
    pts, row = staged(lambda: [O.point_deser_compressed(CV, b[33 * j:33 * j + 33]) for b in blobs for j in range(NVAL)])
    print(json.dumps(dict(head, figure="parent: CPU decode of every commitment, one core", us_per_root=round(1e6 * row["wall_s"] / (B * NVAL), 2), **row)), flush=True)

    def decode_parallel():
        n = sum(workers.map(decode_chunk, blobs, chunksize=max(1, B // (4 * threads))))
        workers.close(); workers.join()            # (reaped: their CPU time counts)
        return n

    n, row = staged(decode_parallel)
    assert n == B * NVAL
    print(json.dumps(dict(head, figure="parent: CPU decode of every commitment, %d worker processes" % threads, **row)), flush=True)
    decoded = [np.stack(pts[k * NVAL:(k + 1) * NVAL]) for k in range(B)]
    del pts
    assert (decoded[1] == distinct[1 % DISTINCT][1]).all()

    def commit_affine(vs, k0):
        for i, v in enumerate(vs):
            v.commit(decoded[k0 + i])

    def commit_wire(vs, k0):
        e.verifier_commit_compressed_batch(vs, blobs[k0:k0 + len(vs)], defer=True)

    vs, _ = handles(commit_affine)
    verify(vs, "warm-up (affine commitments): templates, first-use allocations")
    walls = []
    for rep in range(2):
        vs, row = handles(commit_affine)
        if rep == 0:
            print(json.dumps(dict(head, figure="parent: bp_verifier_commit, %d verifiers" % (B - 1), **row)), flush=True)
        walls.append(verify(vs, "parent: bp_r1cs_batch_verify, affine commitments, run %d" % (rep + 1)))
    # ---- new path
    wwalls = []
    for rep in range(2):
        vs, row = handles(commit_wire)
        if rep == 0:
            print(json.dumps(dict(head, figure="new: bp_verifier_commit_compressed_batch(defer=1), %d verifiers" % (B - 1), **row)), flush=True)
        wwalls.append(verify(vs, "new: bp_r1cs_batch_verify, deferred wire commitments, run %d" % (rep + 1)))
    print(json.dumps(dict(head, figure="bp_r1cs_batch_verify: deferred against affine", affine_runs_s=walls, noise_s=round(abs(walls[0] - walls[1]), 4),
                          deferred_runs_s=wwalls, deferred_minus_affine_s=round(min(wwalls) - min(walls), 4))), flush=True)
    # ---- one more verifier with m = 1: bp_verifier_verify, the prologue route
    c0 = e.commit_wire_stats()
    v = E.VerifierCS(CV, E.HostTranscript(LABEL))
    var = v.commit_compressed(small[2], defer=True)
    record_range(v, words, var, NBITS)
    rc, row = staged(lambda: v.verify(e, small[0]))
    c1 = e.commit_wire_stats()
    assert rc == 0, rc
    print(json.dumps(dict(figure="new: bp_verifier_verify, one verifier with m = 1 (prologue)", wire_by_front_end=c1[0] - c0[0], wire_by_prologue_gpu=c1[1] - c0[1],
                          wire_on_host=c1[2] - c0[2], **row)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
