#!/usr/bin/env python3
"""The batches that pin the host side of batch verification (tests/test_vfy_host_steps_cpu.py, tests/golden/make_vfy_host_staging.py).

Every batch runs as a dry run on a host-only ctx: framing, square roots on the pool, the transcript replays and the staging of each
block happen as on a device, and the call returns (rc, checksum of every staged byte, instance count, launch slots) in place of a
mega-check.  The proofs come from the CPU oracle with fixed seeds, generators 256.

Run as a program it prints the results of both curves as one JSON line (the test starts it as a fresh child process with
ARKBP_VFY_NOX8=1: the library reads that switch once)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GENS = 256
SEED = bytes([5]) * 32
TUNE_HOST_THREADS = 6
BLOCK = 512   # VFY_BLOCK (csrc/r1cs_host.inc)


def proofs_for(O, cv, sc, prm, count, distinct, gens=GENS):
    base = []
    for i in range(distinct):
        pr = O.r1cs_prove(cv, sc, prm, bytes([40 + i]) * 32, gens, m_cap=64)
        assert pr.rc == 0
        base.append((sc, prm, pr.proof, pr.commitments, pr.publics))
    return [base[i % distinct] for i in range(count)]


def _with_proof(inst, k, proof):
    s, p, _, cm, pb = inst[k]
    out = list(inst)
    out[k] = (s, p, bytes(proof), cm, pb)
    return out


def _off_curve(O, cv, proof, point=2):
    """the proof with the x of one compressed point moved to the next value that is no x of a curve point (flags untouched)"""
    bad = bytearray(proof)
    at = point * 33
    for _ in range(255):
        bad[at] = (bad[at] + 1) & 0xFF
        if O.point_deser_compressed(cv, bytes(bad[at: at + 33])) is None:
            return bytes(bad)
    raise AssertionError("no x off the curve found")


def _identity(proof, point=6):
    bad = bytearray(proof)
    bad[point * 33: (point + 1) * 33] = b"\x00" * 32 + b"\x40"
    return bytes(bad)


def batches(O, cv):
    """(ok rows, error rows): name -> instances"""
    like = proofs_for(O, cv, O.SC_MULTI_RANGE, [3, 8, 0], 9, 3)                       # one lockstep group of 8 + one live replay
    small = proofs_for(O, cv, O.SC_MULTI_RANGE, [2, 4, 0], BLOCK + 8, 4)              # crosses one block boundary
    mixed = (like + proofs_for(O, cv, O.SC_RANGE, [16, 77], 5, 2) + proofs_for(O, cv, O.SC_SHUFFLE, [4], 6, 2)   # (two-phase)
             + proofs_for(O, cv, O.SC_SQUARE_CHAIN, [20, 0], 4, 1) + like[:4])
    widths = []                                                                       # 66 structures: the template cache (64) evicts
    for nbits in range(1, 65):
        widths += proofs_for(O, cv, O.SC_RANGE, [nbits, 1], 1, 1)
    widths += proofs_for(O, cv, O.SC_MULTI_RANGE, [2, 7, 0], 1, 1) + proofs_for(O, cv, O.SC_MULTI_RANGE, [3, 5, 0], 1, 1)
    ok = {"like9": like, "like520": small, "mixed4": mixed, "widths66": widths, "widths66_again": widths[::-1][:40] + widths[:40]}
    proof = small[7][2]
    err = {
        "truncated": _with_proof(small[:30], 5, proof[:-1]),
        "off_curve_block0": _with_proof(small, 12, _off_curve(O, cv, small[12][2])),
        "off_curve_block1": _with_proof(small, BLOCK + 3, _off_curve(O, cv, small[BLOCK + 3][2])),
        "identity_point": _with_proof(small[:30], 3, _identity(small[3][2])),
        "gens_length": small[:20] + proofs_for(O, cv, O.SC_MULTI_RANGE, [40, 8, 0], 1, 1, gens=512),
        "bad_then_truncated": _with_proof(_with_proof(small[:30], 3, _identity(small[3][2])), 10, small[10][2][:-1]),
        "bad_then_off_curve_block1": _with_proof(_with_proof(small, 3, _identity(small[3][2])), BLOCK + 3, _off_curve(O, cv, small[BLOCK + 3][2])),
    }
    return ok, err


def dry(eng, inst):
    rc, _, pt = eng.batch_verify(inst, SEED, want_point=True)
    return [int(rc), "%016x" % int(pt[0]), int(pt[1]), int(pt[2])]


def locate(E, eng, inst):
    """bp_r1cs_batch_verify_locate_scenarios, raw: (rc, statuses); the statuses start at 1, a value the library never writes"""
    from ark_bulletproofs_amd._lib import lib, ptr

    pk = E.PackedInstances(inst)
    st = (C.c_int * pk.n)(*([1] * pk.n))
    rc = lib().bp_r1cs_batch_verify_locate_scenarios(eng.ctx, C.c_size_t(pk.n), pk.scen, ptr(pk.prm), pk.proofs, pk.plens, ptr(pk.cms), pk.ms, ptr(pk.pubs), pk.npubs,
                                                     SEED, st, None)
    return [int(rc), [int(s) for s in st]]


def run_curve(E, O, cv, threads, with_locate=False):
    ok, err = batches(O, cv)
    eng = E.Engine.host_only(cv, GENS)
    try:
        eng.set_tuning(TUNE_HOST_THREADS, threads)
        out = {"ok": {name: dry(eng, inst) for name, inst in ok.items()}, "err": {name: dry(eng, inst)[0] for name, inst in err.items()}}
        if with_locate:
            out["locate"] = {name: locate(E, eng, inst) for name, inst in err.items()}
        return out
    finally:
        eng.close()


def run_all(threads, with_locate=False):
    from ark_bulletproofs_amd import engine as E
    from oracle import pyoracle as O

    return {str(cv): run_curve(E, O, cv, threads, with_locate) for cv in (0, 1)}


if __name__ == "__main__":
    print(json.dumps(run_all(int(sys.argv[1]) if len(sys.argv) > 1 else 8)))
