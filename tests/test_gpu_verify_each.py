"""bp_verifier_verify_batch / bp_r1cs_verify_each_scenarios (include/arkbp.h "Verification of many proofs with a verdict for EACH"):
many proofs per call, a status and a check point for each instance, on both curves.  Expected values come from the CPU oracle: its
own single verification for the statuses, the unit points of tests/batchref.py (an instance's mega-check with weight 1) for the
points — never from the code under test.  A valid instance gives the identity whatever the verifier does with it, so the
all-defective pools and the single defects at group boundaries are what see an instance that is dropped, repeated or swapped."""
import hashlib
import os
import pickle
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import batchref as BR
import gadgets as GD

pytestmark = pytest.mark.gpu
OK, E_VERIFICATION, E_GENS_LENGTH, E_FORMAT = 0, -4, -5, -6
FROM_ORACLE = {0: OK, 1: E_VERIFICATION, 2: E_GENS_LENGTH, 4: E_FORMAT}   # protocol.hpp `enum Err` -> BP_E_*
SC_SHUFFLE, SC_RANGE, SC_MULTI_RANGE = 0, 1, 4
TUNE_VFY_DEVICE, TUNE_DIRECT_MAX, TUNE_VERIFY_EACH = 11, 12, 15
WAITS = 1            # BP_VERIFY_EACH_WAITS_PER_GROUP
GENS = 512
# name -> (scenario, params, padded size N, instances in the pool)
STATEMENTS = {
    "shuffle-2": (SC_SHUFFLE, [2], 2, 257),           # two-phase, N = 2
    "shuffle-3": (SC_SHUFFLE, [3], 4, 9),
    "shuffle-16": (SC_SHUFFLE, [16], 32, 9),
    "range-16": (SC_RANGE, [16, 1234], 16, 9),
    "multi-range-2x8": (SC_MULTI_RANGE, [2, 8, 0], 16, 9),
    "multi-range-8x64": (SC_MULTI_RANGE, [8, 64, 0], 512, 3),   # two blocks of 256 per proof: the per-proof delta sum
}
PTS_OFF = 11 * 33 + 96        # wire offset of L_vec's length (11 points, t_x, t_x_blinding, e_blinding; src/r1cs/proof.rs:74-81)


def wseed(*tag):
    return hashlib.sha256(repr(tag).encode()).digest()


class Pool:
    def __init__(self, O, eng, R, name):
        sc, prm, self.N, count = STATEMENTS[name]
        self.name = name
        self.valid = []
        for j in range(count):
            pr = eng.prove_scenario(sc, prm, wseed("each", eng.curve, name, j))
            self.valid.append((sc, prm, pr.proof, pr.commitments, pr.publics))
        self.bad = [BR.defective(inst, j, O, eng.curve) for j, inst in enumerate(self.valid)]
        self.units = R.units(self.bad)
        assert self.units.any(axis=1).all()


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def env(request, oracle):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(GENS)
    R = BR.BatchRef(oracle, request.param, GENS)
    pools = {}

    def pool(name):
        if name not in pools:
            pools[name] = Pool(oracle, e, R, name)
        return pools[name]

    yield e, R, pool
    e.close()


def each(eng, instances):
    """one call; returns (rc, statuses, points, stats delta)"""
    s0 = eng.verify_each_stats()
    rc, st, pts = eng.verify_each_scenarios(instances, want_points=True)
    s1 = eng.verify_each_stats()
    assert rc == next((s for s in st if s), 0), "the call returns the first non-zero status in instance order"
    return rc, st, pts, tuple(b - a for a, b in zip(s0, s1))


def oracle_status(O, curve, inst):
    sc, prm, proof, cm, pb = inst
    return FROM_ORACLE[O.r1cs_verify(curve, sc, prm, GENS, proof, cm, pb)]


def oracle_status_fresh(curve, inst):
    """the oracle's status from a process of its own.  The oracle keeps ONE generator table per curve that only grows: in a process
    that has used more than GENS generators (this one proves the large statement with 1024; other tests of the suite use more) it
    never finds too few.  A fresh process holds exactly the GENS it is asked for, like the engine under test."""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.NamedTemporaryFile(suffix=".pkl") as f:
        pickle.dump([inst[0], list(inst[1]), bytes(inst[2]), np.asarray(inst[3], dtype=np.uint64), np.asarray(inst[4], dtype=np.uint64)], f)
        f.flush()
        code = ("import sys, pickle; sys.path[:0] = [%r]; from oracle import pyoracle as O; sc, prm, proof, cm, pb = pickle.load(open(%r, 'rb')); "
                "print('status', O.r1cs_verify(%d, sc, prm, %d, proof, cm, pb))" % (os.path.dirname(here), f.name, curve, GENS))
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status" in r.stdout, (r.stdout + r.stderr)[-2000:]
    return FROM_ORACLE[int(r.stdout.split("status")[1].split()[0])]


# ---- valid and all-defective pools --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 257])
def test_valid_distinct_instances(env, count):
    eng, R, pool = env
    P = pool("shuffle-2")
    rc, st, pts, d = each(eng, P.valid[:count])
    assert rc == OK and st == [OK] * count and not pts.any()
    assert d[0] == count and d[1] == 0 and d[2] == 1 and d[3] == WAITS, d
    # without the points the verdicts are the same
    assert eng.verify_each_scenarios(P.valid[:count]) == (OK, [OK] * count)


@pytest.mark.parametrize("name", list(STATEMENTS))
def test_statement_valid_and_all_defective(env, name):
    eng, R, pool = env
    P = pool(name)
    n = min(len(P.valid), 9)
    rc, st, pts, d = each(eng, P.valid[:n])
    assert rc == OK and st == [OK] * n and not pts.any(), (name, st)
    assert d[:3] == (n, 0, 1), d
    rc, st, pts, d = each(eng, P.bad[:n])
    assert st == [E_VERIFICATION] * n and rc == E_VERIFICATION
    for j in range(n):
        assert (pts[j] == P.units[j]).all(), "%s: check point of instance %d is not its unit point" % (name, j)


@pytest.mark.parametrize("count", [1, 2, 64, 65, 257])
def test_all_defective_pool_prefixes(env, count):
    """every instance's point is ITS unit point: a dropped, repeated or swapped instance shows"""
    eng, R, pool = env
    P = pool("shuffle-2")
    rc, st, pts, d = each(eng, P.bad[:count])
    assert st == [E_VERIFICATION] * count
    assert (pts == P.units[:count]).all(), "instances %r carry another instance's point" % np.nonzero((pts != P.units[:count]).any(axis=1))[0].tolist()


# ---- recorded handles (bp_verifier_verify_batch) ---------------------------------------------------------------------------------
CS_LABEL = b"verify each"


def cs_prove(E, eng, F, program, j, m):
    vals, blinds = GD.make_witness(F, 9000 + j, m)
    p = E.ProverCS(eng.curve, E.HostTranscript(CS_LABEL))
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    program(p, F, wit, vars_)
    return p.prove(eng, wseed("each-cs", eng.curve, j)), V


def cs_verifier(E, curve, F, program, V, like=None):
    if like is not None:
        v = E.VerifierCS(curve, E.HostTranscript(CS_LABEL), like=like)
        v.commit(V)
        return v
    v = E.VerifierCS(curve, E.HostTranscript(CS_LABEL))
    program(v, F, None, v.commit(V))
    return v


def cs_oracle_verifier(O, curve, F, program, V):
    v = O.VerifierCS(curve, CS_LABEL).start()
    program(v, F, None, v.commit(V))
    return v


GADGETS = {
    "random one-phase": (lambda cs, F, wit, vars_: GD.random_program(cs, F, 91, wit, vars_, two_phase=False, n_mul=7, n_extra=0, n_alloc=1, n_mul2=3), 2),
    "random two-phase": (lambda cs, F, wit, vars_: GD.random_program(cs, F, 91, wit, vars_, two_phase=True, n_mul=7, n_extra=0, n_alloc=1, n_mul2=3), 2),
    "rare shapes one-phase": (lambda cs, F, wit, vars_: GD.rare_shapes_program(cs, F, wit, vars_, two_phase=False), 3),
    "rare shapes two-phase": (lambda cs, F, wit, vars_: GD.rare_shapes_program(cs, F, wit, vars_, two_phase=True), 3),
}


@pytest.mark.parametrize("gadget", list(GADGETS))
def test_recorded_handles(env, oracle, gadget):
    """own recordings and like-instances in one call: verdicts and points per instance, the transcripts of accepted instances where
    bp_verifier_verify leaves them"""
    from ark_bulletproofs_amd import engine as E

    eng, R, _ = env
    O, cv = oracle, eng.curve
    program, m = GADGETS[gadget]
    F = GD.Field(O, cv)
    count = 7
    good = [cs_prove(E, eng, F, program, j, m) for j in range(count)]
    proofs, Vs = [g[0] for g in good], [g[1] for g in good]
    bproofs = [BR.defect_proof(p, j) for j, p in enumerate(proofs)]
    bVs = [BR.defect_commitments(V, j, O, cv) for j, V in enumerate(Vs)]
    units = R.units_cs([("each", gadget, j) for j in range(count)], lambda j: (cs_oracle_verifier(O, cv, F, program, bVs[j]), bproofs[j]))
    assert units.any(axis=1).all()

    def verifiers(Vlist):   # instances 0 and 3 record the gadget themselves, the others are like-instances of instance 0
        v0 = cs_verifier(E, cv, F, program, Vlist[0])
        return [v0] + [cs_verifier(E, cv, F, program, V, like=None if j == 3 else v0) for j, V in enumerate(Vlist[1:], 1)]

    s0 = eng.verify_each_stats()
    vs = verifiers(Vs)
    rc, st, pts = eng.verify_each(vs, proofs, want_points=True)
    assert rc == OK and st == [OK] * count and not pts.any(), st
    assert eng.verify_each_stats()[0] - s0[0] == count, "the instances took the single route"
    # the twins go through bp_verifier_verify's host replay, which leaves the handle's transcript where the reference's
    # verify_and_return_transcript does (the device front end of like-instances works on a copy of the state)
    twins = verifiers(Vs)
    eng.set_tuning(TUNE_VFY_DEVICE, 0)
    try:
        for j, t in enumerate(twins):
            assert t.verify(eng, proofs[j]) == OK
            assert E.transcript_state(vs[j].transcript_obj) == E.transcript_state(t.transcript_obj), "transcript of instance %d differs from bp_verifier_verify's" % j
    finally:
        eng.set_tuning(TUNE_VFY_DEVICE, 1)
    # consumed: a second call refuses the batch as a whole
    with pytest.raises(Exception):
        eng.verify_each(vs, proofs)
    # mixed valid / defective, every position with its own verdict and point
    mixV = [bVs[j] if j % 2 else Vs[j] for j in range(count)]
    mixP = [bproofs[j] if j % 2 else proofs[j] for j in range(count)]
    rc, st, pts = eng.verify_each(verifiers(mixV), mixP, want_points=True)
    assert rc == E_VERIFICATION and st == [E_VERIFICATION if j % 2 else OK for j in range(count)]
    for j in range(count):
        assert (pts[j] == (units[j] if j % 2 else 0)).all(), "instance %d" % j
    for j, t in enumerate(verifiers(mixV)):
        assert t.verify(eng, mixP[j]) == st[j], "twin handle of instance %d" % j
        assert FROM_ORACLE[cs_oracle_verifier(O, cv, F, program, mixV[j]).verify(GENS, mixP[j])] == st[j]


# ---- mixed batches -----------------------------------------------------------------------------------------------------------------
def split_proof(proof):
    kl = int.from_bytes(proof[PTS_OFF:PTS_OFF + 8], "little")
    L0 = PTS_OFF + 8
    R0 = L0 + 33 * kl + 8
    kr = int.from_bytes(proof[R0 - 8:R0], "little")
    return proof[:PTS_OFF], [proof[L0 + 33 * i:L0 + 33 * (i + 1)] for i in range(kl)], [proof[R0 + 33 * i:R0 + 33 * (i + 1)] for i in range(kr)], proof[R0 + 33 * kr:]


def join_proof(head, L, R, tail):
    return head + len(L).to_bytes(8, "little") + b"".join(L) + len(R).to_bytes(8, "little") + b"".join(R) + tail


def mixed_batch(O, eng, pool):
    cv = eng.curve
    s2, s3, s16, rg, mr = (pool(n) for n in ("shuffle-2", "shuffle-3", "shuffle-16", "range-16", "multi-range-2x8"))
    out = []
    out += [s2.valid[0], rg.valid[0], s2.bad[1], mr.bad[2], s3.valid[1], s16.bad[3], s16.valid[4], rg.bad[5], s2.valid[2]]

    def with_proof(inst, proof):
        return (inst[0], inst[1], proof, inst[3], inst[4])

    pr = rg.valid[1][2]
    out.append(with_proof(rg.valid[1], pr[:-5]))                                   # truncated
    x = bytearray(s2.valid[3][2])                                                  # an x that is on no point of the curve (A_O1)
    while O.point_deser_compressed(cv, bytes(x[33:66])) is not None:
        x[33] = (x[33] + 1) & 0xFF
    out.append(with_proof(s2.valid[3], bytes(x)))
    t1 = bytearray(mr.valid[3][2])                                                 # T_1 = the identity (ark-serialize: x = 0, infinity flag)
    t1[6 * 33:7 * 33] = b"\0" * 32 + b"\x40"
    out.append(with_proof(mr.valid[3], bytes(t1)))
    head, L, R, tail = split_proof(rg.valid[2][2])
    out.append(with_proof(rg.valid[2], join_proof(head, L[:-1], R[:-1], tail)))     # L_vec, R_vec one round short (claims N = 8)
    out.append(with_proof(rg.valid[3], join_proof(head, L[:-1], R, tail)))          # L_vec and R_vec of different lengths
    head, L, R, tail = split_proof(s3.valid[2][2])
    out.append(with_proof(s3.valid[2], join_proof(head, L + L[:1], R + R[:1], tail)))   # one round too many (claims N = 8)
    big = O.r1cs_prove(cv, SC_MULTI_RANGE, [16, 64, 0], wseed("each-big", cv), 1024)    # a statement larger than the generators
    assert big.rc == 0
    out.append((SC_MULTI_RANGE, [16, 64, 0], big.proof, big.commitments, big.publics))
    out += [s3.bad[4], mr.valid[5]]
    return out


def test_mixed_batch_matches_the_oracle_and_the_single_verifier_at_every_position(env, oracle):
    eng, R, pool = env
    O, cv = oracle, eng.curve
    batch = mixed_batch(O, eng, pool)
    BIG = len(batch) - 3                                   # the statement larger than the generators
    expect = [oracle_status_fresh(cv, inst) if i == BIG else oracle_status(O, cv, inst) for i, inst in enumerate(batch)]
    assert expect[BIG] == E_GENS_LENGTH
    assert {OK, E_VERIFICATION, E_FORMAT, E_GENS_LENGTH} <= set(expect), expect
    twin = [eng.verify_scenario(*inst) for inst in batch]
    assert twin == expect, "bp_r1cs_verify_scenario differs from the oracle"
    # the unit point of every instance whose verdict comes from the mega-check itself (the others failed before it, or are valid)
    got_units = {i: R.units([batch[i]])[0] for i in range(len(batch)) if expect[i] == E_VERIFICATION and oracle_reaches_check(O, cv, batch[i])}
    assert len(got_units) >= 5
    for move in (None, "first", "last"):
        order = list(range(len(batch)))
        if move == "first":
            order = [10] + order[:10] + order[11:]          # the off-curve instance leads
        elif move == "last":
            order = order[:2] + order[3:] + [2]             # a defective instance closes
        rc, st, pts, d = each(eng, [batch[i] for i in order])
        assert st == [expect[i] for i in order], (move, st)
        assert d[0] + d[1] == len(batch) and d[1] >= 3, d       # (truncated, unequal lengths, beyond the generators: the single route)
        for pos, i in enumerate(order):
            if i in got_units:
                assert (pts[pos] == got_units[i]).all(), "instance %d (position %d, %s)" % (i, pos, move)
            else:
                assert not pts[pos].any(), "instance %d failed before its check or is valid: all-zero point" % i


def oracle_reaches_check(O, cv, inst):
    """True when the oracle's verdict on inst comes from the mega-check itself (a non-identity point), not from an earlier return"""
    rc, pt = O.batch_verify_point(cv, [inst], GENS, BR.UNIT_SEED)
    return rc == O.E_VERIFICATION and np.asarray(pt).any()


# ---- group boundaries ------------------------------------------------------------------------------------------------------------
def test_groups_of_three(env):
    eng, R, pool = env
    P = pool("shuffle-2")
    eng.set_tuning(TUNE_VERIFY_EACH, 3)
    try:
        rc, st, pts, d = each(eng, P.valid[:8])
        assert st == [OK] * 8 and d == (8, 0, 3, 3 * WAITS), d          # 3 + 3 + 2
        for j in (0, 2, 3, 5, 6, 7):                                    # first and last index of every group
            inst = list(P.valid[:8])
            inst[j] = P.bad[j]
            rc, st, pts, d = each(eng, inst)
            assert st == [E_VERIFICATION if i == j else OK for i in range(8)] and rc == E_VERIFICATION
            assert (pts[j] == P.units[j]).all() and not np.delete(pts, j, axis=0).any()
            assert d[2] == 3
        rc, st, pts, d = each(eng, P.bad[:8])
        assert (pts == P.units[:8]).all() and d[2] == 3
    finally:
        eng.set_tuning(TUNE_VERIFY_EACH, 0)


@pytest.mark.parametrize("count", [1, 2, 64, 65])
def test_single_defect_at_the_ends(env, count):
    eng, R, pool = env
    P = pool("shuffle-2")
    for j in sorted({0, count - 1}):
        inst = list(P.valid[:count])
        inst[j] = P.bad[j]
        rc, st, pts, d = each(eng, inst)
        assert st == [E_VERIFICATION if i == j else OK for i in range(count)]
        assert (pts[j] == P.units[j]).all() and not np.delete(pts, j, axis=0).any()
        assert d == (count, 0, 1, WAITS), d


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def test_routing_from_the_stats(env, oracle):
    eng, R, pool = env
    s2, s3, rg = pool("shuffle-2"), pool("shuffle-3"), pool("range-16")
    batch = [s2.valid[0], rg.valid[0], s3.bad[1], rg.bad[2], s2.valid[1]]
    expect = [OK, OK, E_VERIFICATION, E_VERIFICATION, OK]
    rc, st, pts, d = each(eng, batch)
    assert st == expect and d[:3] == (5, 0, 3), d                          # three templates, three groups
    assert d[3] == WAITS * d[2]
    eng.set_tuning(TUNE_DIRECT_MAX, 8)
    try:
        rc, st, pts2, d = each(eng, batch)
        assert st == expect and d[:3] == (3, 2, 2), d                      # N = 16 goes to the single route in the same call
        assert (pts2 == pts).all() and (pts[2] == s3.units[1]).all() and (pts[3] == rg.units[2]).all()
    finally:
        eng.set_tuning(TUNE_DIRECT_MAX, 8192)
    # N = 1: a shuffle of one value has no multipliers to pad
    pr = eng.prove_scenario(SC_SHUFFLE, [1], wseed("each-k1", eng.curve))
    one = (SC_SHUFFLE, [1], pr.proof, pr.commitments, pr.publics)
    assert oracle_status(oracle, eng.curve, one) == OK
    rc, st, pts, d = each(eng, [one, s2.valid[2], BR.defective(one, 1, oracle, eng.curve)])
    assert st == [OK, OK, E_VERIFICATION] and d[:3] == (1, 2, 1), d
    assert (pts[2] == R.units([BR.defective(one, 1, oracle, eng.curve)])[0]).all()
    # the waits of a group do not depend on the number of instances
    for B in (2, 65):
        rc, st, pts, d = each(eng, s2.valid[:B])
        assert d == (B, 0, 1, WAITS), d


# ---- the rest of the ctx is left as it was ----------------------------------------------------------------------------------------
def test_single_and_batch_verification_afterwards_as_on_a_fresh_ctx(env):
    import ark_bulletproofs_amd as A

    eng, R, pool = env
    s2, rg = pool("shuffle-2"), pool("range-16")
    each(eng, s2.bad[:5] + rg.valid[:3])
    fresh = A.Engine(curve=eng.curve)
    try:
        fresh.gens_derive(GENS)
        seed = bytes([0x21]) * 32
        for e in (eng, fresh):
            assert e.verify_scenario(*rg.valid[0]) == OK and e.verify_scenario(*rg.bad[1]) == E_VERIFICATION
        a = eng.batch_verify(rg.bad[:4] + s2.valid[:3], seed, want_point=True)
        b = fresh.batch_verify(rg.bad[:4] + s2.valid[:3], seed, want_point=True)
        assert a[0] == b[0] == E_VERIFICATION and (a[2] == b[2]).all()
        assert (a[2] == R.point(rg.units[:4], R.alphas(seed, 4))).all()
        assert eng.batch_verify(s2.valid[:6], seed)[0] == fresh.batch_verify(s2.valid[:6], seed)[0] == OK
    finally:
        fresh.close()


def test_three_ctxs_share_one_table_set_from_three_threads(env):
    import ark_bulletproofs_amd as A

    eng, R, pool = env
    s2, mr = pool("shuffle-2"), pool("multi-range-2x8")
    eng.gens_direct_tables(GENS)
    others = [A.Engine(curve=eng.curve) for _ in range(2)]
    res, errs = {}, []
    try:
        for o in others:
            o.share_gens_from(eng)
        batches = [s2.bad[t:t + 20] + mr.valid[:4] + mr.bad[4:8] + s2.valid[40 + t:50 + t] for t in range(3)]

        def work(t, e):
            try:
                res[t] = e.verify_each_scenarios(batches[t], want_points=True)
            except Exception as ex:   # noqa: BLE001
                errs.append(ex)

        ths = [threading.Thread(target=work, args=(t, e)) for t, e in enumerate([eng] + others)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for t in range(3):
            rc, st, pts = res[t]
            assert st == [E_VERIFICATION] * 20 + [OK] * 4 + [E_VERIFICATION] * 4 + [OK] * 10
            assert (pts[:20] == s2.units[t:t + 20]).all() and (pts[24:28] == mr.units[4:8]).all() and not pts[20:24].any() and not pts[28:].any()
        for o in others:
            assert o.direct_stats()[1] == GENS and o.verify_each_stats()[0] == 38
    finally:
        for o in others:
            o.close()


def test_template_cache_eviction_under_verify_each(oracle):
    """the verify_each counterpart of test_gpu_verify.py::test_template_cache_eviction_keeps_what_the_block_uses: a ctx whose template
    cache is past its bound, then ONE call that mixes new shapes (first) with shapes cached before.  The eviction of that call must
    keep every template an instance of the call resolves to, and every instance still gets the oracle's verdict."""
    import ark_bulletproofs_amd as A

    O, cv, gens = oracle, 0, 128
    e = A.Engine(curve=cv)
    e.gens_derive(gens)
    try:
        def stmt(n):
            pr = e.prove_scenario(3, [n, 0], bytes([n & 255]) * 32, m_cap=8)   # square chain with n multipliers: one shape per n
            return (3, [n, 0], pr.proof, pr.commitments, pr.publics)

        shapes = {n: stmt(n) for n in range(2, 76)}
        # 70 shapes, each twice (a shape used once is recorded inside its own replay): more than the cache holds
        rc, _, pt = e.batch_verify([shapes[n] for n in range(2, 72)] * 2, bytes([11]) * 32, want_point=True)
        assert rc == OK and not pt.any()
        mixed = [shapes[n] for n in (72, 73, 74, 75)] + [shapes[n] for n in range(40, 72)]
        sc, prm, proof, cm, pb = mixed[20]
        bad = bytearray(proof)
        bad[11 * 33 + 40] ^= 2                                                  # a low byte of t_x_blinding: still a canonical scalar
        mixed[20] = (sc, prm, bytes(bad), cm, pb)
        want = [FROM_ORACLE[O.r1cs_verify(cv, i[0], i[1], gens, i[2], i[3], i[4])] for i in mixed]
        assert want[20] == E_VERIFICATION and want.count(OK) == len(mixed) - 1
        rc, st, _, d = each(e, mixed)
        assert st == want
        assert d[0] == len(mixed) and d[1] == 0 and d[2] >= 1, d               # every instance took the grouped path
    finally:
        e.close()
