"""bp_r1cs_batch_verify_locate / bp_r1cs_batch_verify_locate_scenarios (include/arkbp.h "Batch verification that NAMES the failing
instances") on both curves: thirteen instances per batch (odd, so the halves differ), the smallest statements at which each route
of the batch verifier's core runs.  Expected statuses come from the CPU oracle, one instance at a time — never from the engine; the
number of passes and of instances in them from the planner's own simulation (bp_debug_locate_plan) of the same bad set."""
import hashlib
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import gadgets as GD

pytestmark = pytest.mark.gpu
OK, E_VERIFICATION, E_GENS_LENGTH, E_FORMAT = 0, -4, -5, -6
FROM_ORACLE = {0: OK, 1: E_VERIFICATION, 2: E_GENS_LENGTH, 4: E_FORMAT}   # protocol.hpp `enum Err` -> BP_E_*
SC_SHUFFLE, SC_RANGE, SC_MULTI_RANGE = 0, 1, 4
TUNE_VFY_DEVICE, TUNE_DIRECT_MAX, TUNE_VERIFY_LOCATE_LEAF = 11, 12, 22
GENS, COUNT = 128, 13
STATEMENTS = {"shuffle-2": (SC_SHUFFLE, [2]), "shuffle-4": (SC_SHUFFLE, [4]), "range-8": (SC_RANGE, [8, 201])}
T_X = 11 * 33                 # wire offset of t_x (11 points first; src/r1cs/proof.rs:74-81)
PTS_OFF = 11 * 33 + 96        # wire offset of L_vec's length
# the bad sets of the issue: none, first, last, middle, two adjacent, two in different halves (6 + 7), all
BAD_SETS = [(), (0,), (COUNT - 1,), (6,), (4, 5), (2, 10), tuple(range(COUNT))]


def wseed(*tag):
    return hashlib.sha256(repr(tag).encode()).digest()


def split_proof(proof):
    kl = int.from_bytes(proof[PTS_OFF:PTS_OFF + 8], "little")
    L0 = PTS_OFF + 8
    R0 = L0 + 33 * kl + 8
    kr = int.from_bytes(proof[R0 - 8:R0], "little")
    return proof[:PTS_OFF], [proof[L0 + 33 * i:L0 + 33 * (i + 1)] for i in range(kl)], [proof[R0 + 33 * i:R0 + 33 * (i + 1)] for i in range(kr)], proof[R0 + 33 * kr:]


def join_proof(head, L, R, tail):
    return head + len(L).to_bytes(8, "little") + b"".join(L) + len(R).to_bytes(8, "little") + b"".join(R) + tail


def through_the_check(proof, j):
    """a well-formed proof that fails only in the mega-check: a byte of t_x changed (even j), or L_0 replaced by another valid point,
    R_0 (odd j)"""
    if j % 2 == 0:
        b = bytearray(proof)
        b[T_X] ^= 1 << (j % 8)
        return bytes(b)
    head, L, R, tail = split_proof(proof)
    assert L and L[0] != R[0]
    return join_proof(head, [R[0]] + L[1:], R, tail)


def with_proof(inst, proof):
    return (inst[0], inst[1], proof, inst[3], inst[4])


class Env:
    def __init__(self, O, curve):
        import ark_bulletproofs_amd as A

        self.O, self.curve = O, curve
        self.eng = A.Engine(curve=curve)
        self.eng.gens_derive(GENS)
        self.F = GD.Field(O, curve)
        self._pools, self._expect, self._cs = {}, {}, {}

    def pool(self, name):
        if name not in self._pools:
            sc, prm = STATEMENTS[name]
            out = []
            for j in range(COUNT):
                pr = self.eng.prove_scenario(sc, prm, wseed("locate", self.curve, name, j))
                out.append((sc, prm, pr.proof, pr.commitments, pr.publics))
            self._pools[name] = out
        return self._pools[name]

    def expect(self, inst):
        """the oracle's single verification of a scenario instance, cached"""
        sc, prm, proof, cm, pb = inst
        key = (sc, tuple(prm), bytes(proof), np.asarray(cm, dtype=np.uint64).tobytes())
        if key not in self._expect:
            self._expect[key] = FROM_ORACLE[self.O.r1cs_verify(self.curve, sc, prm, GENS, proof, cm, pb)]
        return self._expect[key]

    def cs_pool(self, gadget):
        """(program, [(proof, V)]) of a recorded gadget, proved once"""
        from ark_bulletproofs_amd import engine as E

        if gadget not in self._cs:
            program, m = GADGETS[gadget]
            self._cs[gadget] = (program, [cs_prove(E, self.eng, self.F, program, j, m) for j in range(COUNT)])
        return self._cs[gadget]


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def env(request, oracle):
    e = Env(oracle, request.param)
    yield e
    e.eng.close()


def plan_for(expect):
    from ark_bulletproofs_amd import engine as E

    st, passes, inst = E.debug_locate_plan([s == E_VERIFICATION for s in expect], [s not in (OK, E_VERIFICATION) for s in expect])
    return len(passes), inst


def locate(eng, call):
    """one call; returns (rc, statuses, stats delta); the return value is the first non-zero status in instance order"""
    s0 = eng.verify_locate_stats()
    rc, st = call()
    s1 = eng.verify_locate_stats()
    assert rc == next((s for s in st if s), 0), "the call returns the first non-zero status in instance order"
    return rc, st, tuple(b - a for a, b in zip(s0, s1))


# ---- scenario statements: bad sets through the check ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STATEMENTS))
def test_bad_sets_scenarios(env, name):
    """shuffles (randomized constraints: the host replay) and the range statement (like-instances of one single-phase recording: the
    device front end), every bad set of the issue"""
    eng = env.eng
    valid = env.pool(name)
    for bad in BAD_SETS:
        batch = [with_proof(inst, through_the_check(inst[2], j)) if j in bad else inst for j, inst in enumerate(valid)]
        expect = [env.expect(inst) for inst in batch]
        assert expect == [E_VERIFICATION if j in bad else OK for j in range(COUNT)], "the oracle: these defects reach the check"
        d0 = eng.vfe_stats()
        rc, st, d = locate(eng, lambda: eng.batch_verify_locate(batch, wseed("alpha", name, bad)))
        assert st == expect, (name, bad, st)
        passes, inst = plan_for(expect)
        assert d[:3] == (1, passes, inst), (name, bad, d)
        assert d[3] == len(bad), "every bad proof ends as a subset of one"
        if name == "range-8":
            d1 = eng.vfe_stats()
            assert (d1[0] - d0[0], d1[1] - d0[1]) == (passes, 0), "every pass of like-instances completes on the device front end"


# ---- failures before the check, mixed with check failures ----------------------------------------------------------------------------
def oracle_status_fresh(curve, inst):
    """the oracle's status from a process of its own: the oracle keeps ONE generator table per curve that only grows, so a process
    that has used more than GENS generators never finds too few"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.NamedTemporaryFile(suffix=".pkl") as f:
        pickle.dump([inst[0], list(inst[1]), bytes(inst[2]), np.asarray(inst[3], dtype=np.uint64), np.asarray(inst[4], dtype=np.uint64)], f)
        f.flush()
        code = ("import sys, pickle; sys.path[:0] = [%r]; from oracle import pyoracle as O; sc, prm, proof, cm, pb = pickle.load(open(%r, 'rb')); "
                "print('status', O.r1cs_verify(%d, sc, prm, %d, proof, cm, pb))" % (os.path.dirname(here), f.name, curve, GENS))
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status" in r.stdout, (r.stdout + r.stderr)[-2000:]
    return FROM_ORACLE[int(r.stdout.split("status")[1].split()[0])]


def test_failures_before_the_check_keep_their_status_and_leave(env):
    eng, O, cv = env.eng, env.O, env.curve
    valid = env.pool("range-8")
    batch = list(valid)
    proof = valid[1][2]
    x = bytearray(proof)                                                         # an x that is on no point of the curve (A_O1)
    while O.point_deser_compressed(cv, bytes(x[33:66])) is not None:
        x[33] = (x[33] + 1) & 0xFF
    batch[1] = with_proof(valid[1], bytes(x))
    f = bytearray(valid[3][2]); f[32] |= 0x01                                    # an unknown flag bit
    batch[3] = with_proof(valid[3], bytes(f))
    a = bytearray(valid[4][2]); a[0:33] = bytes(32) + b"\x40"                    # A_I1 = the identity
    batch[4] = with_proof(valid[4], bytes(a))
    head, L, R, tail = split_proof(valid[8][2])
    batch[8] = with_proof(valid[8], join_proof(head, L[:-1], R, tail))           # L_vec one entry short
    big = O.r1cs_prove(cv, SC_MULTI_RANGE, [4, 64, 0], wseed("locate-big", cv), 256)   # claims 256 generators, 128 are installed
    assert big.rc == 0
    batch[11] = (SC_MULTI_RANGE, [4, 64, 0], big.proof, big.commitments, big.publics)
    for j in (6, 12):                                                            # ... and two that fail the check itself
        batch[j] = with_proof(valid[j], through_the_check(valid[j][2], j))
    expect = [oracle_status_fresh(cv, inst) if j == 11 else env.expect(inst) for j, inst in enumerate(batch)]
    assert expect[11] == E_GENS_LENGTH and expect[1] == expect[3] == E_FORMAT and expect[4] == E_VERIFICATION and expect[8] in (E_VERIFICATION, E_FORMAT), expect
    assert [expect[j] for j in (0, 2, 5, 6, 7, 9, 10, 12)] == [OK, OK, OK, E_VERIFICATION, OK, OK, OK, E_VERIFICATION]
    rc, st, d = locate(eng, lambda: eng.batch_verify_locate(batch, wseed("alpha", "before")))
    assert st == expect, st
    # the others are decided as if those five were absent: one pass more than the plan without them
    before = (1, 3, 4, 8, 11)
    rest = [expect[j] for j in range(COUNT) if j not in before]
    passes, inst = plan_for(rest)
    assert d[:3] == (1, passes + 1, inst + COUNT), d
    rc2, st2, d2 = locate(eng, lambda: eng.batch_verify_locate([batch[j] for j in range(COUNT) if j not in before], wseed("alpha", "before", 2)))
    assert st2 == rest and d2[:3] == (1, passes, inst)
    # only failures before the check: nothing is left to search
    only = [batch[j] if j in before else valid[j] for j in range(COUNT)]
    rc, st, d = locate(eng, lambda: eng.batch_verify_locate(only, wseed("alpha", "before", 3)))
    assert st == [expect[j] if j in before else OK for j in range(COUNT)] and d[:3] == (1, 2, COUNT + COUNT - len(before)), (st, d)


# ---- recorded handles -------------------------------------------------------------------------------------------------------------
CS_LABEL = b"verify locate"
GADGETS = {
    "one-phase": (lambda cs, F, wit, vars_: GD.random_program(cs, F, 91, wit, vars_, two_phase=False, n_mul=7, n_extra=0, n_alloc=1, n_mul2=3), 2),
    "two-phase": (lambda cs, F, wit, vars_: GD.random_program(cs, F, 91, wit, vars_, two_phase=True, n_mul=7, n_extra=0, n_alloc=1, n_mul2=3), 2),
    "other": (lambda cs, F, wit, vars_: GD.rare_shapes_program(cs, F, wit, vars_, two_phase=False), 3),
}


def cs_prove(E, eng, F, program, j, m):
    vals, blinds = GD.make_witness(F, 7000 + j, m)
    p = E.ProverCS(eng.curve, E.HostTranscript(CS_LABEL))
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    program(p, F, wit, vars_)
    return p.prove(eng, wseed("locate-cs", eng.curve, j)), V


def cs_verifier(E, curve, F, program, V, like=None):
    if like is not None:
        v = E.VerifierCS(curve, E.HostTranscript(CS_LABEL), like=like)
        v.commit(V)
        return v
    v = E.VerifierCS(curve, E.HostTranscript(CS_LABEL))
    program(v, F, None, v.commit(V))
    return v


def cs_expect(env, program, V, proof):
    v = env.O.VerifierCS(env.curve, CS_LABEL).start()
    program(v, env.F, None, v.commit(V))
    return FROM_ORACLE[v.verify(GENS, proof)]


def like_handles(E, env, program, items):
    v0 = cs_verifier(E, env.curve, env.F, program, items[0][1])
    return [v0] + [cs_verifier(E, env.curve, env.F, program, V, like=v0) for _, V in items[1:]]


def own_handles(E, env, program, items):
    return [cs_verifier(E, env.curve, env.F, program, V) for _, V in items]


def alphas(env, *tag):
    return env.O.fe_rand(env.O.fid(env.curve, True), wseed("alpha-cs", *tag), COUNT)


@pytest.mark.parametrize("gadget,device", [("one-phase", 1), ("two-phase", 2)])
def test_like_instances_on_the_device_front_end_and_on_the_host_replay(env, gadget, device):
    """like-instances of one recording: every pass completes on the device front end (two-phase statements with
    BP_TUNE_VFY_DEVICE = 2); the host replay (own recordings of every instance, BP_TUNE_VFY_DEVICE = 0) gives the same statuses"""
    from ark_bulletproofs_amd import engine as E

    eng = env.eng
    program, good = env.cs_pool(gadget)
    for bad in BAD_SETS:
        items = [(through_the_check(p, j), V) if j in bad else (p, V) for j, (p, V) in enumerate(good)]
        proofs = [p for p, _ in items]
        expect = [cs_expect(env, program, V, p) for p, V in items]
        assert expect == [E_VERIFICATION if j in bad else OK for j in range(COUNT)]
        passes, inst = plan_for(expect)
        eng.set_tuning(TUNE_VFY_DEVICE, device)
        try:
            d0 = eng.vfe_stats()
            rc, st, d = locate(eng, lambda: E.batch_verify_locate_cs(eng, like_handles(E, env, program, items), proofs, alphas(env, gadget, bad)))
            d1 = eng.vfe_stats()
            assert st == expect and d[:3] == (1, passes, inst), (gadget, bad, st, d)
            assert (d1[0] - d0[0], d1[1] - d0[1]) == (passes, 0), "passes that did not complete on the device front end"
            eng.set_tuning(TUNE_VFY_DEVICE, 0)
            rc_h, st_h, d_h = locate(eng, lambda: E.batch_verify_locate_cs(eng, own_handles(E, env, program, items), proofs, alphas(env, gadget, bad)))
            assert st_h == expect and rc_h == rc and d_h == d, (gadget, bad, st_h, d_h)
            assert eng.vfe_stats() == d1, "the host replay was asked for"
        finally:
            eng.set_tuning(TUNE_VFY_DEVICE, 1)


def test_two_gadgets_in_one_batch_and_a_callback_error(env):
    """a batch of two different gadgets takes the host replay; an instance whose randomized-phase callback returns 7 keeps that
    status and leaves, the others are decided as if it were absent"""
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    eng = env.eng
    prog_a, good_a = env.cs_pool("two-phase")
    prog_b, good_b = env.cs_pool("other")
    which = [prog_b if j % 3 == 1 else prog_a for j in range(COUNT)]
    good = [good_b[j] if j % 3 == 1 else good_a[j] for j in range(COUNT)]
    bad, cb_at = (1, 9), 5
    items = [(through_the_check(p, j), V) if j in bad else (p, V) for j, (p, V) in enumerate(good)]
    proofs = [p for p, _ in items]
    expect = [cs_expect(env, which[j], V, p) for j, (p, V) in enumerate(items)]
    assert expect == [E_VERIFICATION if j in bad else OK for j in range(COUNT)]
    d0 = eng.vfe_stats()
    vs = [cs_verifier(E, env.curve, env.F, which[j], V) for j, (_, V) in enumerate(items)]
    rc, st, d = locate(eng, lambda: E.batch_verify_locate_cs(eng, vs, proofs, alphas(env, "mixed")))
    passes, inst = plan_for(expect)
    assert st == expect and d[:3] == (1, passes, inst), (st, d)
    assert eng.vfe_stats() == d0, "two gadgets in one batch: no pass qualifies for the device front end"
    # the callback error: a second randomized-phase callback on instance cb_at that returns 7
    vs = [cs_verifier(E, env.curve, env.F, which[j], V) for j, (_, V) in enumerate(items)]
    cb = E._RANDOMIZE_CB(lambda _user, _handle: 7)
    assert lib().bp_cs_specify_randomized_constraints(vs[cb_at].h, cb, None) == OK
    rc, st, d = locate(eng, lambda: E.batch_verify_locate_cs(eng, vs, proofs, alphas(env, "mixed")))
    assert st == [7 if j == cb_at else expect[j] for j in range(COUNT)], st
    passes, inst = plan_for([expect[j] for j in range(COUNT) if j != cb_at])
    assert d[:3] == (1, passes + 1, inst + COUNT), d


def test_leaf_knob_and_direct_tables_do_not_change_the_statuses(env):
    """beyond the tables' reach (BP_TUNE_DIRECT_MAX = 0: the leaves take the single route), and the leaf knob at 4 with the tables on
    (the leaves take the grouped path of bp_verifier_verify_batch): the same statuses as pure bisection"""
    eng = env.eng
    valid = env.pool("shuffle-4")
    bad = (2, 3, 10)
    batch = [with_proof(inst, through_the_check(inst[2], j)) if j in bad else inst for j, inst in enumerate(valid)]
    expect = [env.expect(inst) for inst in batch]
    seed = wseed("alpha", "leaf")
    rc, st, d = locate(eng, lambda: eng.batch_verify_locate(batch, seed))
    passes, inst = plan_for(expect)
    assert st == expect and d == (1, passes, inst, len(bad)), (st, d)
    try:
        eng.set_tuning(TUNE_DIRECT_MAX, 0)
        rc, st, d0 = locate(eng, lambda: eng.batch_verify_locate(batch, seed))
        assert st == expect and d0 == d, (st, d0)
        eng.set_tuning(TUNE_VERIFY_LOCATE_LEAF, 4)
        e0 = eng.verify_each_stats()
        rc, st, d1 = locate(eng, lambda: eng.batch_verify_locate(batch, seed))
        e1 = eng.verify_each_stats()
        # 13 fails -> [0, 6) fails -> [0, 3) fails: a leaf; [3, 6) fails: a leaf; [6, 13) fails -> [6, 9) passes -> [9, 13): a leaf, untested
        assert st == expect and d1 == (1, 6, 13 + 6 + 3 + 3 + 7 + 3, 10), (st, d1)
        assert (e1[0] - e0[0], e1[1] - e0[1]) == (0, 10), "without the tables the leaves take the single route"
        eng.set_tuning(TUNE_DIRECT_MAX, 8192)
        rc, st, d2 = locate(eng, lambda: eng.batch_verify_locate(batch, seed))
        e2 = eng.verify_each_stats()
        assert st == expect and d2 == d1, (st, d2)
        assert (e2[0] - e1[0], e2[1] - e1[1]) == (10, 0), "with the tables the leaves are grouped"
    finally:
        eng.set_tuning(TUNE_DIRECT_MAX, 8192)
        eng.set_tuning(TUNE_VERIFY_LOCATE_LEAF, 0)


def test_rerunning_restores_every_member_and_weights_do_not_matter(env):
    """one bad proof on the host replay, which advances the transcripts and runs the randomized phase on the handles themselves: the
    first members go through three or four passes and are verified from their entry state each time; fresh handles and other weights
    give the same statuses"""
    from ark_bulletproofs_amd import engine as E

    eng = env.eng
    program, good = env.cs_pool("two-phase")
    items = [(through_the_check(p, 0), V) if j == 0 else (p, V) for j, (p, V) in enumerate(good)]
    proofs = [p for p, _ in items]
    expect = [cs_expect(env, program, V, p) for p, V in items]
    assert expect == [E_VERIFICATION] + [OK] * (COUNT - 1)
    eng.set_tuning(TUNE_VFY_DEVICE, 0)
    try:
        for tag, make in (("a", own_handles), ("b", own_handles), ("c", like_handles)):
            rc, st, d = locate(eng, lambda: E.batch_verify_locate_cs(eng, make(E, env, program, items), proofs, alphas(env, "rerun", tag)))
            assert st == expect and d == (1, 7, 13 + 6 + 3 + 1 + 2 + 3 + 7, 1), (tag, st, d)
    finally:
        eng.set_tuning(TUNE_VFY_DEVICE, 1)


def test_scenario_form_equals_recorded_handle_form(env):
    """the 8-bit range statement recorded through the handle API (host_proto.hpp range_gadget, constraint for constraint) against the
    scenario form on the same proofs and weights"""
    from ark_bulletproofs_amd import engine as E

    eng, F, O = env.eng, env.F, env.O
    valid = env.pool("range-8")
    bad = (0, 7, 8)
    batch = [with_proof(inst, through_the_check(inst[2], j)) if j in bad else inst for j, inst in enumerate(valid)]
    expect = [env.expect(inst) for inst in batch]
    seed = wseed("alpha", "forms")

    def range_verifier(V):
        v = E.VerifierCS(env.curve, E.HostTranscript(b"RangeProofTest"))
        (var,) = v.commit(np.asarray(V, dtype=np.uint64).reshape(1, 8))
        lc = [(var, F.w(1))]
        for i in range(8):
            a, b, o = v.allocate_multiplier(None)
            v.constrain([(o, F.w(1))])
            v.constrain([(a, F.w(1)), (b, F.w(1)), (GD.ONE, F.w(-1))])
            lc.append((b, F.w(-(1 << i))))
        v.constrain(lc)
        return v

    rc_s, st_s, d_s = locate(eng, lambda: eng.batch_verify_locate(batch, seed))
    al = O.fe_rand(O.fid(env.curve, True), seed, COUNT)                       # the weights the scenario form draws
    rc_r, st_r, d_r = locate(eng, lambda: E.batch_verify_locate_cs(eng, [range_verifier(i[3]) for i in batch], [i[2] for i in batch], al))
    assert st_s == expect and st_r == expect and rc_s == rc_r and d_s == d_r, (st_s, st_r, d_s, d_r)
