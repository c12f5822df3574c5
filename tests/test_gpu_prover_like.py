"""Like-provers on the GPU (include/arkbp.h bp_prover_new_like, bp_prover_assign_multipliers, bp_ctx_prover_like_stats;
csrc/r1cs.cuh k_r1cs_gate_out; csrc/r1cs_host.inc pl_*): a like-prover proves to the bytes of a prover that recorded the gadget
itself with the same witness, commitments, transcript state, rng bytes and blinding mode, on every route, and leaves its transcript
in the same state; the recording's constraint index is uploaded once per ctx; the gate outputs come from the kernel.  Gadgets:
tests/likecommon.py (tests/gadgets.py programs and the reference's k-shuffle)."""
import ctypes as C

import pytest

import gadgets as GD
import likecommon as LC
import wcheck as W

pytestmark = pytest.mark.gpu
GENS = 512
TUNE_DIRECT_MAX, TUNE_PROVE_BATCH_FRONT = 12, 14   # include/arkbp.h BP_TUNE_DIRECT_MAX, BP_TUNE_PROVE_BATCH_FRONT
E_ARG, E_UNSATISFIED = -1, -8


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def engines(E):
    """per curve: the default engine, and one that proves nothing over the direct tables (BP_TUNE_DIRECT_MAX = 0: folding, and with
    it the non-fused upload path at padded size 64)"""
    out = {}
    for cv in (0, 1):
        for dm in (None, 0):
            e = E.Engine(curve=cv, device=0)
            e.gens_derive(GENS)
            if dm is not None:
                e.set_tuning(TUNE_DIRECT_MAX, dm)
            out[(cv, dm)] = e
    yield out
    for e in out.values():
        e.close()


def prove(E, eng, r, tag, variant="plain"):
    """(proof, transcript state afterwards) of a Rec through bp_prover_prove"""
    if variant == "expanded":
        r.p.set_blinding(E.BLINDING_EXPANDED)
    if variant == "precompute":
        r.p.precompute(LC.rng(tag))
    proof = r.p.prove(eng, LC.rng(tag))
    return proof, E.transcript_state(r.t)


def precompute8(L, recs, tag):
    """bp_prover_precompute_batch over 8 provers with their rng bytes set"""
    for j, r in enumerate(recs):
        assert L.lib().bp_prover_set_rng(r.p.h, LC.rng(tag + j)) == 0
    hs = (C.c_void_p * len(recs))(*[r.p.h for r in recs])
    assert L.lib().bp_prover_precompute_batch(hs, C.c_size_t(len(recs))) == 0


SIZES = [(("single", 1, 41), None), (("single", 3, 42), None), (("single", 5, 43), None), (("single", 33, 44), 0), (("shuffle", 2), None), (("shuffle", 5), None)]


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("variant", ["plain", "precompute", "precompute8", "expanded"])
@pytest.mark.parametrize("spec,dm", SIZES, ids=lambda x: "%s%d" % (x[0], x[1]) if isinstance(x, tuple) else "dm%s" % x)
def test_single_route_byte_identity(E, engines, oracle, curve, variant, spec, dm):
    from ark_bulletproofs_amd import _lib as L

    F, eng = GD.Field(oracle, curve), engines[(curve, dm)]
    src = LC.record(E, curve, F, spec, 11)
    count = 8 if variant == "precompute8" else 1
    twins = [LC.record(E, curve, F, spec, 20 + j) for j in range(count)]
    likes = [LC.like(E, src, tw) for tw in twins]
    for lk, tw in zip(likes, twins):
        assert lk.p.metrics() == tw.p.metrics() and (lk.V == tw.V).all()
        assert E.transcript_state(lk.t) == E.transcript_state(tw.t)
    if variant == "precompute8":
        precompute8(L, twins, 300)
        precompute8(L, likes, 300)
    for j, (lk, tw) in enumerate(zip(likes, twins)):
        want, want_state = prove(E, eng, tw, 300 + j, variant)
        got, got_state = prove(E, eng, lk, 300 + j, variant)
        assert got == want, "the like-prover's proof differs from the self-recorded prover's"
        assert got_state == want_state, "the transcripts end in different states"
        if j == 0:
            assert LC.verifier(E, curve, F, spec, tw.V).verify(eng, got) == 0
            if variant == "plain":
                assert got == LC.oracle_proof(oracle, curve, F, spec, 20, GENS, LC.rng(300))


@pytest.mark.parametrize("curve", [0, 1])
def test_frozen_source_proves_to_its_own_bytes(E, engines, oracle, curve):
    F, eng = GD.Field(oracle, curve), engines[(curve, None)]
    for spec in (("single", 5, 45), ("program2", 4, 46), ("shuffle", 3)):
        untouched = LC.record(E, curve, F, spec, 12)
        src = LC.record(E, curve, F, spec, 12)
        lk = LC.like(E, src, untouched)                    # freezes src
        want, want_state = prove(E, eng, untouched, 310)
        got, got_state = prove(E, eng, src, 310)
        assert got == want and got_state == want_state
        assert prove(E, eng, lk, 310) == (want, want_state)


@pytest.mark.parametrize("curve", [0, 1])
def test_index_is_uploaded_once_per_recording_and_ctx(E, engines, oracle, curve):
    F = GD.Field(oracle, curve)
    eng = E.Engine(curve=curve, device=0)
    eng2 = E.Engine(curve=curve, device=0)
    try:
        eng.gens_derive(GENS)
        eng2.share_gens_from(eng)
        spec = ("single", 5, 47)
        src = LC.record(E, curve, F, spec, 13)
        assert eng.prover_like_stats() == (0, 0, 0, 0, 0)
        twins = [LC.record(E, curve, F, spec, 30 + j) for j in range(5)]
        likes = [LC.like(E, src, tw) for tw in twins]
        for j in range(5):
            assert prove(E, eng, likes[j], 320 + j) == prove(E, eng, twins[j], 320 + j)
        up, hits, resident, gdev, ghost = eng.prover_like_stats()
        assert (up, hits, gdev, ghost) == (1, 4, 25, 0) and resident > 0
        # a second ctx sharing the generators: its own copy
        tw = LC.record(E, curve, F, spec, 36)
        lk = LC.like(E, src, tw)
        assert prove(E, eng2, lk, 326) == prove(E, eng, tw, 326)
        assert eng2.prover_like_stats()[:2] == (1, 0) and eng.prover_like_stats()[:2] == (1, 4)
        # every handle of the recording freed: its bytes leave; a NEW recording of the same gadget with other public constants
        for r in likes + twins + [src, lk, tw]:
            r.p.free()
        assert eng.prover_like_stats()[2] == 0
        pspec = ("public", 6, 48)
        src2 = LC.record(E, curve, F, pspec, 37)
        tw2 = LC.record(E, curve, F, pspec, 37)
        assert src2.publics == tw2.publics and src2.publics != LC.record(E, curve, F, pspec, 38).publics
        lk2 = LC.like(E, src2, tw2)
        got = prove(E, eng, lk2, 327)
        assert got == prove(E, eng, tw2, 327)
        assert LC.verifier(E, curve, F, pspec, tw2.V, tw2.publics).verify(eng, got[0]) == 0
        up, hits, resident2, _, _ = eng.prover_like_stats()
        assert (up, hits) == (2, 4) and resident2 > 0
        # nine recordings in turn: at most 8 entries stay (the new recording above is the oldest and goes)
        keep = [src2, lk2]
        one_entry = None
        for j in range(9):
            s = LC.record(E, curve, F, ("single", 3, 60), 14)      # (the same gadget nine times: nine recordings, entries of one size)
            t = LC.record(E, curve, F, ("single", 3, 60), 15)
            k = LC.like(E, s, t)
            before = eng.prover_like_stats()[2]
            assert prove(E, eng, k, 330 + j) == prove(E, eng, t, 330 + j)
            keep += [s, k]
            if j == 0:
                one_entry = eng.prover_like_stats()[2] - before
                assert one_entry > 0
        up, hits, resident3, _, _ = eng.prover_like_stats()
        assert (up, hits) == (11, 4)
        assert resident3 == 8 * one_entry, "eight entries of the small gadget: the ninth lookup evicted the least recently used"
    finally:
        eng2.close()
        eng.close()


def edge_witness(F, n, seed):
    """inputs of n multipliers containing 0, 1, r - 1 and random values"""
    import random

    rs = random.Random(seed)
    edge = [0, 1, F.p - 1]
    left = [edge[i % 3] if i % 4 == 0 else rs.randrange(F.p) for i in range(n)]
    right = [edge[(i // 4 + 1) % 3] if i % 4 in (0, 1) else rs.randrange(F.p) for i in range(n)]
    return left, right


def gates_prover(E, curve, F, n, seed):
    """n multipliers allocated with the edge witness and one row on the commitment (no row holds a constant that depends on the
    witness: every witness shares the recording); a wrong product would move A_O, t(x) and with them every later byte of the proof"""
    left, right = edge_witness(F, n, seed)
    r = LC.Rec()
    r.t = LC.transcript(E)
    r.p = E.ProverCS(curve, r.t)
    r.v, r.b = [F.w(7)], [F.w(9)]
    r.V, vars_ = r.p.commit(r.v, r.b)
    r.m = W.Model(F)
    r.m.val[vars_[0]] = 7
    rec = W.Recorder(r.p, r.m)
    for i in range(n):
        rec.allocate_multiplier((F.w(left[i]), F.w(right[i])))
    rec.constrain([(vars_[0], F.w(1)), (GD.ONE, F.w(F.p - 7))])
    r.spec, r.n1 = ("gates", n), n
    r.left, r.right = LC.multipliers(F, r.m, n)
    return r


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gate_kernel_at_the_block_edges(E, engines, oracle, curve, n):
    """the products come from k_r1cs_gate_out: counted on the device, checked by the guard's gate check against the assigned inputs,
    and every later stage of the proof reads them (the bytes equal the twin's, whose a_O the host formed)"""
    F, eng = GD.Field(oracle, curve), engines[(curve, None)]
    src = gates_prover(E, curve, F, n, 70)
    for guarded in (False, True):
        tw = gates_prover(E, curve, F, n, 71 + n)
        lk = LC.like(E, src, tw)
        if guarded:
            tw.p.set_check(True)
            lk.p.set_check(True)
        want = prove(E, eng, tw, 340)
        s0 = eng.prover_like_stats()
        got = prove(E, eng, lk, 340)
        s1 = eng.prover_like_stats()
        assert (s1[3] - s0[3], s1[4] - s0[4]) == (n, 0)
        assert got == want
        assert eng.last_unsatisfied() == []
    # the device check of a like-prover (its own upload reads the host's a_O: formed there, counted there)
    tw = gates_prover(E, curve, F, n, 72)
    lk = LC.like(E, src, tw)
    s0 = eng.prover_like_stats()
    rep = lk.p.check(eng)
    s1 = eng.prover_like_stats()
    assert rep == tw.p.check(eng) and rep.satisfied and (rep.gates_checked, rep.bad_gates) == (n, 0)
    assert (s1[3] - s0[3], s1[4] - s0[4]) == (0, n)


@pytest.mark.parametrize("curve", [0, 1])
def test_two_phase_like_prover_counts_its_gates_on_the_host(E, engines, oracle, curve):
    F, eng = GD.Field(oracle, curve), engines[(curve, None)]
    # (the program's randomized callbacks allocate variables with values their closure computed from the SOURCE's witness — callbacks are
    # shared with the recording — so its like-prover holds the source's witness; the shuffle's callbacks only multiply and constrain)
    for spec, n1, seed in ((("shuffle", 4), 0, 17), (("program2", 4, 49), 4, 16)):
        src = LC.record(E, curve, F, spec, 16)
        tw = LC.record(E, curve, F, spec, seed)
        lk = LC.like(E, src, tw)
        assert tw.n1 == n1
        s0 = eng.prover_like_stats()
        assert prove(E, eng, lk, 350) == prove(E, eng, tw, 350)
        s1 = eng.prover_like_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[3] - s0[3], s1[4] - s0[4]) == (0, 0, 0, n1), "no resident index, phase-1 gates on the host"


def violating(E, curve, F, spec, src, wit_seed):
    """(twin, like-prover) whose a_L of the last multiplier is off by 5 (a_O with it: the gates hold); with two multipliers that is
    constraint 2 alone"""
    tw = LC.record(E, curve, F, spec, wit_seed)
    i = tw.n1 - 1
    new_l = (tw.m.val[(1, i)] + 5) % F.p
    left = tw.left.copy()
    left[i] = F.w(new_l)
    lk = LC.like(E, src, tw, left=left)
    W.poke(E, tw.p, tw.m, 0, i, new_l)
    W.poke(E, tw.p, tw.m, 2, i, new_l * tw.m.val[(2, i)] % F.p)
    return tw, lk


@pytest.mark.parametrize("curve", [0, 1])
def test_guard(E, engines, oracle, curve):
    F, eng = GD.Field(oracle, curve), engines[(curve, None)]
    spec = ("single", 2, 50)
    src = LC.record(E, curve, F, spec, 18)
    # a satisfying witness: the guarded proof equals the unguarded one
    tw = LC.record(E, curve, F, spec, 19)
    plain, guarded = LC.like(E, src, tw), LC.like(E, src, tw)
    guarded.p.set_check(True)
    assert prove(E, eng, guarded, 360) == prove(E, eng, plain, 360) == prove(E, eng, tw, 360)
    # constraint 2 violated through the assigned vectors
    tw, lk = violating(E, curve, F, spec, src, 19)
    host = lk.p.check()
    assert host == tw.p.check() and (host.bad_gates, host.bad_constraints, host.first_bad_constraint) == (0, 1, 2)
    assert lk.p.check(eng) == host
    lk.p.set_check(True)
    buf = C.create_string_buffer(b"\xAA" * 4096, 4096)
    plen = C.c_size_t(4096)
    from ark_bulletproofs_amd import _lib as L

    rc = L.lib().bp_prover_prove(eng.ctx, lk.p.h, LC.rng(361), buf, C.byref(plen), None)
    assert rc == E_UNSATISFIED
    assert buf.raw == b"\xAA" * 4096, "no proof bytes are written"
    assert eng.last_unsatisfied() == [(0, host)]
    # check_batch over a mix of like and self-recorded provers equals the per-prover reports
    tw2, lk2 = violating(E, curve, F, spec, src, 21)
    good_tw = LC.record(E, curve, F, spec, 22)
    good_lk = LC.like(E, src, good_tw)
    sh = LC.record(E, curve, F, ("shuffle", 3), 23)
    sh_lk = LC.like(E, LC.record(E, curve, F, ("shuffle", 3), 24), sh)
    mix = [lk2.p, good_tw.p, good_lk.p, tw2.p, sh_lk.p, sh.p, src.p]
    each = [p.check(eng) for p in mix]
    assert eng.check_batch(mix) == each
    assert each[0] == each[3] and not each[0].satisfied and each[1] == each[2] and each[2].satisfied and each[4] == each[5]


def _batch_members(E, curve, F, spec, wit0, bad=None, unassigned=None):
    """6 provers — 3 like-provers of one recording, 1 like-prover of another, 2 self-recorded — and their twins"""
    srcA, srcB = LC.record(E, curve, F, spec, 80), LC.record(E, curve, F, spec, 81)
    twins = [LC.record(E, curve, F, spec, wit0 + j) for j in range(6)]
    provers = []
    for j in range(6):
        if j == bad:
            tw, lk = violating(E, curve, F, spec, srcA, wit0 + j)
            twins[j] = tw
            provers.append(lk)
        elif j < 3:
            provers.append(LC.like(E, srcA, twins[j], assign=j != unassigned))
        elif j == 3:
            provers.append(LC.like(E, srcB, twins[j]))
        else:
            provers.append(LC.record(E, curve, F, spec, wit0 + j))
    return provers, twins, (srcA, srcB)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("spec", [("single", 3, 51), ("shuffle", 2)], ids=["single3", "shuffle2"])
def test_batch(E, engines, oracle, curve, spec):
    F, eng = GD.Field(oracle, curve), engines[(curve, None)]
    rngs = [LC.rng(400 + j) for j in range(6)]
    singles = None
    for front in (1, 0):
        eng.set_tuning(TUNE_PROVE_BATCH_FRONT, front)
        try:
            provers, twins, keep = _batch_members(E, curve, F, spec, 90)
            if singles is None:
                singles = [prove(E, eng, tw, 400 + j) for j, tw in enumerate(twins)]
                assert len(set(p for p, _ in singles)) == 6
            f0 = eng.prove_batch_front_stats()
            got = eng.prove_batch([r.p for r in provers], rngs)
            f1 = eng.prove_batch_front_stats()
            assert [st for st, _ in got] == [0] * 6
            assert [(pf, E.transcript_state(r.t)) for (_, pf), r in zip(got, provers)] == singles, "front = %d" % front
            assert f1[0] - f0[0] == (6 if front else 0), "every member runs its front stages in a group"
        finally:
            eng.set_tuning(TUNE_PROVE_BATCH_FRONT, 1)
    assert LC.verifier(E, curve, F, spec, twins[0].V).verify(eng, singles[0][0]) == 0
    if spec[0] != "single":
        return
    # one like-prover with an unsatisfying witness and the guard on fails alone
    for front in (1, 0):
        eng.set_tuning(TUNE_PROVE_BATCH_FRONT, front)
        try:
            provers, twins, keep = _batch_members(E, curve, F, spec, 90, bad=1)
            want_rep = provers[1].p.check()
            for r in provers:
                r.p.set_check(True)
            got = eng.prove_batch([r.p for r in provers], rngs)
            assert [st for st, _ in got] == [0, E_UNSATISFIED, 0, 0, 0, 0] and got[1][1] == b""
            assert [pf for j, (_, pf) in enumerate(got) if j != 1] == [singles[j][0] for j in range(6) if j != 1]
            assert eng.last_unsatisfied() == [(1, want_rep)]
        finally:
            eng.set_tuning(TUNE_PROVE_BATCH_FRONT, 1)
    # an unassigned like-prover: the whole batch is refused up front and consumes nothing
    provers, twins, keep = _batch_members(E, curve, F, spec, 90, unassigned=2)
    states = [E.transcript_state(r.t) for r in provers]
    with pytest.raises(E.ArkbpError) as ei:
        eng.prove_batch([r.p for r in provers], rngs)
    assert ei.value.code == E_ARG and "instance 2" in str(ei.value)
    assert [E.transcript_state(r.t) for r in provers] == states
    provers[2].p.assign_multipliers(twins[2].left, twins[2].right)
    got = eng.prove_batch([r.p for r in provers], rngs)
    assert [pf for _, pf in got] == [pf for pf, _ in singles]
