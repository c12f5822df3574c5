"""Like-provers without a GPU (include/arkbp.h bp_prover_new_like, bp_prover_assign_multipliers): every refusal with "nothing
changed" checked, what the new handle inherits, the host twin of the witness check on a like-prover against a prover that recorded
the gadget itself, and the stand-alone host self-test of the constraint indices over a shared recording
(csrc/prove_like_selftest.cpp, built with the sanitizers and run as a child process; nothing of it is loaded into this process)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gadgets as GD
import likecommon as LC
import wcheck as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_bulletproofs_amd", "csrc")
OUT = os.path.join(ROOT, "ark_bulletproofs_amd", "_obj")


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def L(E):
    from ark_bulletproofs_amd import _lib

    return _lib


def _new_like_rc(L, of_h, t_h, out):
    return L.lib().bp_prover_new_like(of_h, t_h, out)


def _records(F, p, vars_):
    """phase-1 recording still works on p (and is undone by nothing: the caller compares metrics around it)"""
    p.constrain([(vars_[0], F.w(0))])


def test_exports(L):
    for name in ("bp_prover_new_like", "bp_prover_assign_multipliers", "bp_ctx_prover_like_stats"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().bp_ctx_prover_like_stats(None, None, None, None, None, None) == L.BP_E_ARG


@pytest.mark.parametrize("curve", [0, 1])
def test_refused_freezes_change_nothing(E, L, oracle, curve):
    F = GD.Field(oracle, curve)
    src = LC.record(E, curve, F, ("single", 3, 31), 1)
    t = LC.transcript(E)
    state = E.transcript_state(t)
    out = C.c_void_p()
    before = src.p.metrics()
    v = E.VerifierCS(curve, LC.transcript(E))
    vvars = v.commit(src.V)
    assert _new_like_rc(L, None, t.h, C.byref(out)) == L.BP_E_ARG
    assert _new_like_rc(L, v.h, t.h, C.byref(out)) == L.BP_E_ARG            # a verifier handle
    assert _new_like_rc(L, src.p.h, None, C.byref(out)) == L.BP_E_ARG
    assert _new_like_rc(L, src.p.h, t.h, None) == L.BP_E_ARG
    assert not out.value and E.transcript_state(t) == state, "a refused call touches neither the output nor the transcript"
    assert src.p.metrics() == before
    # nothing was frozen: both still record phase 1
    _records(F, src.p, [(0, 0)])
    v.constrain([(vvars[0], F.w(0))])
    assert src.p.metrics() == (before[0], before[1] + 1, before[2])
    # the verifier's own entry point refuses a prover, and nothing is frozen by that either
    assert L.lib().bp_verifier_new_like(src.p.h, t.h, C.byref(out)) == L.BP_E_ARG
    _records(F, src.p, [(0, 0)])
    # a prover whose head has run
    src.p.precompute(LC.rng(1))
    assert _new_like_rc(L, src.p.h, t.h, C.byref(out)) == L.BP_E_ARG
    _records(F, src.p, [(0, 0)])
    assert src.p.metrics() == (before[0], before[1] + 3, before[2]) and not out.value and E.transcript_state(t) == state


@pytest.mark.parametrize("curve", [0, 1])
def test_after_the_freeze_both_refuse_phase1_recording(E, L, oracle, curve):
    F = GD.Field(oracle, curve)
    src = LC.record(E, curve, F, ("single", 3, 32), 2)
    n, q, m = src.p.metrics()
    lk = LC.like(E, src, src, assign=False)
    assert lk.p.metrics() == (n, q, 3) and src.p.metrics() == (n, q, m)     # the shared counts; the like-prover's own commitments
    one = [((0, 0), F.w(1))]
    for p in (src.p, lk.p):
        with pytest.raises(E.ArkbpError) as ei:
            p.multiply(one, one)
        assert ei.value.code == L.BP_E_ARG and "bp_prover_new_like" in str(ei.value)
        for call in (lambda: p.constrain(one), lambda: p.allocate(F.w(1)), lambda: p.allocate_multiplier((F.w(1), F.w(2))),
                     lambda: p.allocate_multipliers([F.w(1)], [F.w(2)]), lambda: p.constrain_many([(0, 0)], [F.w(1)], [0, 1]),
                     lambda: p.specify_randomized_constraints(lambda cs: None)):
            with pytest.raises(E.ArkbpError) as ei:
                call()
            assert ei.value.code == L.BP_E_ARG
        with pytest.raises(E.ArkbpError):
            p.challenge_scalar(b"x")      # (still only inside the randomized phase)
    assert lk.p.metrics() == (n, q, 3) and src.p.metrics() == (n, q, m)
    # commits are still taken, by both; a second freeze shares the same recording
    src.p.commit([F.w(9)], [F.w(8)])
    lk.p.commit([F.w(9)], [F.w(8)])
    lk2 = LC.like(E, src, src, assign=False)
    lk3 = LC.like(E, lk, src, assign=False)          # a like-prover is a valid source too
    assert lk.p.metrics() == (n, q, 4) and src.p.metrics() == (n, q, m + 1) and lk2.p.metrics() == (n, q, 3) and lk3.p.metrics() == (n, q, 3)


@pytest.mark.parametrize("curve", [0, 1])
def test_inherits_pair_and_curve_and_starts_plain(E, L, oracle, curve):
    import pedersen_gens_common as PG

    F = GD.Field(oracle, curve)
    pair = PG.pair(curve, "chain")
    src = LC.record(E, curve, F, ("single", 3, 33), 3, pc_gens=pair)
    src.p.set_blinding(E.BLINDING_EXPANDED)
    src.p.set_check(True)
    t = LC.transcript(E)
    ref = LC.transcript(E)
    before = E.transcript_state(t)
    lk = src.p.new_like(t)
    # Prover::new's domain separator went into the transcript, nothing else
    probe = E.ProverCS(curve, ref)
    assert E.transcript_state(t) == E.transcript_state(ref) != before
    assert lk.curve == curve and lk.metrics() == (src.n1, src.p.metrics()[1], 0)
    assert lk.blinding == E.BLINDING_TRANSCRIPT and lk.checking() is False
    assert src.p.blinding == E.BLINDING_EXPANDED and src.p.checking() is True
    # the pair: commitments equal those of a prover created with it, and differ from the default pair's
    V, _ = lk.commit(src.v, src.b)
    assert (V == src.V).all()
    for i in range(len(V)):
        assert (V[i] == PG.commit_expected(oracle, curve, "chain", src.v[i], src.b[i])).all()
    Vd, _ = probe.commit(src.v, src.b)
    assert not (Vd == V).all()
    # a host-only engine holds the default pair: the like-prover's pair is checked against it like any prover's
    he = E.Engine.host_only(curve, 64)
    try:
        with pytest.raises(E.ArkbpError):
            lk.commit([F.w(1)], [F.w(1)], engine=he)
    finally:
        he.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_assign_refusals_change_nothing(E, L, oracle, curve):
    F = GD.Field(oracle, curve)
    lib = L.lib()
    src = LC.record(E, curve, F, ("single", 3, 34), 4)
    twin = LC.record(E, curve, F, ("single", 3, 34), 5)
    lk = LC.like(E, src, twin, assign=False)
    rep = E._WitnessReportC()
    rep.gates_checked = 4242
    n = C.c_size_t(3)

    def unassigned():
        """still without a witness: checking and the head of prove() refuse it, and nothing is written"""
        assert lib.bp_prover_check(None, lk.p.h, C.byref(rep)) == L.BP_E_ARG and rep.gates_checked == 4242
        assert lib.bp_prover_precompute(lk.p.h, LC.rng(2)) == L.BP_E_ARG
        assert "bp_prover_assign_multipliers" in lib.bp_last_error().decode()

    unassigned()
    l, r = twin.left, twin.right
    assert lib.bp_prover_assign_multipliers(None, L.ptr(l), L.ptr(r), n) == L.BP_E_ARG
    assert lib.bp_prover_assign_multipliers(lk.p.h, None, L.ptr(r), n) == L.BP_E_ARG
    assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(l), None, n) == L.BP_E_ARG
    assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(l), L.ptr(r), C.c_size_t(2)) == L.BP_E_ARG      # the wrong count
    l4 = np.concatenate([l, l[:1]])
    assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(l4), L.ptr(l4), C.c_size_t(4)) == L.BP_E_ARG
    assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(l), L.ptr(r), C.c_size_t(0)) == L.BP_E_ARG
    modulus = np.array([(F.p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    for pos in (0, 2):                                                                                     # words at or above r
        bad = l.copy()
        bad[pos] = modulus
        assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(bad), L.ptr(r), n) == L.BP_E_ARG
        assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(l), L.ptr(bad), n) == L.BP_E_ARG
        bad[pos] = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(bad), L.ptr(r), n) == L.BP_E_ARG
    # a prover that is not a like-prover: the recording's source, a plain prover, a verifier
    assert lib.bp_prover_assign_multipliers(src.p.h, L.ptr(l), L.ptr(r), n) == L.BP_E_ARG
    assert lib.bp_prover_assign_multipliers(twin.p.h, L.ptr(l), L.ptr(r), n) == L.BP_E_ARG
    v = E.VerifierCS(curve, LC.transcript(E))
    assert lib.bp_prover_assign_multipliers(v.h, L.ptr(l), L.ptr(r), n) == L.BP_E_ARG
    unassigned()
    # the one valid call, then a second one is refused and leaves the first in place
    lk.p.assign_multipliers(l, r)
    good = lk.p.check()
    assert good == twin.p.check() and good.satisfied
    other = LC.record(E, curve, F, ("single", 3, 34), 6)
    assert lib.bp_prover_assign_multipliers(lk.p.h, L.ptr(other.left), L.ptr(other.right), n) == L.BP_E_ARG
    assert lk.p.check() == good
    # fewer commitments than the shared constraints name: refused like the verifier's like-instances
    short = LC.Rec()
    short.t = LC.transcript(E)
    short.p = src.p.new_like(short.t)
    short.p.commit(twin.v[:1], twin.b[:1])
    short.p.assign_multipliers(l, r)
    assert lib.bp_prover_check(None, short.p.h, C.byref(rep)) == L.BP_E_ARG and rep.gates_checked == 4242
    assert "fewer commitments" in lib.bp_last_error().decode()
    assert lib.bp_prover_precompute(short.p.h, LC.rng(3)) == L.BP_E_ARG
    short.p.commit(twin.v[1:], twin.b[1:])
    assert short.p.check() == good


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("spec", [("single", 1, 35), ("single", 5, 36), ("public", 6, 37), ("program2", 4, 38), ("shuffle", 3)], ids=lambda s: "%s%d" % (s[0], s[1]))
def test_host_check_equals_the_recorded_provers(E, L, oracle, curve, spec):
    """bp_prover_check with a NULL ctx and with a host-only ctx: the like-prover's report is the self-recorded prover's, field by
    field, for a satisfying witness and for one that violates a single constraint through the assigned vectors (its gates hold: a_O
    is the product of what was assigned); then a poked a_O is seen."""
    F = GD.Field(oracle, curve)
    he = E.Engine.host_only(curve, 64)
    try:
        src = LC.record(E, curve, F, spec, 7)
        if spec[0] == "public":
            src = LC.record(E, curve, F, spec, 8)      # (public constants: the recording fits this witness only)
        twin = LC.record(E, curve, F, spec, 8)
        lk = LC.like(E, src, twin)
        deferred = 0 if spec[0] in ("single", "public") else 1
        want = twin.p.check()
        assert W.observed(F, want) == twin.m.expect(deferred) and want.satisfied
        for got in (lk.p.check(), lk.p.check(he), he.check_batch([lk.p])[0], src.p.check() if spec[0] == "public" else want):
            assert got == want
        assert lk.p.metrics() == twin.p.metrics()
        if twin.n1 == 0 or spec[0] == "public":
            return
        # the last multiplier's inputs enter no later row: changing a_L there (a_O with it) violates its own left row alone
        i = twin.n1 - 1
        new_l = (twin.m.val[(1, i)] + 5) % F.p
        left = twin.left.copy()
        left[i] = F.w(new_l)
        twin2 = LC.record(E, curve, F, spec, 8)
        W.poke(E, twin2.p, twin2.m, 0, i, new_l)
        W.poke(E, twin2.p, twin2.m, 2, i, new_l * twin2.m.val[(2, i)] % F.p)
        lk2 = LC.like(E, src, twin, left=left)
        want2 = twin2.p.check()
        assert W.observed(F, want2) == twin2.m.expect(deferred)
        rows = [q for q, row in enumerate(twin2.m.rows) if any(tuple(v) in ((1, i), (3, i)) for v, _ in row)]
        assert (want2.bad_gates, want2.bad_constraints, want2.first_bad_constraint) == (0, len(rows), rows[0]) and len(rows) == 1
        assert F.i(want2.first_bad_residual) == F.p - 5
        for got in (lk2.p.check(), lk2.p.check(he)):
            assert got == want2 and got.bad_gates == 0
        # poke a_O of multiplier 0 on the like-prover: the host twin sees the gate (and whatever rows name the output)
        val = (twin.m.val[(3, 0)] + 1) % F.p
        E.debug_poke_witness(lk.p, 2, 0, F.w(val))
        W.poke(E, twin.p, twin.m, 2, 0, val)
        got = lk.p.check()
        assert got == twin.p.check() and (got.bad_gates, got.first_bad_gate) == (1, 0)
        assert W.observed(F, lk.p.check(he)) == twin.m.expect(deferred)
    finally:
        he.close()


def test_index_over_a_shared_recording_selftest():
    """csrc/prove_like_selftest.cpp: the indices of base + own terms equal those of the same constraints recorded flat, n = 1, 3, 257"""
    exe = os.path.join(OUT, "prove_like_selftest")
    srcs = [os.path.join(CSRC, f) for f in ("prove_like_selftest.cpp", "prove_steps.hpp", "host_proto.hpp", "host_math.hpp", "keccak_unrolled.inc", "arkbp_params.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs)):
        os.makedirs(OUT, exist_ok=True)
        base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-o", exe, srcs[0]]
        r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
        if r.returncode != 0:
            assert "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr, r.stderr[-3000:]   # (only a missing runtime is excused)
            subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prove_like selftest ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
