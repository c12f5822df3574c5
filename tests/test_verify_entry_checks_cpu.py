"""The up-front checks of the three entry points over verifier handle arrays — bp_r1cs_batch_verify (batch_verify_cs),
bp_verifier_verify_batch (verify_each) and bp_r1cs_batch_verify_locate (batch_verify_locate_cs) — on a host-only ctx: ONE table of
defective inputs, and for every (defect, entry point) the return code, the full bp_last_error() text and that no handle was consumed.
The expected values are what the library returned when the three entry points still carried a copy of the checks each; the order in
which an entry point looks at two defects at once is part of them (bp_r1cs_batch_verify looks at pending wire commitments before the
generators and runs on a host-only ctx as a dry run; the other two answer BP_E_NO_DEVICE before they look at pending commitments).
Left out: rows that bp_r1cs_batch_verify would accept (a clean batch, a like-instance short of commitments) — its dry run consumes."""
import ctypes as C

import numpy as np
import pytest

OK, E_ARG, E_NO_DEVICE, E_GENS_LENGTH = 0, -1, -3, -5
CURVES = pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])
BV, VE, VL = "batch_verify", "verify_each", "batch_verify_locate"
SENTINEL = "set_blinding: not a prover handle"
LABEL = b"verify entry checks"


def _reset_err(L):
    """leaves a known text in bp_last_error(): a refusal that sets none shows as this one"""
    assert L.bp_prover_set_blinding(None, 0) == E_ARG and L.bp_last_error().decode() == SENTINEL


def _live(L, h):
    """not consumed — asked without touching the handle: outside the randomized phase bp_cs_challenge_scalar refuses a live handle
    with a message, a consumed one without"""
    _reset_err(L)
    assert L.bp_cs_challenge_scalar(h, b"x", (C.c_uint64 * 4)()) == E_ARG
    return L.bp_last_error().decode().startswith("challenge_scalar is only available")


def _verifier(E, curve):
    v = E.VerifierCS(curve, E.HostTranscript(LABEL))
    v.commit(E.pedersen_gens(curve)[0].reshape(1, 8))
    return v


def _consumed(E, curve, eng):
    v = _verifier(E, curve)
    v.verify(eng, b"\0" * 32)   # (the dry run of a host-only ctx consumes like the real call)
    return v


def _moved(E, curve):
    """pending wire commitments, then the transcript moves on"""
    v = E.VerifierCS(curve, E.HostTranscript(LABEL))
    v.commit_compressed(E.points_compress(curve, E.pedersen_gens(curve)[:1]), defer=True)
    v.transcript().append_message(b"extra", b"bound behind our back")
    return v


def _short(E, curve):
    """(recording, like-instance that holds one of the two commitments the shared constraints name)"""
    v0 = E.VerifierCS(curve, E.HostTranscript(LABEL))
    pts = E.pedersen_gens(curve)
    x, y = v0.commit(np.stack([pts[0], pts[1]]).reshape(2, 8))
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    v0.constrain([(x, one), (y, one)])
    short = E.VerifierCS(curve, E.HostTranscript(LABEL), like=v0)
    short.commit(pts[0].reshape(1, 8))
    return [v0, short]


# name -> (generators installed, handles(E, curve, eng) -> list, weights: "ones" | None | "zero", entry points)
CASES = {
    "clean": (True, lambda E, cv, eng: [_verifier(E, cv), _verifier(E, cv)], "ones", (VE, VL)),
    "consumed": (True, lambda E, cv, eng: [_verifier(E, cv), _consumed(E, cv, eng)], "ones", (BV, VE, VL)),
    "prover": (True, lambda E, cv, eng: [E.ProverCS(cv, E.HostTranscript(LABEL)), _verifier(E, cv)], "ones", (BV, VE, VL)),
    "other_curve": (True, lambda E, cv, eng: [_verifier(E, cv), _verifier(E, 1 - cv)], "ones", (BV, VE, VL)),
    "twice": (True, lambda E, cv, eng: (lambda a, b: [a, b, a])(_verifier(E, cv), _verifier(E, cv)), "ones", (BV, VE, VL)),
    "no_weights": (True, lambda E, cv, eng: [_verifier(E, cv), _verifier(E, cv)], None, (BV, VL)),
    "zero_weight": (True, lambda E, cv, eng: [_verifier(E, cv), _verifier(E, cv)], "zero", (VL,)),
    "short_like": (True, lambda E, cv, eng: _short(E, cv), "ones", (VE, VL)),
    "no_gens": (False, lambda E, cv, eng: [_verifier(E, cv), _verifier(E, cv)], "ones", (BV, VE, VL)),
    "moved": (True, lambda E, cv, eng: [_verifier(E, cv), _moved(E, cv)], "ones", (BV, VE, VL)),
    # two defects at once
    "twice+no_gens": (False, lambda E, cv, eng: (lambda a, b: [a, b, a])(_verifier(E, cv), _verifier(E, cv)), "ones", (BV, VE, VL)),
    "no_gens+moved": (False, lambda E, cv, eng: [_verifier(E, cv), _moved(E, cv)], "ones", (BV, VE, VL)),
    "consumed+no_weights": (True, lambda E, cv, eng: [_verifier(E, cv), _consumed(E, cv, eng)], None, (BV, VL)),
}

LIVE_VERIFIER = ": every instance needs a live verifier of the ctx's curve"
ONE_INSTANCE = ": a verifier is consumed by ONE instance"
NO_GENS = ": generators not installed"
NO_DEVICE = ": a host-only ctx has no device to verify on"
NEED_WEIGHTS = ": per-instance weights (alphas) are required for more than one instance"
MOVED_1 = ": instance 1: the transcript changed while wire commitments were pending (bp_verifier_materialize before binding more data)"
PFX = {BV: "batch_verify", VE: "verify_batch", VL: "batch_verify_locate"}

# (case, entry point) -> (return code, bp_last_error() without the entry point's prefix)
EXPECTED = {
    ("clean", VE): (E_NO_DEVICE, NO_DEVICE),
    ("clean", VL): (E_NO_DEVICE, NO_DEVICE),
    ("consumed", BV): (E_ARG, LIVE_VERIFIER),
    ("consumed", VE): (E_ARG, LIVE_VERIFIER),
    ("consumed", VL): (E_ARG, LIVE_VERIFIER),
    ("prover", BV): (E_ARG, LIVE_VERIFIER),
    ("prover", VE): (E_ARG, LIVE_VERIFIER),
    ("prover", VL): (E_ARG, LIVE_VERIFIER),
    ("other_curve", BV): (E_ARG, LIVE_VERIFIER),
    ("other_curve", VE): (E_ARG, LIVE_VERIFIER),
    ("other_curve", VL): (E_ARG, LIVE_VERIFIER),
    ("twice", BV): (E_ARG, ONE_INSTANCE),
    ("twice", VE): (E_ARG, ONE_INSTANCE),
    ("twice", VL): (E_ARG, ONE_INSTANCE),
    ("no_weights", BV): (E_ARG, NEED_WEIGHTS),
    ("no_weights", VL): (E_ARG, NEED_WEIGHTS),
    ("zero_weight", VL): (E_ARG, ": a zero weight hides its instance from every sum"),
    ("short_like", VE): (E_NO_DEVICE, NO_DEVICE),
    ("short_like", VL): (E_ARG, ": the constraints refer to more commitments than a verifier holds (bp_verifier_commit)"),
    ("no_gens", BV): (E_GENS_LENGTH, NO_GENS),
    ("no_gens", VE): (E_GENS_LENGTH, NO_GENS),
    ("no_gens", VL): (E_GENS_LENGTH, NO_GENS),
    ("moved", BV): (E_ARG, MOVED_1),
    ("moved", VE): (E_NO_DEVICE, NO_DEVICE),      # (a host-only ctx is refused before the pending commitments are looked at)
    ("moved", VL): (E_NO_DEVICE, NO_DEVICE),
    ("twice+no_gens", BV): (E_ARG, ONE_INSTANCE),
    ("twice+no_gens", VE): (E_ARG, ONE_INSTANCE),
    ("twice+no_gens", VL): (E_ARG, ONE_INSTANCE),
    ("no_gens+moved", BV): (E_ARG, MOVED_1),      # (bp_r1cs_batch_verify: pending commitments before the generators)
    ("no_gens+moved", VE): (E_GENS_LENGTH, NO_GENS),
    ("no_gens+moved", VL): (E_GENS_LENGTH, NO_GENS),
    ("consumed+no_weights", BV): (E_ARG, NEED_WEIGHTS),
    ("consumed+no_weights", VL): (E_ARG, NEED_WEIGHTS),
}


def run_case(E, L, curve, case, entry):
    """-> (return code, bp_last_error(), handles whose liveness changed, statuses the library wrote)"""
    gens, make, weights, _ = CASES[case]
    eng = E.Engine.host_only(curve, 64 if gens else 0)
    helper = E.Engine.host_only(curve, 64)   # (what consumes the "consumed" handle has generators in every row)
    try:
        vs = make(E, curve, helper)
        n = len(vs)
        hs = (C.c_void_p * n)(*[v.h for v in vs])
        lens = (C.c_size_t * n)(*([32] * n))
        proofs = b"\0" * (32 * n)
        al = None
        if weights is not None:
            al = np.ones((n, 4), dtype=np.uint64)
            if weights == "zero":
                al[1] = 0
        alp = al.ctypes.data_as(C.c_void_p) if al is not None else None
        st = (C.c_int * n)(*([7] * n))
        before = [_live(L, v.h) for v in vs]
        _reset_err(L)
        if entry == BV:
            rc = L.bp_r1cs_batch_verify(eng.ctx, C.c_size_t(n), hs, proofs, lens, alp, None, None)
        elif entry == VE:
            rc = L.bp_verifier_verify_batch(eng.ctx, C.c_size_t(n), hs, proofs, lens, st, None, None)
        else:
            rc = L.bp_r1cs_batch_verify_locate(eng.ctx, C.c_size_t(n), hs, proofs, lens, alp, st, None)
        msg = L.bp_last_error().decode()
        after = [_live(L, v.h) for v in vs]
        return rc, msg, [k for k in range(n) if before[k] != after[k]], [s for s in st if s != 7]
    finally:
        eng.close()
        helper.close()


def test_the_table_covers_every_case():
    assert set(EXPECTED) == {(case, entry) for case, (_, _, _, entries) in CASES.items() for entry in entries}


@CURVES
@pytest.mark.parametrize("case,entry", sorted(EXPECTED), ids=["%s-%s" % ce for ce in sorted(EXPECTED)])
def test_entry_checks(curve, case, entry):
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    rc, msg, changed, written = run_case(E, lib(), curve, case, entry)
    want_rc, want_tail = EXPECTED[(case, entry)]
    assert (rc, msg) == (want_rc, PFX[entry] + want_tail)
    assert changed == [], "a refused call consumed (or revived) a handle"
    assert written == [], "a refused call wrote statuses"
