"""Verifier commitments from compressed bytes on the GPU (include/arkbp.h "Commitments from the wire"): the immediate batch form
(one k_points_decompress launch for all verifiers of a call), the prologue every verifying entry point runs for handles with pending
wire commitments, and the device front end, where k_vfe_points decodes the commitments itself (Shape::vwire) and they never reach
the host.  Every result is compared with the same call over affine commitments (bp_verifier_commit): statuses and check points; the
counters of bp_ctx_commit_wire_stats and bp_ctx_vfe_stats show which route ran."""
import numpy as np
import pytest

import commit_wire_common as CW
import gadgets as GD

pytestmark = pytest.mark.gpu
OK, E_VERIFICATION, E_FORMAT = 0, -4, -6
TUNE_VFY_DEVICE = 11


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def ctx(request, oracle):
    """(engine module, engine, oracle, field, proof cache)"""
    from ark_bulletproofs_amd import engine as E

    eng = E.Engine(curve=request.param, device=0)
    eng.gens_derive(CW.GENS)
    cache = {}

    def items(m, two_phase, distinct=3):
        key = (m, two_phase)
        if key not in cache:
            cache[key] = CW.prove_items(oracle, request.param, F, distinct, m, two_phase)
        return cache[key]

    F = GD.Field(oracle, request.param)
    yield E, eng, oracle, F, items
    eng.close()


def batch(items, P):
    return [items[k % len(items)][0] for k in range(P)], [items[k % len(items)][1] for k in range(P)]


def tamper(proof):
    b = bytearray(proof); b[363 + 5] ^= 4     # t_x
    return bytes(b)


def alphas_for(O, cv, n):
    return O.fe_rand(O.fid(cv, True), bytes([8]) * 32, n)


@pytest.mark.parametrize("count", [1, 2, 67])
def test_immediate_batch_form(ctx, count):
    E, eng, O, F, items = ctx
    cv = eng.curve
    ms = [(0, 1, 5)[k % 3] for k in range(count)]
    its = {m: items(m, False) for m in set(ms)}
    Vs = [its[m][k % 3][1] for k, m in enumerate(ms)]
    aff = [E.VerifierCS(cv, E.HostTranscript(CW.LABEL)) for _ in range(count)]
    wir = [E.VerifierCS(cv, E.HostTranscript(CW.LABEL)) for _ in range(count)]
    want = [v.commit(V) for v, V in zip(aff, Vs)]
    g0 = eng.commit_wire_stats()
    got = eng.verifier_commit_compressed_batch(wir, [CW.wire(O, cv, V) for V in Vs], defer=False)
    g1 = eng.commit_wire_stats()
    assert (g1[0] - g0[0], g1[1] - g0[1], g1[2] - g0[2]) == (0, sum(ms), 0)
    assert got == want
    for a, w, m, vars_ in zip(aff, wir, ms, got):
        assert w.metrics()[2] == m
        assert E.transcript_state(w.transcript()) == E.transcript_state(a.transcript())
        for v in (a, w):
            GD.random_program(v, F, 41, None, vars_, publics=[], **CW.KW)
    # V itself comes back through verifications that succeed (and one that must not)
    proofs = [its[m][k % 3][0] for k, m in enumerate(ms)]
    if count > 1:
        proofs[1] = tamper(proofs[1])
    rc_a, st_a, pt_a = eng.verify_each(aff, proofs, want_points=True)
    rc_w, st_w, pt_w = eng.verify_each(wir, proofs, want_points=True)
    assert st_a == [E_VERIFICATION if (count > 1 and k == 1) else OK for k in range(count)]
    assert rc_w == rc_a and st_w == st_a and (pt_w == pt_a).all()


@pytest.mark.parametrize("entry", ["verify", "batch_verify", "verify_batch", "locate"])
def test_prologue_route(ctx, entry):
    E, eng, O, F, items = ctx
    cv = eng.curve
    P, m = (1, 3) if entry == "verify" else (6, 3)
    pf, Vs = batch(items(m, False), P)
    if entry == "locate":
        pf[4] = tamper(pf[4])
    al = alphas_for(O, cv, P)

    def call(wired):
        vs = CW.verifiers(E, O, cv, F, Vs, False, wired=wired)
        if entry == "verify":
            return vs[0].verify(eng, pf[0]),
        if entry == "batch_verify":
            rc, pt = E.batch_verify_cs(eng, vs, pf, al, want_point=True)
            return rc, pt.tolist()
        if entry == "verify_batch":
            rc, st, pts = eng.verify_each(vs, pf, want_points=True)
            return rc, st, pts.tolist()
        return E.batch_verify_locate_cs(eng, vs, pf, al)

    eng.set_tuning(TUNE_VFY_DEVICE, 0)
    try:
        ref = call(False)
        g0 = eng.commit_wire_stats()
        got = call(True)
        g1 = eng.commit_wire_stats()
    finally:
        eng.set_tuning(TUNE_VFY_DEVICE, 1)
    assert got == ref
    assert ref[0] == (E_VERIFICATION if entry == "locate" else OK)
    if entry == "locate":
        assert ref[1] == [OK, OK, OK, OK, E_VERIFICATION, OK]
    assert (g1[0] - g0[0], g1[1] - g0[1], g1[2] - g0[2]) == (0, P * m, 0)


def device_pair(ctx, P, m, two_phase, pf, Vs, blobs=None, Vs_affine=None):
    """the same batch with affine commits and with deferred wire commits through the device front end: (affine, wire) results as
    (rc, check point), the vfe_stats deltas of the wire run and its commit_wire_stats deltas"""
    E, eng, O, F, _ = ctx
    cv = eng.curve
    al = alphas_for(O, cv, P)
    eng.set_tuning(TUNE_VFY_DEVICE, 2 if two_phase else 1)
    try:
        rc_a, pt_a = E.batch_verify_cs(eng, CW.verifiers(E, O, cv, F, Vs_affine if Vs_affine is not None else Vs, two_phase, wired=False), pf, al, want_point=True)
        vs = CW.verifiers(E, O, cv, F, Vs, two_phase, wired=True, blobs=blobs)
        d0, f0 = eng.vfe_stats()
        g0 = eng.commit_wire_stats()
        rc_w, pt_w = E.batch_verify_cs(eng, vs, pf, al, want_point=True)
        d1, f1 = eng.vfe_stats()
        g1 = eng.commit_wire_stats()
    finally:
        eng.set_tuning(TUNE_VFY_DEVICE, 1)
    return (rc_a, pt_a), (rc_w, pt_w), (d1 - d0, f1 - f0), tuple(b - a for a, b in zip(g0, g1))


@pytest.mark.parametrize("P,m", [(5, 3), (67, 5), (3, 0)])
def test_device_front_end_decodes_the_commitments(ctx, P, m):
    """the three lane regions of k_vfe_points (proof points | commitments | scalars) end inside a wavefront and inside a block"""
    pf, Vs = batch(ctx[4](m, False), P)
    for bad in (None, P - 2):
        pfb = list(pf)
        if bad is not None:
            pfb[bad] = tamper(pfb[bad])
        (rc_a, pt_a), (rc_w, pt_w), vfe, cw = device_pair(ctx, P, m, False, pfb, Vs)
        assert vfe == (1, 0), "the device front end did not take the batch of pending wire commitments"
        assert cw == (P * m, 0, 0)
        assert rc_a == rc_w == (OK if bad is None else E_VERIFICATION)
        assert (pt_a == pt_w).all() and pt_w.any() == (bad is not None)


def test_device_front_end_two_phase(ctx):
    P, m = 5, 2
    pf, Vs = batch(ctx[4](m, True), P)
    for bad in (None, 3):
        pfb = list(pf)
        if bad is not None:
            pfb[bad] = tamper(pfb[bad])
        (rc_a, pt_a), (rc_w, pt_w), vfe, cw = device_pair(ctx, P, m, True, pfb, Vs)
        assert vfe == (1, 0)
        assert cw[0] == P * m and cw[1] + cw[2] <= m, "more host roots than instance 0's rehearsal"
        assert rc_a == rc_w == (OK if bad is None else E_VERIFICATION)
        assert (pt_a == pt_w).all() and pt_w.any() == (bad is not None)


def test_identity_commitment_on_the_device_route(ctx):
    E, eng, O, F, items = ctx
    P, m = 5, 3
    pf, Vs = batch(items(m, False), P)
    ident = bytes(32) + b"\x40"
    blobs = [None] * P
    blobs[2] = CW.wire(O, eng.curve, Vs[2][:1]) + ident + CW.wire(O, eng.curve, Vs[2][2:])
    Vz = [v.copy() for v in Vs]
    Vz[2][1] = 0
    (rc_a, pt_a), (rc_w, pt_w), vfe, cw = device_pair(ctx, P, m, False, pf, Vs, blobs=blobs, Vs_affine=Vz)
    assert vfe == (1, 0) and cw == (P * m, 0, 0)
    assert rc_a == rc_w == E_VERIFICATION and pt_w.any() and (pt_a == pt_w).all()


def test_rejected_encoding_in_a_device_eligible_batch(ctx):
    E, eng, O, F, items = ctx
    cv = eng.curve
    P, m = 5, 3
    pf, Vs = batch(items(m, False), P)
    bad = bytearray(CW.wire(O, cv, Vs[3])); bad[2 * 33 + 32] = 0xC0
    blobs = [None] * P; blobs[3] = bytes(bad)
    al = alphas_for(O, cv, P)
    d0, f0 = eng.vfe_stats()
    assert E.batch_verify_cs(eng, CW.verifiers(E, O, cv, F, Vs, False, wired=True, blobs=blobs), pf, al) == E_FORMAT
    d1, f1 = eng.vfe_stats()
    assert (d1 - d0, f1 - f0) == (0, 1)
    rc, st = E.batch_verify_locate_cs(eng, CW.verifiers(E, O, cv, F, Vs, False, wired=True, blobs=blobs), pf, al)
    assert rc == E_FORMAT and st == [OK, OK, OK, E_FORMAT, OK]
    # the other two entry points: bp_verifier_verify_batch leaves the instance out and goes on, bp_verifier_verify returns it
    vs = CW.verifiers(E, O, cv, F, Vs, False, wired=True, blobs=blobs)
    rc, st = eng.verify_each(vs[:4], pf[:4])
    assert rc == E_FORMAT and st == [OK, OK, OK, E_FORMAT]
    assert vs[4].verify(eng, pf[4]) == OK
    v3 = CW.verifiers(E, O, cv, F, Vs[3:4], False, wired=True, blobs=blobs[3:4])[0]
    assert v3.verify(eng, tamper(pf[3])) == E_FORMAT and v3.metrics()[2] == 0     # (before the proof's own VerificationError; nothing committed)
    # an x that is on no curve point: the device's square root decides
    x = 1
    while O.point_deser_compressed(cv, (x + 1).to_bytes(32, "little") + b"\x00") is not None:
        x += 1
    bad = bytearray(CW.wire(O, cv, Vs[3])); bad[0:33] = (x + 1).to_bytes(32, "little") + b"\x00"
    blobs[3] = bytes(bad)
    rc, st = E.batch_verify_locate_cs(eng, CW.verifiers(E, O, cv, F, Vs, False, wired=True, blobs=blobs), pf, al)
    assert rc == E_FORMAT and st == [OK, OK, OK, E_FORMAT, OK]


def test_ark_layout_commitments_after_a_wire_batch(ctx):
    """the shape flag does not stick: bp_debug_vfe_challenges (ark-layout commitments) after a wire batch on the same ctx gives the
    host transcript's challenges"""
    from test_gpu_vfe import parse_proof, replay

    E, eng, O, F, items = ctx
    cv = eng.curve
    P, m = 5, 3
    pf, Vs = batch(items(m, False), P)
    _, (rc_w, _), vfe, _ = device_pair(ctx, P, m, False, pf, Vs)
    assert rc_w == OK and vfe == (1, 0)
    t0 = E.HostTranscript(CW.LABEL)
    t0.append_message(b"dom-sep", b"r1cs v1")
    state = E.transcript_state(t0)
    seeds, chal, status = eng.debug_vfe_challenges(pf, np.stack(Vs), state, True)
    assert status == 0
    for i in range(P):
        k, pts, scal, L, R = parse_proof(O, cv, pf[i])
        th = E.transcript_from_state(state)
        exp = replay(th, cv, m, k, Vs[i], pts, scal, L, R, lambda T, l, p: T.append_point(cv, l, p), lambda T, l, b: T.append_message(l, b),
                     lambda T, l: T.challenge_scalar(cv, l))
        assert (np.stack(exp) == chal[i]).all()
