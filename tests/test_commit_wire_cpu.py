"""Verifier commitments from compressed bytes, without a GPU (include/arkbp.h "Commitments from the wire"): the public codec on a
host-only ctx against the oracle's serializer, deferred wire commitments against bp_verifier_commit (transcript state, commitment
count, variables), the transcript-state check that guards pending commitments, and the host-only dry run of bp_r1cs_batch_verify,
whose check point is the checksum of everything the host staged."""
import ctypes as C

import numpy as np
import pytest

import commit_wire_common as CW
import gadgets as GD

OK, E_ARG, E_FORMAT = 0, -1, -6
CURVES = pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])


@pytest.fixture()
def E():
    from ark_bulletproofs_amd import engine

    return engine


def reject_set(O, cv, enc0):
    """as test_gpu_primitives.py::test_point_decompression_on_gpu builds it: x off the curve, both flags, low flag bits, x >= p,
    identity flag with x != 0"""
    bad, x = [], 1
    q = O.modulus(O.fid(cv, False))
    while len(bad) < 5:
        x += 1
        b = x.to_bytes(32, "little") + b"\x00"
        if O.point_deser_compressed(cv, b) is None:
            bad.append(b)
    bad += [enc0[:32] + b"\xc0", enc0[:32] + b"\x01", q.to_bytes(32, "little") + b"\x00", enc0[:32] + b"\x40"]
    for b in bad:
        assert O.point_deser_compressed(cv, b) is None
    return bad


def some_points(O, cv, n, seed=7):
    B, Bb = O.pedersen_default(cv)
    sc = O.fe_rand(O.fid(cv, True), bytes([seed]) * 32, n)
    return np.array([O.scalar_mul(cv, B if i % 2 else Bb, sc[i]) for i in range(n)], dtype=np.uint64).reshape(n, 8)


@CURVES
def test_codec_round_trip_on_a_host_only_ctx(E, oracle, curve):
    O = oracle
    eng = E.Engine.host_only(curve, 0)
    try:
        G, H = O.bp_gens(curve, 6)
        pts = np.concatenate([G, H, np.zeros((1, 8), dtype=np.uint64)])
        enc = E.points_compress(curve, pts)
        assert enc == b"".join(O.point_ser(curve, p, True) for p in pts[:-1]) + bytes(32) + b"\x40"
        out, ok = eng.points_decompress(enc)
        assert ok.all() and (out == pts).all()
        for i in range(len(pts) - 1):
            assert (out[i] == O.point_deser_compressed(curve, enc[33 * i:33 * i + 33])).all()
        # both roots of one x
        flipped = bytearray(enc[:33]); flipped[32] ^= 0x80
        o2, ok2 = eng.points_decompress(bytes(flipped))
        assert ok2[0] and (o2[0, :4] == pts[0, :4]).all() and (O.point_add(curve, o2[0], pts[0]) == 0).all()
        assert E.points_compress(curve, o2) == bytes(flipped)
        # the test hook is the same function
        o3, ok3 = eng.debug_decompress(enc)
        assert ok3.all() and (o3 == pts).all()
        assert eng.points_decompress(b"")[1].size == 0
    finally:
        eng.close()


@CURVES
def test_codec_rejects(E, oracle, curve):
    from ark_bulletproofs_amd._lib import lib

    O = oracle
    eng = E.Engine.host_only(curve, 0)
    try:
        G, _ = O.bp_gens(curve, 1)
        enc0 = O.point_ser(curve, G[0], True)
        bad = reject_set(O, curve, enc0)
        mixed = b"".join(bad[:3]) + enc0 + b"".join(bad[3:])
        out, ok = eng.points_decompress(mixed)
        assert list(ok) == [0, 0, 0, 1] + [0] * (len(bad) - 3)
        assert not out[:3].any() and not out[4:].any() and (out[3] == G[0]).all()
        # an affine input off the curve
        off = G[0].copy(); off[4] ^= np.uint64(1)
        buf = C.create_string_buffer(66)
        two = np.ascontiguousarray(np.stack([G[0], off]))
        assert lib().bp_points_compress(curve, two.ctypes.data_as(C.c_void_p), C.c_size_t(2), buf) == E_ARG
        assert lib().bp_points_compress(2, two.ctypes.data_as(C.c_void_p), C.c_size_t(1), buf) == E_ARG
        with pytest.raises(Exception):
            E.points_compress(curve, off.reshape(1, 8))
    finally:
        eng.close()


@CURVES
@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("like", [False, True], ids=["plain", "new_like"])
def test_deferred_commit_then_materialize_equals_commit(E, oracle, curve, m, like):
    O = oracle
    V = some_points(O, curve, m) if m else np.zeros((0, 8), dtype=np.uint64)
    blob = CW.wire(O, curve, V)

    def handle():
        t = E.HostTranscript(b"deferred commit")
        if not like:
            return t, E.VerifierCS(curve, t), None
        src = E.VerifierCS(curve, E.HostTranscript(b"deferred commit"))
        src.commit_compressed(blob, defer=True)          # new_like on a handle with pending commitments: the new one starts with none
        v = E.VerifierCS(curve, t, like=src)
        return t, v, src

    ta, a, _ = handle()
    va = a.commit(V)
    tb, b, src = handle()
    before = E.transcript_state(tb)
    vb = b.commit_compressed(blob, defer=True)
    assert E.transcript_state(tb) == before, "a deferred commit touched the transcript"
    assert vb == va
    assert b.materialize(None) == OK
    assert b.materialize(None) == OK                      # nothing pending
    assert E.transcript_state(tb) == E.transcript_state(ta)
    assert b.metrics()[2] == a.metrics()[2] == m
    assert b.commit(V[:1]) == a.commit(V[:1])             # the next variable follows
    if src is not None:
        assert src.metrics()[2] == 0 and src.materialize(None) == OK and src.metrics()[2] == m


@CURVES
def test_transcript_touched_while_pending(E, oracle, curve):
    O = oracle
    F = GD.Field(O, curve)
    eng = E.Engine.host_only(curve, CW.GENS)
    try:
        (proof, V), = CW.prove_items(O, curve, F, 1, 2, False)
        v = CW.verifier(E, O, curve, F, V, False, blob=CW.wire(O, curve, V))
        t = v.transcript()
        state = E.transcript_state(t)
        t.append_message(b"extra", b"bound behind our back")
        assert v.materialize(None) == E_ARG
        assert v.materialize(eng) == E_ARG
        assert E.batch_verify_cs(eng, [v], [proof], None) == E_ARG
        with pytest.raises(Exception, match="instance 0"):
            v.commit_compressed(CW.wire(O, curve, V[:1]), defer=True)      # a second deferred call after the transcript changed
        # nothing was consumed and the bytes are still pending: with the transcript back in place the verification goes through
        from ark_bulletproofs_amd._lib import lib
        assert lib().bp_transcript_import_state(t.h, state) == OK
        assert v.metrics()[2] == 0
        assert E.batch_verify_cs(eng, [v], [proof], None) == OK
        assert v.metrics()[2] == 2
    finally:
        eng.close()


@CURVES
def test_commit_while_pending_and_second_deferred_call(E, oracle, curve):
    O = oracle
    V = some_points(O, curve, 3)
    ta = E.HostTranscript(b"pending")
    a = E.VerifierCS(curve, ta)
    va = a.commit(V)
    tb = E.HostTranscript(b"pending")
    b = E.VerifierCS(curve, tb)
    v1 = b.commit_compressed(CW.wire(O, curve, V[:1]), defer=True)
    with pytest.raises(Exception):
        b.commit(V[1:2])                                  # bp_verifier_commit while pending
    eng = E.Engine.host_only(curve, 0)
    try:
        rc, _, _ = eng.verifier_commit_compressed_batch([b], [CW.wire(O, curve, V[1:2])], defer=False, want_status=True)
        assert rc == E_ARG                                # the immediate form likewise
        # recording calls are allowed while commitments are pending, on the pending variables too
        F = GD.Field(O, curve)
        b.constrain([(v1[0], F.w(1)), (GD.ONE, F.w(5))])
        a.constrain([(va[0], F.w(1)), (GD.ONE, F.w(5))])
        v2 = b.commit_compressed(CW.wire(O, curve, V[1:]), defer=True)     # unchanged transcript: appends in order
        assert v1 + v2 == va
        assert b.materialize(eng) == OK
        assert E.transcript_state(tb) == E.transcript_state(ta) and b.metrics() == a.metrics()
        assert eng.commit_wire_stats() == (0, 0, 3)
    finally:
        eng.close()


@CURVES
def test_host_only_batch_verify_stages_the_same_bytes(E, oracle, curve):
    """9 like-instances (the lockstep replay takes 8, one is left): the dry run's check point — the checksum of everything the
    host staged — is the same for affine commits and for deferred wire commits"""
    O = oracle
    F = GD.Field(O, curve)
    m, count = 3, 9
    items = CW.prove_items(O, curve, F, 3, m, False)
    pf = [items[k % 3][0] for k in range(count)]
    Vs = [items[k % 3][1] for k in range(count)]
    alphas = O.fe_rand(O.fid(curve, True), bytes([4]) * 32, count)
    eng = E.Engine.host_only(curve, CW.GENS)
    try:
        rc_a, pt_a = E.batch_verify_cs(eng, CW.verifiers(E, O, curve, F, Vs, False, wired=False), pf, alphas, want_point=True)
        assert eng.commit_wire_stats() == (0, 0, 0)
        rc_w, pt_w = E.batch_verify_cs(eng, CW.verifiers(E, O, curve, F, Vs, False, wired=True), pf, alphas, want_point=True)
        assert rc_a == OK and rc_w == OK and int(pt_a[1]) == count
        assert (pt_a == pt_w).all()
        assert eng.commit_wire_stats() == (0, 0, count * m)
        # one rejected encoding: the call is that instance's FormatError, whatever the proofs say
        bad = bytearray(CW.wire(O, curve, Vs[4])); bad[33 + 32] = 0xC0
        blobs = [None] * count; blobs[4] = bytes(bad)
        pf_bad = list(pf); pf_bad[2] = pf[2][:-1]         # (a truncated proof earlier in the batch: the commitment error comes first)
        assert E.batch_verify_cs(eng, CW.verifiers(E, O, curve, F, Vs, False, wired=True, blobs=blobs), pf_bad, alphas) == E_FORMAT
    finally:
        eng.close()


@CURVES
def test_immediate_batch_with_one_bad_encoding(E, oracle, curve):
    from ark_bulletproofs_amd._lib import lib

    O = oracle
    V = some_points(O, curve, 6)
    eng = E.Engine.host_only(curve, 0)
    try:
        ts = [E.HostTranscript(b"immediate") for _ in range(3)]
        vs = [E.VerifierCS(curve, t) for t in ts]
        before = E.transcript_state(ts[1])
        blobs = [CW.wire(O, curve, V[:2]), bytearray(CW.wire(O, curve, V[2:5])), CW.wire(O, curve, V[5:])]
        blobs[1][33 + 32] |= 0x01
        rc, st, vars_ = eng.verifier_commit_compressed_batch(vs, blobs, defer=False, want_status=True)
        assert rc == E_FORMAT and list(st) == [OK, E_FORMAT, OK]
        assert [v.metrics()[2] for v in vs] == [2, 0, 1]
        assert E.transcript_state(ts[1]) == before
        assert [len(x) for x in vars_] == [2, 3, 1]
        ref = E.VerifierCS(curve, E.HostTranscript(b"immediate"))
        assert ref.commit(V[:2]) == vars_[0]
        assert E.transcript_state(ts[0]) == E.transcript_state(ref.transcript())
        # up-front checks change nothing: a handle twice, a prover handle, the other curve's verifier, NULL bytes
        hs = (C.c_void_p * 2)(vs[1].h, vs[1].h)
        ms = (C.c_size_t * 2)(1, 1)
        assert lib().bp_verifier_commit_compressed_batch(eng.ctx, C.c_size_t(2), hs, ms, bytes(blobs[0]), 1, None, None) == E_ARG
        p = E.ProverCS(curve, E.HostTranscript(b"immediate"))
        other = E.VerifierCS(1 - curve, E.HostTranscript(b"immediate"))
        for h in (p.h, other.h):
            hs = (C.c_void_p * 2)(vs[1].h, h)
            assert lib().bp_verifier_commit_compressed_batch(eng.ctx, C.c_size_t(2), hs, ms, bytes(blobs[0]), 1, None, None) == E_ARG
        hs = (C.c_void_p * 1)(vs[1].h)
        assert lib().bp_verifier_commit_compressed_batch(eng.ctx, C.c_size_t(1), hs, ms, None, 1, None, None) == E_ARG
        assert vs[1].materialize(None) == OK and vs[1].metrics()[2] == 0      # nothing became pending
    finally:
        eng.close()
