"""The two-phase sponge schedule (csrc/vfe_sched.hpp build_verifier_schedule_2phase) without a GPU: a statement with randomized
constraints appends "dom-sep" / "r1cs-2phase" after S1 and then draws one challenge_scalar per gadget challenge before A_I2
(src/r1cs/verifier.rs:353-376, 403-420).  The callbacks append nothing, so the plan is still a function of the shape plus the
ordered gadget labels.  Run by its CPU interpreter it must produce the challenge_bytes outputs of a live merlin transcript, here
through the product's host transcript AND through the independent Python STROBE model of tests/pystrobe.py; the gadget
challenges come out after r (y z u x w u_1..u_k r g_1..g_G)."""
import numpy as np
import pytest

from ark_bulletproofs_amd import engine as E

import pystrobe


def live_replay_2phase(tr_append, tr_challenge, m, k, n, items, absorb, labels):
    """verify_prepare_t (r1cs_host.inc) with the randomized phase between S1 and A_I2, message for message, on a live transcript;
    returns the challenges in the schedule's index order"""
    it = iter(items)

    def pt(label):
        tr_append(label, bytes(next(it)[:65]))

    if absorb:
        for _ in range(m):
            pt(b"V")
    rest = list(it)
    pts, scal = rest[: 11 + 2 * k], rest[11 + 2 * k:]
    it = iter(pts)
    out = []
    tr_append(b"m", int(m).to_bytes(8, "little"))
    pt(b"A_I1"), pt(b"A_O1"), pt(b"S1")
    tr_append(b"dom-sep", b"r1cs-2phase")
    gadget = [tr_challenge(l) for l in labels]
    pt(b"A_I2"), pt(b"A_O2"), pt(b"S2")
    out.append(tr_challenge(b"y")), out.append(tr_challenge(b"z"))
    pt(b"T_1"), pt(b"T_3"), pt(b"T_4"), pt(b"T_5"), pt(b"T_6")
    out.append(tr_challenge(b"u")), out.append(tr_challenge(b"x"))
    for label, s in zip((b"t_x", b"t_x_blinding", b"e_blinding"), scal):
        tr_append(label, bytes(s[:32]))
    out.append(tr_challenge(b"w"))
    tr_append(b"dom-sep", b"ipp v1")
    tr_append(b"n", int(n).to_bytes(8, "little"))
    L, R = pts[11: 11 + k], pts[11 + k:]
    for i in range(k):
        tr_append(b"L", bytes(L[i][:65])), tr_append(b"R", bytes(R[i][:65]))
        out.append(tr_challenge(b"u"))
    out.append(tr_challenge(b"r"))
    return out + gadget


LABELS = {
    1: [b"shuffle challenge"],
    2: [b"z", b"a much longer gadget challenge label that takes a good part of the rate block by itself" * 2],
    3: [b"c0", b"second challenge", b"x" * 170],
}


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("m,k,absorb,prefix", [(0, 0, 1, 0), (2, 1, 1, 3), (4, 3, 0, 17), (6, 2, 1, 160), (33, 5, 0, 165), (128, 11, 1, 77)])
def test_two_phase_schedule_equals_live_transcript(G, m, k, absorb, prefix):
    labels = LABELS[G]
    rng = np.random.default_rng(100000 * G + 1000 * m + 10 * k + absorb)
    nitems = (m if absorb else 0) + 11 + 2 * k + 3
    items = rng.integers(0, 256, size=(nitems, 72), dtype=np.uint8)
    n = 1 << k
    label = b"vfe two-phase schedule test"
    t = E.HostTranscript(label)
    junk = bytes(rng.integers(0, 256, size=prefix, dtype=np.uint8))
    t.append_message(b"prefix", junk)          # moves the starting position around the rate block
    state = E.transcript_state(t)
    seeds, nblocks = E.vfe_schedule_replay_2phase(state, absorb, m, k, n, labels, items)
    assert seeds.shape == (6 + k + G, 32)
    exp = live_replay_2phase(lambda l, msg: t.append_message(l, msg), lambda l: bytes(t.challenge_bytes(l, 32)), m, k, n, items, absorb, labels)
    assert [bytes(s) for s in seeds] == exp
    if m <= 33:
        pt = pystrobe.Transcript(label)
        pt.append_message(b"prefix", junk)
        exp2 = live_replay_2phase(lambda l, msg: pt.append_message(l, msg), lambda l: bytes(pt.challenge_bytes(l, 32)), m, k, n, items, absorb, labels)
        assert exp2 == exp
    assert nblocks >= 6 + k + G


def test_two_phase_schedule_differs_from_single_phase():
    """the same proof items under the single-phase schedule give other protocol challenges (the separator differs, and the gadget
    squeezes move the sponge)"""
    rng = np.random.default_rng(7)
    m, k = 2, 2
    items = rng.integers(0, 256, size=(m + 11 + 2 * k + 3, 72), dtype=np.uint8)
    state = E.transcript_state(E.HostTranscript(b"x"))
    s1, _ = E.vfe_schedule_replay(state, 1, m, k, 1 << k, items)
    s2, _ = E.vfe_schedule_replay_2phase(state, 1, m, k, 1 << k, [b"shuffle challenge"], items)
    assert not any(bytes(a) == bytes(b) for a, b in zip(s1, s2[: 6 + k]))


def test_two_phase_schedule_rejects_bad_arguments():
    from ark_bulletproofs_amd import _lib
    import ctypes as C

    L = _lib.lib()
    st = bytearray(203)
    st[200] = 200   # a position outside the rate
    buf = (C.c_uint8 * 72)()
    out = (C.c_uint8 * 2048)()
    labels = (C.c_char_p * 1)(b"z")
    assert L.bp_debug_vfe_schedule_replay_2phase(bytes(st), 0, C.c_uint64(0), C.c_uint32(0), C.c_uint64(1), labels, C.c_size_t(1), buf, out, None) == _lib.BP_E_ARG
    assert L.bp_debug_vfe_schedule_replay_2phase(bytes(203), 0, C.c_uint64(0), C.c_uint32(32), C.c_uint64(1), labels, C.c_size_t(1), buf, out, None) == _lib.BP_E_ARG
    assert L.bp_debug_vfe_schedule_replay_2phase(bytes(203), 0, C.c_uint64(0), C.c_uint32(0), C.c_uint64(1), None, C.c_size_t(1), buf, out, None) == _lib.BP_E_ARG
