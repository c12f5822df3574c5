"""A like-prover's witness from device memory (include/arkbp.h bp_prover_assign_multipliers_dev, bp_witness_range_bits_dev,
bp_ctx_witness_dev_stats; csrc/witness_dev.cuh k_wit_take, k_r1cs_import_gate, k_wit_range_bits): a like-prover assigned from
device buffers proves to the bytes of the same like-prover assigned from host vectors holding the same words, and leaves its
transcript in the same state — on the resident route (single-phase, bp_prover_prove) and on every route that takes the witness to the
host first; a word at or above r is refused with the vector and the index named and nothing changed; the handle's copy outlives the
ctx that assigned it; the range gadget's witness builder writes exactly the bits.  Gadgets: tests/likecommon.py."""
import ctypes as C

import numpy as np
import pytest

import gadgets as GD
import likecommon as LC

pytestmark = pytest.mark.gpu
GENS = 512
TUNE_DIRECT_MAX = 12   # include/arkbp.h BP_TUNE_DIRECT_MAX
E_ARG, E_UNSATISFIED = -1, -8


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def engines(E):
    """per curve: the default engine, and one that proves nothing over the direct tables (BP_TUNE_DIRECT_MAX = 0: the folding route)"""
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


_RECS = {}


def recs(E, oracle, curve, spec, same_witness=False):
    """(field, source, witness holder) of a spec, recorded once per module: the source is only ever frozen, the holder only read
    (what it committed, and its multiplier inputs as ark words) — neither is proved, so every test may share them"""
    key = (curve, spec, same_witness)
    if key not in _RECS:
        F = GD.Field(oracle, curve)
        _RECS[key] = (F, LC.record(E, curve, F, spec, 11), LC.record(E, curve, F, spec, 11 if same_witness else 23))
    return _RECS[key]


def host_like(E, src, tw, left=None, right=None):
    return LC.like(E, src, tw, left=left, right=right)


def dev_like(E, eng, src, tw, left=None, right=None):
    """the same like-prover with its witness assigned from device buffers of eng, which are freed at once: the handle reads its own copy"""
    lk = LC.like(E, src, tw, assign=False)
    l, r = tw.left if left is None else left, tw.right if right is None else right
    bl, br = eng.upload_scalars(l), eng.upload_scalars(r)
    try:
        lk.p.assign_multipliers_dev(eng, bl, br, len(l))
    finally:
        bl.free()
        br.free()
    return lk


def prove(E, eng, r, tag, expanded=False):
    if expanded:
        r.p.set_blinding(E.BLINDING_EXPANDED)
    proof = r.p.prove(eng, LC.rng(tag))
    return proof, E.transcript_state(r.t)


def delta(eng, s0):
    return tuple(a - b for a, b in zip(eng.witness_dev_stats(), s0))


# ---- the resident route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("expanded", [False, True], ids=["transcript", "expanded"])
@pytest.mark.parametrize("dm", [None, 0], ids=["direct", "folding"])
@pytest.mark.parametrize("n", [1, 3, 33, 255, 256, 257])
def test_resident_route_byte_identity(E, engines, oracle, curve, expanded, dm, n):
    eng = engines[(curve, dm)]
    F, src, tw = recs(E, oracle, curve, ("single", n, 40 + n))
    want = prove(E, eng, host_like(E, src, tw), 500 + n, expanded)
    s0, p0 = eng.witness_dev_stats(), eng.prover_like_stats()
    lk = dev_like(E, eng, src, tw)
    assert lk.p.metrics()[0] == n
    got = prove(E, eng, lk, 500 + n, expanded)
    assert got[0] == want[0], "the device-assigned like-prover's proof differs from the host-assigned one's"
    assert got[1] == want[1], "the transcripts end in different states"
    assert delta(eng, s0) == (1, n, 0), "one assignment, every multiplier imported from device memory, nothing downloaded"
    p1 = eng.prover_like_stats()
    assert (p1[3] - p0[3], p1[4] - p0[4]) == (n, 0), "the import kernel's products count as gates on the device"
    if n == 33 and dm is None and not expanded:
        assert LC.verifier(E, curve, F, ("single", n, 40 + n), tw.V).verify(eng, got[0]) == 0


# ---- the routes that take the witness to the host -------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_two_phase_takes_the_witness_to_the_host(E, engines, oracle, curve):
    eng = engines[(curve, None)]
    # (the program's randomized callbacks are shared with the recording and hold the source's witness: the like-prover holds it too)
    F, src, tw = recs(E, oracle, curve, ("program2", 4, 49), same_witness=True)
    assert tw.n1 == 4
    want = prove(E, eng, host_like(E, src, tw), 520)
    s0 = eng.witness_dev_stats()
    assert prove(E, eng, dev_like(E, eng, src, tw), 520) == want
    assert delta(eng, s0) == (1, 0, 4)


@pytest.mark.parametrize("curve", [0, 1])
def test_batch_takes_the_witness_to_the_host(E, engines, oracle, curve):
    eng = engines[(curve, None)]
    n = 3
    F, src, _ = recs(E, oracle, curve, ("single", n, 51))
    twins = [LC.record(E, curve, F, ("single", n, 51), 60 + j) for j in range(5)]
    rngs = [LC.rng(530 + j) for j in range(5)]
    want = eng.prove_batch([host_like(E, src, tw).p for tw in twins], rngs)
    assert [st for st, _ in want] == [0] * 5 and len(set(pf for _, pf in want)) == 5
    members = [dev_like(E, eng, src, tw) if j != 2 else host_like(E, src, tw) for j, tw in enumerate(twins)]   # 4 from the device, 1 from the host
    s0 = eng.witness_dev_stats()
    got = eng.prove_batch([r.p for r in members], rngs)
    assert got == want
    assert delta(eng, s0) == (0, 0, 4 * n), "every device member came to the host, at the entry"


@pytest.mark.parametrize("curve", [0, 1])
def test_check_takes_the_witness_to_the_host_and_the_prover_still_proves(E, engines, oracle, curve):
    eng = engines[(curve, None)]
    n = 33
    F, src, tw = recs(E, oracle, curve, ("single", n, 40 + n))
    hl = host_like(E, src, tw)
    want_rep = hl.p.check(eng)
    want = prove(E, eng, hl, 540)
    lk = dev_like(E, eng, src, tw)
    s0 = eng.witness_dev_stats()
    rep = lk.p.check(eng)
    assert rep == want_rep and rep.satisfied and rep.gates_checked == n
    assert delta(eng, s0) == (0, 0, n)
    assert lk.p.check(eng) == want_rep
    assert prove(E, eng, lk, 540) == want
    assert delta(eng, s0) == (0, 0, n), "taken to the host once"


@pytest.mark.parametrize("curve", [0, 1])
def test_wrong_ctx_is_refused_before_anything_is_consumed(E, engines, oracle, curve):
    eng = engines[(curve, None)]
    F, src, tw = recs(E, oracle, curve, ("single", 3, 43))
    lk = dev_like(E, eng, src, tw)
    host = E.Engine.host_only(curve=curve, gens_capacity=GENS)
    try:
        state = E.transcript_state(lk.t)
        with pytest.raises(E.ArkbpError) as ei:
            lk.p.prove(host, LC.rng(545))
        assert ei.value.code == E_ARG and "device" in str(ei.value)
        with pytest.raises(E.ArkbpError) as ei:
            lk.p.check(host)
        assert ei.value.code == E_ARG
        with pytest.raises(E.ArkbpError) as ei:
            lk.p.check()
        assert ei.value.code == E_ARG
        with pytest.raises(E.ArkbpError) as ei:
            host.prove_batch([lk.p], [LC.rng(545)])
        assert ei.value.code == E_ARG
        assert E.transcript_state(lk.t) == state
    finally:
        host.close()
    assert prove(E, eng, lk, 545) == prove(E, eng, host_like(E, src, tw), 545)


# ---- the guard ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_guard(E, engines, oracle, curve):
    from ark_bulletproofs_amd import _lib as L

    eng = engines[(curve, None)]
    n = 33
    F, src, tw = recs(E, oracle, curve, ("single", n, 40 + n))
    plain = prove(E, eng, host_like(E, src, tw), 550)
    lk = dev_like(E, eng, src, tw)
    lk.p.set_check(True)
    s0 = eng.witness_dev_stats()
    assert prove(E, eng, lk, 550) == plain
    assert delta(eng, s0) == (0, n, 0), "the guard reads the resident vectors"
    assert eng.last_unsatisfied() == []
    # a_R of the last multiplier changed (a_O follows it: the gates hold, rows that name it do not)
    right = tw.right.copy()
    right[n - 1] = F.w(F.i(right[n - 1]) + 5)
    reports = []
    for make in (host_like, lambda E_, s, t, right: dev_like(E_, eng, s, t, right=right)):
        bad = make(E, src, tw, right=right)
        bad.p.set_check(True)
        buf = C.create_string_buffer(b"\xAA" * 4096, 4096)
        plen = C.c_size_t(4096)
        assert L.lib().bp_prover_prove(eng.ctx, bad.p.h, LC.rng(551), buf, C.byref(plen), None) == E_UNSATISFIED
        assert buf.raw == b"\xAA" * 4096, "no proof bytes are written"
        reports.append(eng.last_unsatisfied())
    assert reports[0] == reports[1] and len(reports[0]) == 1
    assert reports[0][0][1].bad_gates == 0 and reports[0][0][1].bad_constraints >= 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_words(x):
    """a 256-bit integer as four 64-bit words, as it is (no reduction, no Montgomery form)"""
    return np.array([(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


@pytest.mark.parametrize("curve", [0, 1])
def test_words_at_or_above_r_are_refused(E, engines, oracle, curve):
    from ark_bulletproofs_amd import _lib as L

    eng = engines[(curve, None)]
    n = 257
    F, src, tw = recs(E, oracle, curve, ("single", n, 40 + n))
    lk = LC.like(E, src, tw, assign=False)
    s0 = eng.witness_dev_stats()

    def refused(left, right, names):
        bl, br = eng.upload_scalars(left), eng.upload_scalars(right)
        try:
            with pytest.raises(E.ArkbpError) as ei:
                lk.p.assign_multipliers_dev(eng, bl, br, n)
            assert ei.value.code == E_ARG and names in str(ei.value), str(ei.value)
            assert (bl.download(nbytes=n * 32).reshape(n, 4) == left).all() and (br.download(nbytes=n * 32).reshape(n, 4) == right).all(), "the caller's buffers are unchanged"
        finally:
            bl.free()
            br.free()

    for word in (F.p, F.p + 1, (1 << 256) - 1):
        left = tw.left.copy()
        left[0] = raw_words(word)
        refused(left, tw.right, "left[0]")
        right = tw.right.copy()
        right[256] = raw_words(word)
        refused(tw.left, right, "right[256]")
        refused(left, right, "left[0]")          # both at once: the smallest index
    left = tw.left.copy()
    left[200], left[256] = raw_words(F.p), raw_words(F.p)
    refused(left, tw.right, "left[200]")         # two lanes of one vector, in different workgroups: the smallest index
    # the largest reduced word passes; the handle is unchanged by all of the above and takes a valid witness now
    assert delta(eng, s0) == (0, 0, 0)
    other = engines[(1 - curve, None)]
    bl, br = other.upload_scalars(tw.left), other.upload_scalars(tw.right)
    try:
        with pytest.raises(E.ArkbpError) as ei:
            lk.p.assign_multipliers_dev(other, bl, br, n)      # a ctx of the other curve
        assert ei.value.code == E_ARG
    finally:
        bl.free()
        br.free()
    left = tw.left.copy()
    left[0] = raw_words(F.p - 1)                 # (as ark words: some reduced scalar — the same in both provers)
    bl, br = eng.upload_scalars(left), eng.upload_scalars(tw.right)
    try:
        lk.p.assign_multipliers_dev(eng, bl, br, n)
        with pytest.raises(E.ArkbpError) as ei:
            lk.p.assign_multipliers_dev(eng, bl, br, n)        # a second assignment
        assert ei.value.code == E_ARG
        with pytest.raises(E.ArkbpError) as ei:
            lk.p.assign_multipliers(left, tw.right)
        assert ei.value.code == E_ARG
    finally:
        bl.free()
        br.free()
    assert delta(eng, s0) == (1, 0, 0)
    assert prove(E, eng, lk, 560) == prove(E, eng, host_like(E, src, tw, left=left), 560)
    # after a refusal the host form succeeds as well
    lk2 = LC.like(E, src, tw, assign=False)
    bad = tw.left.copy()
    bad[0] = raw_words(F.p)
    bl, br = eng.upload_scalars(bad), eng.upload_scalars(tw.right)
    try:
        assert L.lib().bp_prover_assign_multipliers_dev(lk2.p.h, eng.ctx, bl.ptr, br.ptr, C.c_size_t(n)) == E_ARG
    finally:
        bl.free()
        br.free()
    lk2.p.assign_multipliers(tw.left, tw.right)
    assert prove(E, eng, lk2, 561) == prove(E, eng, host_like(E, src, tw), 561)


# ---- count == 0, lifetime -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_count_zero(E, engines, oracle, curve):
    eng = engines[(curve, None)]
    F, src, tw = recs(E, oracle, curve, ("shuffle", 2))
    assert tw.n1 == 0
    want = prove(E, eng, host_like(E, src, tw), 570)
    lk = LC.like(E, src, tw, assign=False)
    s0 = eng.witness_dev_stats()
    lk.p.assign_multipliers_dev(eng, None, None, 0)
    assert prove(E, eng, lk, 570) == want
    assert delta(eng, s0) == (1, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_the_copy_outlives_the_assigning_ctx(E, engines, oracle, curve):
    engB = engines[(curve, None)]
    n = 33
    F, src, tw = recs(E, oracle, curve, ("single", n, 40 + n))
    want = prove(E, engB, host_like(E, src, tw), 580)
    engA = E.Engine(curve=curve, device=0)          # shares nothing with engB, holds no generators: it only assigns
    try:
        lk = dev_like(E, engA, src, tw)
        assert engA.witness_dev_stats() == (1, 0, 0)
    finally:
        engA.close()
    s0 = engB.witness_dev_stats()
    assert prove(E, engB, lk, 580) == want
    assert delta(engB, s0) == (0, n, 0)
    # a device witness that is never proved goes with its handle
    engA = E.Engine(curve=curve, device=0)
    try:
        lk = dev_like(E, engA, src, tw)
    finally:
        engA.close()
    lk.p.free()


# ---- the range gadget's witness builder -----------------------------------------------------------------------------------------------
VALUES = [0, 1, 1 << 63, (1 << 64) - 1, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x8000000000000001, 0x5555555555555555]
PATTERN = 0xA5


def expected_bits(F, values, nbits):
    w = np.array([F.w(0), F.w(1)], dtype=np.uint64).reshape(2, 4)
    bits = np.array([(v >> i) & 1 for v in values for i in range(nbits)], dtype=np.int64)
    return w[1 - bits], w[bits]


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("calls", [[(1, 1)], [(3, 64)], [(5, 13)], [(4, 64), (1, 1)], [(257, 1)]], ids=["1x1", "3x64", "5x13", "4x64+1x1", "257x1"])
def test_range_bits_builder(E, engines, oracle, curve, calls):
    """each call writes behind the previous one into the same two buffers ([(4, 64), (1, 1)]: 256 elements and a 257th); eight bytes
    past the last element stay as they were"""
    from ark_bulletproofs_amd import _lib as L

    eng = engines[(curve, None)]
    F = GD.Field(oracle, curve)
    total = sum(c * b for c, b in calls)
    fill = np.full(total * 32 + 8, PATTERN, dtype=np.uint8)
    left, right = eng.alloc(total * 32 + 8).upload(fill), eng.alloc(total * 32 + 8).upload(fill)
    want_l, want_r, at, k = [], [], 0, 0
    try:
        for count, nbits in calls:
            vals = [VALUES[(k + j) % len(VALUES)] for j in range(count)]
            k += count
            d_v = eng.alloc(count * 8).upload(np.array(vals, dtype=np.uint64))
            try:
                rc = L.lib().bp_witness_range_bits_dev(eng.ctx, d_v.ptr, C.c_size_t(count), C.c_uint(nbits), C.c_void_p(left.ptr.value + at * 32), C.c_void_p(right.ptr.value + at * 32))
                assert rc == 0, L.lib().bp_last_error()
            finally:
                d_v.free()
            wl, wr = expected_bits(F, vals, nbits)
            want_l.append(wl)
            want_r.append(wr)
            at += count * nbits
        got_l, got_r = left.download(dtype=np.uint8), right.download(dtype=np.uint8)
    finally:
        left.free()
        right.free()
    for got, want in ((got_l, np.concatenate(want_l)), (got_r, np.concatenate(want_r))):
        assert (got[total * 32:] == PATTERN).all(), "eight bytes past the output are unchanged"
        assert (got[: total * 32].view(np.uint64).reshape(total, 4) == want).all()


# ---- end to end: a range statement whose witness never exists on the host --------------------------------------------------------------
NBITS = 8


def range_gadget(cs, F, var, value, nbits):
    """the reference's range gadget (tests/r1cs_secq256k1.rs:361-445) on any recorder; value None: the verifier's side"""
    lc = [(var, F.w(1))]
    for i in range(nbits):
        if value is None:
            a, b, o = cs.allocate_multiplier()
        else:
            bit = (value >> i) & 1
            a, b, o = cs.allocate_multiplier((F.w(1 - bit), F.w(bit)))
        cs.constrain([(o, F.w(1))])
        cs.constrain([(a, F.w(1)), (b, F.w(1)), (GD.ONE, F.w(F.p - 1))])
        lc.append((b, F.w(F.p - (1 << i))))
    cs.constrain(lc)


def range_prover(E, curve, F, values):
    r = LC.Rec()
    r.t = LC.transcript(E)
    r.p = E.ProverCS(curve, r.t)
    r.v, r.b = [F.w(v) for v in values], [F.w(900 + 7 * j) for j in range(len(values))]
    r.V, vars_ = r.p.commit(r.v, r.b)
    for var, v in zip(vars_, values):
        range_gadget(r.p, F, var, v, NBITS)
    r.spec = ("range", len(values))
    return r


@pytest.mark.parametrize("curve", [0, 1])
def test_range_statement_end_to_end(E, engines, oracle, curve):
    eng = engines[(curve, None)]
    F = GD.Field(oracle, curve)
    values = [0, 0xA7, 0xFF]
    src = range_prover(E, curve, F, [1, 2, 3])
    tw = range_prover(E, curve, F, values)
    assert tw.p.metrics() == (3 * NBITS, 3 * (2 * NBITS + 1), 3)
    want = prove(E, eng, tw, 590)

    def committed_only(vals):
        r = LC.Rec()
        r.v, r.b = [F.w(v) for v in vals], tw.b
        return r

    def from_builder(vals):
        lk = LC.like(E, src, committed_only(vals), assign=False)
        left, right = eng.witness_range_bits(vals, NBITS)
        try:
            lk.p.assign_multipliers_dev(eng, left, right, len(vals) * NBITS)
        finally:
            left.free()
            right.free()
        return lk

    s0 = eng.witness_dev_stats()
    lk = from_builder(values)
    got = prove(E, eng, lk, 590)
    assert got == want
    assert delta(eng, s0) == (1, 3 * NBITS, 0)
    v = E.VerifierCS(curve, LC.transcript(E))
    for var in v.commit(tw.V):
        range_gadget(v, F, var, None, NBITS)
    assert v.verify(eng, got[0]) == 0
    # one value out of range: only its low bits are decomposed, the sum row fails, the guard refuses
    lk = from_builder([0, 1 << NBITS, 0xFF])
    lk.p.set_check(True)
    from ark_bulletproofs_amd import _lib as L

    with pytest.raises(L.UnsatisfiedError) as ei:
        lk.p.prove(eng, LC.rng(591))
    assert ei.value.code == E_UNSATISFIED
    (inst, rep), = eng.last_unsatisfied()
    assert inst == 0 and rep.bad_gates == 0 and (rep.bad_constraints, rep.first_bad_constraint) == (1, 2 * (2 * NBITS + 1) - 1)
