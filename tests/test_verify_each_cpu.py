"""bp_verifier_verify_batch / bp_r1cs_verify_each_scenarios without a GPU (include/arkbp.h "Verification of many proofs with a verdict
for EACH"): the up-front checks on a host-only ctx — every BP_E_ARG case consumes nothing, BP_E_GENS_LENGTH without generators,
BP_E_NO_DEVICE after the checks, count == 0 — and the digit / layout functions of k_ve_tail (csrc/vfy_each.cuh, reached through the
host-only hook bp_debug_ve_plan) against Python integers."""
import ctypes as C
import random

import numpy as np
import pytest

OK, E_ARG, E_NO_DEVICE, E_GENS_LENGTH = 0, -1, -3, -5
TUNE_VERIFY_EACH = 15
CURVES = pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])


def _verifier(E, curve, label=b"verify-each cpu"):
    v = E.VerifierCS(curve, E.HostTranscript(label))
    v.commit(E.pedersen_gens(curve)[0].reshape(1, 8))
    return v


def _call(lib, ctx, hs, n, proofs=b"\0" * 64, lens=None, status=True):
    arr = (C.c_void_p * max(len(hs), 1))(*hs) if hs is not None else None
    ln = (C.c_size_t * max(n, 1))(*([32] * max(n, 1))) if lens is None else lens
    st = (C.c_int * max(n, 1))(*([7] * max(n, 1)))
    rc = lib.bp_verifier_verify_batch(ctx, C.c_size_t(n), arr, proofs, ln, st if status else None, None, None)
    return rc, list(st)


@CURVES
def test_upfront_checks_consume_nothing(curve):
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    eng = E.Engine.host_only(curve, 64)
    try:
        a, b = _verifier(E, curve), _verifier(E, curve)
        hs = [a.h, b.h]
        assert L.bp_verifier_verify_batch(None, C.c_size_t(2), (C.c_void_p * 2)(*hs), b"\0" * 64, (C.c_size_t * 2)(32, 32), (C.c_int * 2)(), None, None) == E_ARG
        # a NULL array
        assert _call(L, eng.ctx, None, 2)[0] == E_ARG
        assert _call(L, eng.ctx, hs, 2, proofs=None)[0] == E_ARG
        assert L.bp_verifier_verify_batch(eng.ctx, C.c_size_t(2), (C.c_void_p * 2)(*hs), b"\0" * 64, None, (C.c_int * 2)(), None, None) == E_ARG
        assert _call(L, eng.ctx, hs, 2, status=False)[0] == E_ARG
        assert _call(L, eng.ctx, [a.h, None], 2)[0] == E_ARG
        # a consumed verifier (Verifier::verify takes self: the dry run of a host-only ctx consumes like the real one)
        used = _verifier(E, curve)
        used.verify(eng, b"\0" * 32)
        assert _call(L, eng.ctx, [a.h, used.h], 2)[0] == E_ARG
        # a prover handle
        p = E.ProverCS(curve, E.HostTranscript(b"verify-each cpu"))
        assert _call(L, eng.ctx, [p.h, b.h], 2)[0] == E_ARG
        # the wrong curve
        other = _verifier(E, 1 - curve)
        assert _call(L, eng.ctx, [a.h, other.h], 2)[0] == E_ARG
        # the same handle twice
        assert _call(L, eng.ctx, [a.h, b.h, a.h], 3)[0] == E_ARG
        # ... and after every refusal the handles are still live: the checks pass, a host-only ctx stops AFTER them — twice, since
        # BP_E_NO_DEVICE consumes nothing either — and the recorders still record
        for _ in range(2):
            rc, st = _call(L, eng.ctx, hs, 2)
            assert rc == E_NO_DEVICE and st == [7, 7]
        for v in (a, b, other):
            v.commit(E.pedersen_gens(v.curve)[1].reshape(1, 8))
            assert L.bp_cs_metrics(v.h, None, None, None) == OK
        p.commit([np.zeros(4, dtype=np.uint64)], [np.zeros(4, dtype=np.uint64)])
        # count == 0 is the empty loop
        assert _call(L, eng.ctx, None, 0, proofs=None, status=False)[0] == OK
        # the counters of a ctx that never verified; the knob
        g, s, n, w = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
        assert L.bp_ctx_verify_each_stats(eng.ctx, C.byref(g), C.byref(s), C.byref(n), C.byref(w)) == OK
        assert (g.value, s.value, n.value, w.value) == (0, 0, 0, 0)
        assert eng.verify_each_stats() == (0, 0, 0, 0)
        assert L.bp_ctx_verify_each_stats(None, None, None, None, None) == E_ARG
        for val in (0, 3, 4096, 1 << 20):
            assert L.bp_ctx_set_tuning(eng.ctx, TUNE_VERIFY_EACH, C.c_uint64(val)) == OK
    finally:
        eng.close()


@CURVES
def test_no_generators_is_gens_length(curve):
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    eng = E.Engine.host_only(curve, 0)
    try:
        a = _verifier(E, curve)
        rc, st = _call(L, eng.ctx, [a.h], 1)
        assert rc == E_GENS_LENGTH and st == [7]
        eng2 = E.Engine.host_only(curve, 64)
        try:
            assert _call(L, eng2.ctx, [a.h], 1)[0] == E_NO_DEVICE      # (not consumed by the refusal)
        finally:
            eng2.close()
    finally:
        eng.close()


@CURVES
def test_scenario_entry_checks(curve):
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    eng = E.Engine.host_only(curve, 64)
    try:
        pk = E.PackedInstances([(0, [2], b"\0" * 40, np.zeros((4, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))])
        st = (C.c_int * 1)(7)
        args = [eng.ctx, C.c_size_t(1), pk.scen, pk.prm.ctypes.data_as(C.c_void_p), pk.proofs, pk.plens, pk.cms.ctypes.data_as(C.c_void_p), pk.ms,
                pk.pubs.ctypes.data_as(C.c_void_p), pk.npubs, st, None, None]
        assert L.bp_r1cs_verify_each_scenarios(*args) == E_NO_DEVICE and st[0] == 7
        for hole in (2, 3, 4, 5, 6, 7, 9, 10):
            bad = list(args)
            bad[hole] = None
            assert L.bp_r1cs_verify_each_scenarios(*bad) == E_ARG, hole
        assert L.bp_r1cs_verify_each_scenarios(None, *args[1:]) == E_ARG
        assert L.bp_r1cs_verify_each_scenarios(eng.ctx, C.c_size_t(0), None, None, None, None, None, None, None, None, None, None, None) == OK
        assert eng.verify_each_scenarios([]) == (0, [])
    finally:
        eng.close()


# ---- k_ve_tail's digit and layout functions ------------------------------------------------------------------------------------
def _words(x):
    return [(x >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def test_digits_planes_and_layout_against_python_integers():
    from ark_bulletproofs_amd import engine as E

    rnd = random.Random(20250)
    top = 1 << 252
    special = [0, 1, (1 << 256) - 1, top, 15 << 252, 1 << 255, 0x8421 << 100, sum(1 << (4 * w) for w in range(64)), sum(8 << (4 * w) for w in range(64))]
    lengths = [0, 1, 2, 25, 64, 300, 0, 3]
    offsets = [5]                                    # (a first offset that is not zero: ranges are relative to it)
    for n in lengths:
        offsets.append(offsets[-1] + n)
    total = offsets[-1] - offsets[0]
    ks = [special[i] if i < len(special) else rnd.getrandbits(256) for i in range(total)]
    sc = np.array([_words(k) for k in ks], dtype=np.uint64)
    at = 0
    for job, n in enumerate(lengths):
        first, terms, dg, pl, lanes, groups = E.debug_ve_plan(offsets, sc, job)
        assert (first, terms) == (at, n), "job %d owns terms [%d, %d)" % (job, at, at + n)
        for t in range(n):
            k = ks[at + t]
            assert [int(d) for d in dg[t]] == [(k >> (4 * w)) & 15 for w in range(64)], "digits of term %d of job %d" % (t, job)
            # the bit planes rebuild the scalar: sum over windows and planes of bit * 2^(4 w + b)
            assert sum(((int(pl[t][w]) >> b) & 1) << (4 * w + b) for w in range(64) for b in range(4)) == k
            assert (pl[t] == dg[t]).all()
        # quad w = lanes 4w .. 4w + 3; window w folds into group w // 4, whose LDS slot follows the 64 window slots
        assert [int(x) for x in lanes] == [4 * w for w in range(64)]
        assert [int(x) for x in groups] == [64 + w // 4 for w in range(64)]
        at += n
    # the Horner order of the two passes gives sum_w 16^w * window[w]: checked on integers with the slots the hook reports
    win = [rnd.getrandbits(40) for _ in range(64)]
    gsum = {}
    for g in sorted(set(int(x) for x in groups)):
        ws = [w for w in range(64) if int(groups[w]) == g]
        acc = 0
        for w in reversed(ws):
            acc = acc * 16 + win[w]
        gsum[g] = acc
    acc = 0
    for g in sorted(gsum, reverse=True):
        acc = acc * 16 ** 4 + gsum[g]
    assert acc == sum(16 ** w * win[w] for w in range(64))


def test_plan_hook_rejects_bad_arguments():
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    off = (C.c_size_t * 3)(0, 2, 1)
    f, t = C.c_uint32(0), C.c_uint32(0)
    assert L.bp_debug_ve_plan(C.c_size_t(2), off, None, C.c_size_t(0), C.byref(f), C.byref(t), None, None, None, None) == E_ARG      # offsets decrease
    off = (C.c_size_t * 3)(0, 2, 4)
    assert L.bp_debug_ve_plan(C.c_size_t(2), off, None, C.c_size_t(2), C.byref(f), C.byref(t), None, None, None, None) == E_ARG      # no such job
    assert L.bp_debug_ve_plan(C.c_size_t(2), None, None, C.c_size_t(0), C.byref(f), C.byref(t), None, None, None, None) == E_ARG
    assert L.bp_debug_ve_plan(C.c_size_t(2), off, None, C.c_size_t(1), C.byref(f), C.byref(t), None, None, None, None) == OK and (f.value, t.value) == (2, 2)
