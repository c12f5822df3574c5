"""bp_msm_batch / bp_msm_batch_dev without a GPU (include/arkbp.h "VariableBaseMSM::msm"): the up-front checks on a host-only ctx —
every BP_E_ARG case, BP_E_NO_DEVICE after the checks, count == 0, the counters of a fresh ctx, the knobs — and the planner's own
route / slice / digit functions (csrc/msm_batch.cuh, reached through the host-only hook bp_debug_msm_batch_plan) against Python
integers.  The four knobs take every value (0 = the default): a slice cap of 0 is NOT refused, it stands for the default, which
follows from the call's bucketed terms."""
import ctypes as C
import random

import numpy as np
import pytest

import pymodel

OK, E_ARG, E_NO_DEVICE = 0, -1, -3
SHORT, BUCKETED, SINGLE = 0, 1, 2
CURVES = pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])


def _offs(*v):
    return (C.c_size_t * len(v))(*v)


@CURVES
def test_upfront_checks_then_no_device(curve):
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib, ptr

    L = lib()
    eng = E.Engine.host_only(curve, 0)
    try:
        B, S, out = np.zeros((4, 8), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64), np.full((3, 8), 7, dtype=np.uint64)
        good = _offs(0, 1, 3)
        for fn, b, s in ((L.bp_msm_batch, ptr(B), ptr(S)), (L.bp_msm_batch_dev, C.c_void_p(64), C.c_void_p(64))):   # (the resident pointers are never read here)
            n2 = C.c_size_t(2)
            assert fn(None, n2, good, b, s, 0, ptr(out)) == E_ARG                       # null ctx
            assert fn(eng.ctx, n2, None, b, s, 0, ptr(out)) == E_ARG                    # null offsets
            assert fn(eng.ctx, n2, good, b, s, 0, None) == E_ARG                        # null out
            assert fn(eng.ctx, n2, _offs(0, 3, 1), b, s, 0, ptr(out)) == E_ARG          # decreasing offsets
            assert fn(eng.ctx, n2, _offs(2, 3, 1), b, s, 1, ptr(out)) == E_ARG
            assert fn(eng.ctx, n2, _offs(0, 5, 1 << 31), b, s, 0, ptr(out)) == E_ARG    # 2^31 terms
            assert fn(eng.ctx, n2, _offs(7, 7, 7 + (1 << 31)), b, s, 0, ptr(out)) == E_ARG
            assert fn(eng.ctx, n2, good, None, s, 0, ptr(out)) == E_ARG                 # null bases / scalars with terms
            assert fn(eng.ctx, n2, good, b, None, 0, ptr(out)) == E_ARG
            assert (out == 7).all(), "a refused call wrote results"
            # the checks pass: a host-only ctx stops after them
            assert fn(eng.ctx, n2, good, b, s, 0, ptr(out)) == E_NO_DEVICE
            assert fn(eng.ctx, n2, _offs(0, 0, 0), None, None, 0, ptr(out)) == E_NO_DEVICE   # no terms: null operands are fine
            assert (out == 7).all()
            # count == 0 is the empty loop, before every check
            assert fn(eng.ctx, C.c_size_t(0), None, None, None, 0, None) == OK
            assert fn(None, C.c_size_t(0), None, None, None, 0, None) == OK
        with pytest.raises(E.ArkbpError) as e:
            eng.msm_batch([(B[:2], S[:2]), (B[:0], S[:0])])
        assert e.value.code == E_NO_DEVICE
        with pytest.raises(ValueError):
            eng.msm_batch([(B[:2], S[:1])])
        assert eng.msm_batch([]).shape == (0, 8)
        # the counters of a ctx that never ran a batch
        v = [C.c_uint64(9) for _ in range(5)]
        assert L.bp_ctx_msm_batch_stats(eng.ctx, *[C.byref(x) for x in v]) == OK and [x.value for x in v] == [0] * 5
        assert eng.msm_batch_stats() == (0, 0, 0, 0, 0)
        assert L.bp_ctx_msm_batch_stats(eng.ctx, None, None, None, None, None) == OK
        assert L.bp_ctx_msm_batch_stats(None, None, None, None, None, None) == E_ARG
        # the knobs: every value is accepted, 0 = the default
        assert (E.TUNE_MSM_BATCH_SHORT, E.TUNE_MSM_BATCH_SLICE, E.TUNE_MSM_BATCH_MAX, E.TUNE_MSM_BATCH_MIN_JOBS) == (16, 17, 18, 19)
        for knob in (16, 17, 18, 19):
            for val in (0, 1, 8, 4096, 1 << 31, (1 << 64) - 1):
                assert L.bp_ctx_set_tuning(eng.ctx, knob, C.c_uint64(val)) == OK
        assert L.bp_ctx_set_tuning(eng.ctx, 20, C.c_uint64(1)) == E_ARG
    finally:
        eng.close()


def _lengths(S, L, M):
    return [0, 1, S, S + 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, M, M + 1]


@pytest.mark.parametrize("knobs", [(4, 8, 40), (0, 0, 0)], ids=["lowered", "defaults"])
def test_routes_and_slices(knobs):
    from ark_bulletproofs_amd import engine as E

    S, L, M = [k or d for k, d in zip(knobs, E.MSM_BATCH_DEFAULTS)]
    if L is None:
        # the default slice cap follows from the call's bucketed terms, and the lengths below from the cap: take the fixed point
        L = next(c for c in range(64, 513) if E.msm_batch_default_slice(sum(n for n in _lengths(S, c, M) if S < n <= M)) == c)
        assert [E.msm_batch_default_slice(t) for t in (0, 1, 64 * 128, 64 * 128 + 1, 16648, 512 * 128, 1 << 31)] == [64, 64, 64, 65, 131, 512, 512]
    assert 0 < S < L - 1 and 2 * L + 1 < M, "the lengths below are meant to be distinct routes"
    lengths = _lengths(S, L, M)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for job, n in enumerate(lengths):
        route, nsl, first, length, _ = E.debug_msm_batch_plan(lengths, None, job, *knobs)
        assert list(route) == [SHORT if m <= S else BUCKETED if m <= M else SINGLE for m in lengths]
        assert list(nsl) == [-(-m // L) for m in lengths]
        # the job's slices: in order, disjoint, exactly its terms, none longer than L, near-equal
        assert len(first) == -(-n // L)
        pos = int(starts[job])
        for f, ln in zip(first, length):
            assert int(f) == pos and 1 <= int(ln) <= L
            pos += int(ln)
        assert pos == int(starts[job]) + n
        if len(length):
            assert int(max(length)) - int(min(length)) <= 1
    # a max at or below the short cap leaves no bucketed route
    route, _, _, _, _ = E.debug_msm_batch_plan([3, 5, 9, 50], None, 0, 8, 4, 8)
    assert list(route) == [SHORT, SHORT, SINGLE, SINGLE]


def test_plan_refusals():
    from ark_bulletproofs_amd._lib import lib

    Lb = lib()
    r8, n32 = (C.c_uint8 * 2)(), (C.c_uint32 * 2)()
    z = C.c_uint64(0)
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(2), None, z, z, z, None, C.c_size_t(0), r8, n32, None, None, None) == E_ARG
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(2), _offs(0, 3, 1), z, z, z, None, C.c_size_t(0), r8, n32, None, None, None) == E_ARG      # offsets decrease
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(2), _offs(0, 1, 1 << 31), z, z, z, None, C.c_size_t(0), r8, n32, None, None, None) == E_ARG
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(2), _offs(0, 1, 3), z, z, z, None, C.c_size_t(2), r8, n32, n32, None, None) == E_ARG       # no such job
    d8 = (C.c_int8 * 128)()
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(2), _offs(0, 1, 3), z, z, z, None, C.c_size_t(1), r8, n32, None, None, d8) == E_ARG        # digits without scalars
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(2), _offs(5, 6, 8), z, z, z, None, C.c_size_t(1), r8, n32, n32, None, None) == OK
    assert list(r8) == [SHORT, SHORT] and n32[0] == 1   # slice_first of job 1 = 1: relative to offsets[0]
    assert Lb.bp_debug_msm_batch_plan(C.c_size_t(0), _offs(0), z, z, z, None, C.c_size_t(0), None, None, None, None, None) == OK


@CURVES
def test_digits_rebuild_the_integer(curve):
    from ark_bulletproofs_amd import engine as E

    r = pymodel.CURVES[curve]["r"]
    rnd = random.Random(1708 + curve)
    special = [0, 1, r - 1, (1 << 256) - 1] + [d << (4 * w) for w in (0, 37, 63) for d in (1, 8, 15)] + \
              [sum(15 << (4 * w) for w in range(64)), sum(8 << (4 * w) for w in range(64))]
    ks = special + [rnd.randrange(1 << 256) for _ in range(20)] + [rnd.randrange(r) for _ in range(20)]
    rnd.shuffle(ks)
    lengths = [3, 0, 17, len(ks) - 20]
    sc = np.array([[(k >> (64 * i)) & ((1 << 64) - 1) for i in range(4)] for k in ks], dtype=np.uint64)
    pos = 0
    for job, n in enumerate(lengths):
        _, _, _, _, dg = E.debug_msm_batch_plan(lengths, sc, job, 4, 8, 40)
        assert dg.shape == (n, 64)
        for t in range(n):
            # unsigned digits: 0 .. 15, no carry window, and sum_w digit[w] 16^w is the integer itself (2^256 - 1 included)
            assert dg[t].min() >= 0 and dg[t].max() <= 15
            assert sum(int(dg[t, w]) << (4 * w) for w in range(64)) == ks[pos + t], "term %d of job %d" % (t, job)
        pos += n
    assert pos == len(ks)
