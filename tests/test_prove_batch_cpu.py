"""bp_prover_prove_batch's up-front checks (include/arkbp.h "Batch proving") on a host-only ctx: a batch that fails a check returns
BP_E_ARG and consumes no prover; a valid batch returns BP_E_NO_DEVICE there, never BP_OK without proofs."""
import ctypes as C

import pytest

E_ARG, E_NO_DEVICE = -1, -3


@pytest.fixture(params=[0, 1], ids=["secq256k1", "zorro"])
def hostctx(request):
    from ark_bulletproofs_amd._lib import lib

    ctx = C.c_void_p()
    assert lib().bp_debug_ctx_create_hostonly(request.param, C.c_size_t(64), C.byref(ctx)) == 0
    yield request.param, ctx
    lib().bp_ctx_destroy(ctx)


def _prover(curve, transcript=None):
    from ark_bulletproofs_amd import engine as A

    t = transcript or A.HostTranscript(b"batch-check")
    p = A.ProverCS(curve, t)
    p.commit([[3, 0, 0, 0]], [[5, 0, 0, 0]])
    return p, t


def _call(ctx, provers, rngs, stride=1 << 12):
    from ark_bulletproofs_amd._lib import lib

    n = len(provers)
    hs = (C.c_void_p * n)(*[p.h for p in provers])
    out = C.create_string_buffer(max(stride, 1) * n)
    lens = (C.c_size_t * n)()
    st = (C.c_int * n)(*([7] * n))
    rb = b"".join(rngs) if rngs is not None else None
    rc = lib().bp_prover_prove_batch(ctx, C.c_size_t(n), hs, rb, out, C.c_size_t(stride), lens, st, None)
    return rc, list(lens), list(st)


def _live(p):
    from ark_bulletproofs_amd._lib import lib

    return lib().bp_prover_set_rng(p.h, bytes(32)) == 0


def test_prove_batch_up_front_checks_consume_nothing(hostctx):
    curve, ctx = hostctx
    a, _ = _prover(curve)
    b, _ = _prover(curve)
    rng = [bytes([1]) * 32, bytes([2]) * 32]
    # the same prover twice
    assert _call(ctx, [a, a], rng)[0] == E_ARG
    # two provers borrowing one transcript
    c, t = _prover(curve)
    d, _ = _prover(curve, t)
    assert _call(ctx, [c, d], rng)[0] == E_ARG
    # a stride shorter than a proof with lg(64) = 6 rounds (11 * 33 + 3 * 32 + 2 * (8 + 6 * 33) + 2 * 32 = 935 bytes)
    assert _call(ctx, [a, b], rng, stride=934)[0] == E_ARG
    # no rng bytes anywhere
    assert _call(ctx, [a, b], None)[0] == E_ARG
    # the status array is left alone and every prover is still live (nothing was consumed)
    rc, lens, st = _call(ctx, [a, a], rng)
    assert rc == E_ARG and st == [7, 7] and lens == [0, 0]
    assert all(_live(p) for p in (a, b, c, d))
    # a valid batch: no device here, so no proofs — and still nothing consumed
    rc, lens, _ = _call(ctx, [a, b], rng, stride=935)
    assert rc == E_NO_DEVICE and lens == [0, 0]
    assert _live(a) and _live(b)


def test_prover_commit_batch_needs_a_device(hostctx):
    from ark_bulletproofs_amd._lib import lib

    curve, ctx = hostctx
    a, _ = _prover(curve)
    hs = (C.c_void_p * 1)(a.h)
    me = (C.c_size_t * 1)(1)
    v = (C.c_uint64 * 4)(1, 0, 0, 0)
    assert lib().bp_prover_commit_batch(ctx, C.c_size_t(1), hs, me, v, v, None, None) == E_NO_DEVICE
    assert lib().bp_prover_commit_batch(ctx, C.c_size_t(1), hs, me, None, None, None, None) == E_ARG
