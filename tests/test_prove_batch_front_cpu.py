"""BP_TUNE_PROVE_BATCH_FRONT and bp_ctx_prove_batch_front_stats (include/arkbp.h "Batch proving") on a host-only ctx: the knob is
accepted like the other knobs, and a ctx that never proved a batch reports zeros."""
import ctypes as C

import pytest

E_ARG = -1
FRONT = 14   # BP_TUNE_PROVE_BATCH_FRONT


@pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])
def test_front_knob_and_stats_on_a_host_only_ctx(curve):
    from ark_bulletproofs_amd._lib import lib

    ctx = C.c_void_p()
    assert lib().bp_debug_ctx_create_hostonly(curve, C.c_size_t(64), C.byref(ctx)) == 0
    try:
        assert lib().bp_ctx_set_tuning(ctx, FRONT, C.c_uint64(0)) == 0
        assert lib().bp_ctx_set_tuning(ctx, FRONT, C.c_uint64(1)) == 0
        assert lib().bp_ctx_set_tuning(ctx, FRONT, C.c_uint64(2)) == E_ARG
        a, g, w = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        assert lib().bp_ctx_prove_batch_front_stats(ctx, C.byref(a), C.byref(g), C.byref(w)) == 0
        assert (a.value, g.value, w.value) == (0, 0, 0)
        assert lib().bp_ctx_prove_batch_front_stats(ctx, None, None, None) == 0
        assert lib().bp_ctx_prove_batch_front_stats(None, C.byref(a), C.byref(g), C.byref(w)) == E_ARG
    finally:
        lib().bp_ctx_destroy(ctx)
