"""Batches of several gadgets (include/arkbp.h "Batches of several gadgets"): the host side.  bp_debug_vfy_class_plan IS the
partition batch verification uses (csrc/r1cs_host.inc vfy_class_plan): classes by key, ordered by size then by first member, the
largest max_classes of at least class_min eligible members become device classes in launch order, the rest is the remainder (-1).
Plus the knob, the counters of a ctx that never took the class path, and the null-argument cases.  No GPU."""
import ctypes as C

import numpy as np
import pytest

OK, E_ARG = 0, -1
TUNE_VFY_CLASS_MIN = 24


def plan(keys, eligible=None, class_min=1, max_classes=0):
    from ark_bulletproofs_amd import engine as E

    return E.debug_vfy_class_plan(keys, eligible, class_min, max_classes)


def test_interleaved_keys_keep_their_classes():
    # A B A C A B: A has 3 members, B 2, C 1
    A, B, Cc = 0xAAAA0000AAAA, 7, 1 << 63
    of, n = plan([A, B, A, Cc, A, B], class_min=1)
    assert n == 3 and of == [0, 1, 0, 2, 0, 1]


def test_order_is_size_then_first_member():
    # sizes: 5 -> 2, 9 -> 3, 4 -> 2, 8 -> 3; ties go to the class whose first member comes first
    keys = [5, 9, 4, 8, 9, 8, 5, 9, 4, 8]
    of, n = plan(keys, class_min=1)
    num = {9: 0, 8: 1, 5: 2, 4: 3}
    assert n == 4 and of == [num[k] for k in keys]
    # the same keys in another arrival order: 8 comes first now, and 4 before 5
    keys = [8, 4, 9, 5, 9, 8, 5, 9, 4, 8]
    of, n = plan(keys, class_min=1)
    num = {8: 0, 9: 1, 4: 2, 5: 3}
    assert n == 4 and of == [num[k] for k in keys]


def test_class_min():
    keys = [1, 2, 1, 3, 1, 2]          # sizes 3, 2, 1
    assert plan(keys, class_min=1) == ([0, 1, 0, 2, 0, 1], 3)
    assert plan(keys, class_min=2) == ([0, 1, 0, -1, 0, 1], 2)
    assert plan(keys, class_min=3) == ([0, -1, 0, -1, 0, -1], 1)
    assert plan(keys, class_min=4) == ([-1] * 6, 0)      # one above the largest class: everything is the remainder
    # 0 is the default, which is far above three members; values above 65535 act as 65535
    assert plan(keys, class_min=0) == ([-1] * 6, 0)
    big = [4] * 65535 + [5] * 3
    for cm in (65535, 65536, 1 << 40):
        of, n = plan(big, class_min=cm)
        assert n == 1 and of[:65535] == [0] * 65535 and of[65535:] == [-1] * 3
    assert plan(big[1:], class_min=1 << 40)[1] == 0


def test_more_classes_than_max():
    from ark_bulletproofs_amd import engine as E

    # ten classes of sizes 10, 9, .., 1, interleaved by construction order; the default takes the eight largest
    keys = []
    for i in range(10):
        keys += [100 + i] * (10 - i)
    rng = np.random.default_rng(5)
    keys = [keys[i] for i in rng.permutation(len(keys))]
    of, n = plan(keys, class_min=1)
    assert n == E.VFY_MAX_CLASSES == 8
    for k, c in zip(keys, of):
        assert c == (k - 100 if k - 100 < 8 else -1)
    of, n = plan(keys, class_min=1, max_classes=3)
    assert n == 3 and all(c == (k - 100 if k - 100 < 3 else -1) for k, c in zip(keys, of))
    of, n = plan(keys, class_min=1, max_classes=64)
    assert n == 10 and all(c == k - 100 for k, c in zip(keys, of))
    # class_min cuts first where it is the tighter bound
    of, n = plan(keys, class_min=8, max_classes=64)
    assert n == 3 and all(c == (k - 100 if k - 100 < 3 else -1) for k, c in zip(keys, of))


def test_ineligible_members_stay_in_the_remainder_and_do_not_count():
    keys = [1, 1, 1, 2, 2, 1, 3]
    elig = [1, 0, 1, 1, 1, 0, 0]
    # class 1 has two eligible members, class 2 two (first member later), class 3 none
    assert plan(keys, elig, class_min=1) == ([0, -1, 0, 1, 1, -1, -1], 2)
    assert plan(keys, elig, class_min=3) == ([-1] * 7, 0)
    assert plan(keys, [0] * 7, class_min=1) == ([-1] * 7, 0)
    # an ineligible first member does not decide the tie: both have two eligible members, class 2's first is 1, class 1's is 2
    assert plan([1, 2, 1, 2, 1], [0, 1, 1, 1, 1], class_min=1) == ([-1, 0, 1, 0, 1], 2)


def test_empty_and_single_class():
    assert plan([], class_min=1) == ([], 0)
    assert plan([42] * 7, class_min=1) == ([0] * 7, 1)
    assert plan([42] * 7, class_min=7) == ([0] * 7, 1)
    assert plan([42] * 7, class_min=8) == ([-1] * 7, 0)
    assert plan([0], class_min=1) == ([0], 1)            # (the key's value means nothing)


def test_null_arguments():
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    keys = (C.c_uint64 * 3)(1, 1, 2)
    of = (C.c_int32 * 3)()
    n = C.c_uint32(77)
    assert L.bp_debug_vfy_class_plan(C.c_size_t(3), keys, None, C.c_uint64(1), C.c_uint32(0), of, C.byref(n)) == OK and n.value == 2 and list(of) == [0, 0, 1]
    assert L.bp_debug_vfy_class_plan(C.c_size_t(3), None, None, C.c_uint64(1), C.c_uint32(0), of, C.byref(n)) == E_ARG
    assert L.bp_debug_vfy_class_plan(C.c_size_t(3), keys, None, C.c_uint64(1), C.c_uint32(0), None, C.byref(n)) == E_ARG
    assert L.bp_debug_vfy_class_plan(C.c_size_t(3), keys, None, C.c_uint64(1), C.c_uint32(0), of, None) == E_ARG
    n.value = 77
    assert L.bp_debug_vfy_class_plan(C.c_size_t(0), None, None, C.c_uint64(1), C.c_uint32(0), None, C.byref(n)) == OK and n.value == 0


@pytest.mark.parametrize("curve", [0, 1])
def test_knob_and_counters_on_a_host_only_ctx(curve):
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    eng = E.Engine.host_only(curve, 0)
    try:
        assert E.TUNE_VFY_CLASS_MIN == TUNE_VFY_CLASS_MIN
        for val in (0, 1, 2, 64, 65535, 65536, 1 << 50):
            assert L.bp_ctx_set_tuning(eng.ctx, TUNE_VFY_CLASS_MIN, C.c_uint64(val)) == OK
        assert L.bp_ctx_set_tuning(eng.ctx, 20, C.c_uint64(1)) == E_ARG
        assert L.bp_ctx_set_tuning(eng.ctx, 23, C.c_uint64(1)) == E_ARG
        assert L.bp_ctx_set_tuning(eng.ctx, 25, C.c_uint64(1)) == E_ARG
        v = [C.c_uint64(9) for _ in range(5)]
        assert L.bp_ctx_vfe_class_stats(eng.ctx, *[C.byref(x) for x in v]) == OK and [x.value for x in v] == [0] * 5
        assert eng.vfe_class_stats() == (0, 0, 0, 0, 0)
        assert L.bp_ctx_vfe_class_stats(eng.ctx, None, None, None, None, None) == OK
        assert L.bp_ctx_vfe_class_stats(None, *[C.byref(x) for x in v]) == E_ARG
    finally:
        eng.close()
