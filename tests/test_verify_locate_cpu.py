"""bp_r1cs_batch_verify_locate without a GPU (include/arkbp.h "Batch verification that NAMES the failing instances"): the planner
(csrc/verify_locate.inc, reached through the host-only hook bp_debug_locate_plan, which runs it over a simulated core) exhaustively
at small counts — statuses, the bounds on passes and on instances in passes, contiguous ranges of the survivors, no pass whose outcome
was implied — and the ABI on a host-only ctx: every BP_E_ARG case consumes nothing, BP_E_GENS_LENGTH without generators,
BP_E_NO_DEVICE after the checks, count == 0, the leaf knob, the counters of a fresh ctx."""
import ctypes as C

import numpy as np
import pytest

OK, E_ARG, E_NO_DEVICE, E_VERIFICATION, E_GENS_LENGTH, E_FORMAT = 0, -1, -3, -4, -5, -6
PASSED, FAILED_CHECK, FAILED_BEFORE = 0, 1, 2
TUNE_VERIFY_LOCATE_LEAF = 22
CURVES = pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])


class Plan:
    """bp_debug_locate_plan with buffers that are allocated once (the exhaustive sweeps make a quarter of a million calls)"""

    def __init__(self, count):
        from ark_bulletproofs_amd._lib import lib

        self.fn, self.n, cap = lib().bp_debug_locate_plan, count, 2 * count + 2
        self.fc, self.fb = (C.c_uint8 * count)(), (C.c_uint8 * count)()
        self.lo, self.cnt, self.out = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint8 * cap)()
        self.st, self.np_, self.inst = (C.c_int * count)(), C.c_uint32(0), C.c_uint64(0)

    def run(self, mask_check, mask_before):
        n = self.n
        for k in range(n):
            self.fc[k] = (mask_check >> k) & 1
            self.fb[k] = (mask_before >> k) & 1
        assert self.fn(C.c_size_t(n), self.fc, self.fb, C.byref(self.np_), self.lo, self.cnt, self.out, C.byref(self.inst), self.st) == OK
        p = self.np_.value
        assert p <= 2 * n + 2
        return list(self.st), [(self.lo[i], self.cnt[i], self.out[i]) for i in range(p)], self.inst.value


def ceil_log2(n):
    return (n - 1).bit_length()


def check_plan(n, mask_check, mask_before, st, passes, inst):
    """everything the planner promises, from the masks alone"""
    tag = (n, bin(mask_check), bin(mask_before))
    assert st == [E_FORMAT if (mask_before >> k) & 1 else E_VERIFICATION if (mask_check >> k) & 1 else OK for k in range(n)], tag
    surv = list(range(n))            # the instances still in the batch, in instance order
    known_ok = 0                     # bit k: instance k is inside a range that passed
    failed_sets = []                 # the member sets of ranges known to fail their check (tested, or implied)
    total = 0
    drops = 0
    for i, (lo, cnt, outcome) in enumerate(passes):
        assert cnt >= 1 and lo + cnt <= len(surv), (tag, i, "a pass is a contiguous range of the survivors")
        members = surv[lo:lo + cnt]
        S = sum(1 << k for k in members)
        total += cnt
        if i == 0:
            assert (lo, cnt) == (0, n), (tag, "pass 1 covers everything")
        # the simulated core: members that fail before the check are named (and leave), else the check decides
        want = FAILED_BEFORE if S & mask_before else FAILED_CHECK if S & mask_check else PASSED
        assert outcome == want, (tag, i)
        if outcome == FAILED_BEFORE:
            assert i == 0, (tag, "only pass 1 can meet members that fail before their check")
            surv = [k for k in surv if not (mask_before >> k) & 1]
            drops += 1
            continue
        # no pass whose outcome was implied: all members known valid, or a known-failing set whose unknown part lies inside
        assert S & ~known_ok, (tag, i, "every member was already known to be valid")
        for F in failed_sets:
            assert (F & ~known_ok) & ~S, (tag, i, "the range was known to fail: e.g. the upper half after a passing lower half")
        if outcome == PASSED:
            known_ok |= S
        else:
            failed_sets.append(S)
    assert total == inst, tag
    ns = n - bin(mask_before).count("1")
    f = bin(mask_check & ~mask_before).count("1")
    assert drops == (1 if mask_before else 0), tag
    if ns == 0:
        assert len(passes) == 1, tag
    elif f == 0:
        assert len(passes) == 1 + drops, (tag, "a valid batch is one pass")
    else:
        assert len(passes) <= 1 + 2 * f * ceil_log2(ns) + drops, (tag, len(passes))
        if f == 1:
            assert inst - drops * n <= 3 * ns, (tag, inst)


@pytest.mark.parametrize("count", list(range(1, 13)))
def test_planner_every_check_mask(count):
    P = Plan(count)
    for mask in range(1 << count):
        st, passes, inst = P.run(mask, 0)
        check_plan(count, mask, 0, st, passes, inst)
        if mask == 0:
            assert passes == [(0, count, PASSED)] and inst == count


def test_planner_every_pair_of_masks_at_nine():
    P = Plan(9)
    for before in range(1 << 9):
        for mask in range(1 << 9):
            st, passes, inst = P.run(mask, before)
            check_plan(9, mask, before, st, passes, inst)


def test_planner_tests_the_smaller_lower_half_and_skips_the_implied_upper_half():
    """the plan of one bad proof in thirteen, spelled out: 13 -> 6 + 7, lower half first, the upper half never tested after a passing
    lower half.  (With the lower half ceil(n / 2) the first of nine would cost 9 + 5 + 4 + 3 + 2 + 2 + 1 + 1 + 1 = 28 > 3 * 9.)"""
    P = Plan(13)
    st, passes, inst = P.run(1 << 12, 0)          # the last instance: every lower half passes, 12 is implied
    assert passes == [(0, 13, FAILED_CHECK), (0, 6, PASSED), (6, 3, PASSED), (9, 2, PASSED), (11, 1, PASSED)] and inst == 25
    assert st == [OK] * 12 + [E_VERIFICATION]
    st, passes, inst = P.run(1, 0)                # the first instance
    assert passes == [(0, 13, FAILED_CHECK), (0, 6, FAILED_CHECK), (0, 3, FAILED_CHECK), (0, 1, FAILED_CHECK), (1, 2, PASSED), (3, 3, PASSED), (6, 7, PASSED)]
    assert st == [E_VERIFICATION] + [OK] * 12 and inst == 35


def test_plan_hook_arguments():
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib

    L = lib()
    st = (C.c_int * 4)()
    assert L.bp_debug_locate_plan(C.c_size_t(4), None, None, None, None, None, None, None, st) == E_ARG      # no fails_check
    assert L.bp_debug_locate_plan(C.c_size_t(4), (C.c_uint8 * 4)(), None, None, None, None, None, None, None) == E_ARG   # no status
    # every output but the statuses is optional; fails_before may be NULL
    assert L.bp_debug_locate_plan(C.c_size_t(4), (C.c_uint8 * 4)(0, 1, 0, 0), None, None, None, None, None, None, st) == OK
    assert list(st) == [OK, E_VERIFICATION, OK, OK]
    assert E.debug_locate_plan([]) == ([], [], 0)
    st, passes, inst = E.debug_locate_plan([0, 0, 1], [1, 0, 0])
    assert st == [E_FORMAT, OK, E_VERIFICATION] and passes == [(0, 3, FAILED_BEFORE), (0, 2, FAILED_CHECK), (0, 1, PASSED)] and inst == 6


# ---- the ABI on a ctx without a device ---------------------------------------------------------------------------------------------
def _verifier(E, curve, label=b"verify-locate cpu"):
    v = E.VerifierCS(curve, E.HostTranscript(label))
    v.commit(E.pedersen_gens(curve)[0].reshape(1, 8))
    return v


ONES = object()


def _call(lib, ctx, hs, n, proofs=b"\0" * 96, lens=True, status=True, alphas=ONES):
    arr = (C.c_void_p * max(len(hs), 1))(*hs) if hs is not None else None
    ln = (C.c_size_t * max(n, 1))(*([32] * max(n, 1))) if lens else None
    st = (C.c_int * max(n, 1))(*([7] * max(n, 1)))
    if alphas is ONES:
        alphas = np.ones((max(n, 1), 4), dtype=np.uint64)
    al = alphas.ctypes.data_as(C.c_void_p) if alphas is not None else None
    rc = lib.bp_r1cs_batch_verify_locate(ctx, C.c_size_t(n), arr, proofs, ln, al, st if status else None, None)
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
        al2 = np.ones((2, 4), dtype=np.uint64)
        assert L.bp_r1cs_batch_verify_locate(None, C.c_size_t(2), (C.c_void_p * 2)(*hs), b"\0" * 64, (C.c_size_t * 2)(32, 32), al2.ctypes.data_as(C.c_void_p),
                                             (C.c_int * 2)(), None) == E_ARG
        # a NULL array
        assert _call(L, eng.ctx, None, 2)[0] == E_ARG
        assert _call(L, eng.ctx, hs, 2, proofs=None)[0] == E_ARG
        assert _call(L, eng.ctx, hs, 2, lens=False)[0] == E_ARG
        assert _call(L, eng.ctx, hs, 2, status=False)[0] == E_ARG
        assert _call(L, eng.ctx, [a.h, None], 2)[0] == E_ARG
        # the weights: required for more than one instance, none of them zero
        assert _call(L, eng.ctx, hs, 2, alphas=None)[0] == E_ARG
        for z in (0, 1):
            al = np.ones((2, 4), dtype=np.uint64)
            al[z] = 0
            assert _call(L, eng.ctx, hs, 2, alphas=al)[0] == E_ARG
        assert _call(L, eng.ctx, [a.h], 1, alphas=np.zeros((1, 4), dtype=np.uint64))[0] == E_ARG
        with pytest.raises(E.ArkbpError) as e:
            E.batch_verify_locate_cs(eng, [a, b], [b"\0" * 32] * 2, np.zeros((2, 4), dtype=np.uint64))
        assert e.value.code == E_ARG
        with pytest.raises(ValueError):
            E.batch_verify_locate_cs(eng, [a, b], [b"\0" * 32], al2)
        # a consumed verifier (Verifier::verify takes self: the dry run of a host-only ctx consumes like the real one)
        used = _verifier(E, curve)
        used.verify(eng, b"\0" * 32)
        assert _call(L, eng.ctx, [a.h, used.h], 2)[0] == E_ARG
        # a prover handle
        p = E.ProverCS(curve, E.HostTranscript(b"verify-locate cpu"))
        assert _call(L, eng.ctx, [p.h, b.h], 2)[0] == E_ARG
        # the wrong curve
        other = _verifier(E, 1 - curve)
        assert _call(L, eng.ctx, [a.h, other.h], 2)[0] == E_ARG
        # the same handle twice
        assert _call(L, eng.ctx, [a.h, b.h, a.h], 3)[0] == E_ARG
        # a like-instance that holds fewer commitments than the shared constraints name
        v0 = E.VerifierCS(curve, E.HostTranscript(b"verify-locate cpu"))
        pts = E.pedersen_gens(curve)
        x, y = v0.commit(np.stack([pts[0], pts[1]]).reshape(2, 8))
        one = np.array([1, 0, 0, 0], dtype=np.uint64)
        v0.constrain([(x, one), (y, one)])
        short = E.VerifierCS(curve, E.HostTranscript(b"verify-locate cpu"), like=v0)
        short.commit(pts[0].reshape(1, 8))
        assert _call(L, eng.ctx, [v0.h, short.h], 2)[0] == E_ARG
        assert _call(L, eng.ctx, [short.h], 1)[0] == E_ARG
        # ... and after every refusal the handles are still live: the checks pass, a host-only ctx stops AFTER them — twice, since
        # BP_E_NO_DEVICE consumes nothing either — and the recorders still record
        for _ in range(2):
            rc, st = _call(L, eng.ctx, hs, 2)
            assert rc == E_NO_DEVICE and st == [7, 7]
        assert _call(L, eng.ctx, [a.h], 1, alphas=None) == (E_NO_DEVICE, [7])         # one instance: NULL = weight 1
        short.commit(pts[1].reshape(1, 8))                                            # now it holds both
        assert _call(L, eng.ctx, [v0.h, short.h], 2)[0] == E_NO_DEVICE
        for v in (a, b, other):
            v.commit(E.pedersen_gens(v.curve)[1].reshape(1, 8))
            assert L.bp_cs_metrics(v.h, None, None, None) == OK
        p.commit([np.zeros(4, dtype=np.uint64)], [np.zeros(4, dtype=np.uint64)])
        # count == 0 is the empty loop
        assert _call(L, eng.ctx, None, 0, proofs=None, status=False, alphas=None)[0] == OK
        assert E.batch_verify_locate_cs(eng, [], [], None) == (OK, [])
        # the counters of a ctx that never located anything
        v = [C.c_uint64(9) for _ in range(4)]
        assert L.bp_ctx_verify_locate_stats(eng.ctx, *[C.byref(x) for x in v]) == OK and [x.value for x in v] == [0] * 4
        assert eng.verify_locate_stats() == (0, 0, 0, 0)
        assert L.bp_ctx_verify_locate_stats(eng.ctx, None, None, None, None) == OK
        assert L.bp_ctx_verify_locate_stats(None, None, None, None, None) == E_ARG
        # the knob: 22, up to 4096; 20 stays refused
        assert E.TUNE_VERIFY_LOCATE_LEAF == TUNE_VERIFY_LOCATE_LEAF
        for val in (0, 1, 4, 4096):
            assert L.bp_ctx_set_tuning(eng.ctx, TUNE_VERIFY_LOCATE_LEAF, C.c_uint64(val)) == OK
        assert L.bp_ctx_set_tuning(eng.ctx, TUNE_VERIFY_LOCATE_LEAF, C.c_uint64(4097)) == E_ARG
        assert L.bp_ctx_set_tuning(eng.ctx, 20, C.c_uint64(1)) == E_ARG
        assert L.bp_ctx_set_tuning(eng.ctx, 23, C.c_uint64(1)) == E_ARG
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
        inst = (0, [2], b"\0" * 40, np.zeros((4, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
        pk = E.PackedInstances([inst, inst])
        st = (C.c_int * 2)(7, 7)
        args = [eng.ctx, C.c_size_t(2), pk.scen, pk.prm.ctypes.data_as(C.c_void_p), pk.proofs, pk.plens, pk.cms.ctypes.data_as(C.c_void_p), pk.ms,
                pk.pubs.ctypes.data_as(C.c_void_p), pk.npubs, bytes(32), st, None]
        assert L.bp_r1cs_batch_verify_locate_scenarios(*args) == E_NO_DEVICE and list(st) == [7, 7]
        for hole in (2, 3, 4, 5, 6, 7, 9, 10, 11):          # (10: the weights' seed, required for more than one instance)
            bad = list(args)
            bad[hole] = None
            assert L.bp_r1cs_batch_verify_locate_scenarios(*bad) == E_ARG, hole
        assert L.bp_r1cs_batch_verify_locate_scenarios(None, *args[1:]) == E_ARG
        assert L.bp_r1cs_batch_verify_locate_scenarios(eng.ctx, C.c_size_t(0), None, None, None, None, None, None, None, None, None, None, None) == OK
        assert eng.batch_verify_locate([], bytes(32)) == (OK, [])
        with pytest.raises(E.ArkbpError) as e:
            eng.batch_verify_locate([inst, inst], bytes(32))
        assert e.value.code == E_NO_DEVICE
    finally:
        eng.close()
