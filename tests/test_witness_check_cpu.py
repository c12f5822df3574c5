"""The witness check without a GPU (include/arkbp.h bp_prover_check, bp_prover_set_check): the host twin — what a NULL or host-only
ctx runs, and what the kernels are compared with in test_gpu_witness_check.py — against Python integers, and the argument checks
of every new entry point."""
import ctypes as C

import numpy as np
import pytest

import gadgets as GD
import wcheck as W


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def L(E):
    from ark_bulletproofs_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def host_engines(E):
    out = {cv: E.Engine.host_only(cv, 64) for cv in (0, 1)}
    yield out
    for e in out.values():
        e.close()


def both(p, host_engines, curve):
    """the report through a NULL ctx and through a host-only ctx: the same"""
    a, b = p.check(), p.check(host_engines[curve])
    assert a == b
    return a


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("two_phase", [False, True])
def test_satisfiable_program_reports_nothing(E, oracle, host_engines, curve, two_phase):
    F = GD.Field(oracle, curve)
    p, m, _, _ = W.random_prover(E, curve, F, 21, 4, two_phase)
    rep = both(p, host_engines, curve)
    assert W.observed(F, rep) == m.expect(deferred=1 if two_phase else 0)
    assert rep.satisfied and rep.first_bad_gate == W.NONE and rep.first_bad_constraint == W.NONE and not rep.first_bad_residual.any()
    nm, nq, _ = p.metrics()
    assert (rep.gates_checked, rep.constraints_checked) == (nm, nq)
    assert rep.deferred_callbacks == (1 if two_phase else 0)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("two_phase", [False, True])
def test_spoiled_variable_names_exactly_pythons_rows(E, oracle, host_engines, curve, two_phase):
    F = GD.Field(oracle, curve)
    for vec, index in ((3, 0), (0, 2), (1, 5), (3, 2)):
        p, m, _, _ = W.random_prover(E, curve, F, 22, 5, two_phase)
        kind = (1, 2, 3, 0)[vec]
        W.poke(E, p, m, vec, index, m.val[(kind, index)] + 1)
        exp = m.expect(deferred=1 if two_phase else 0)
        assert W.observed(F, both(p, host_engines, curve)) == exp
        if vec == 3:
            assert exp[2] == 0 and exp[4] >= 1, "a committed value touches rows only (the program names every committed variable)"
    # a poked a_O: exactly one bad gate
    p, m, _, _ = W.random_prover(E, curve, F, 22, 5, two_phase)
    W.poke(E, p, m, 2, 3, m.val[(3, 3)] + 7)
    rep = both(p, host_engines, curve)
    assert W.observed(F, rep) == m.expect(deferred=1 if two_phase else 0)
    assert (rep.bad_gates, rep.first_bad_gate) == (1, 3)


@pytest.mark.parametrize("curve", [0, 1])
def test_rows_of_special_shape(E, oracle, host_engines, curve):
    F = GD.Field(oracle, curve)
    r1 = F.p - 1

    def fresh():
        p, m, rec, vars_, _ = W.new_prover(E, curve, F, [r1, 5, 0], [1, 2, 3])
        rec.allocate_multiplier((F.w(r1), F.w(r1)))
        return p, m, rec, vars_

    # no terms: satisfied
    p, m, rec, v = fresh()
    rec.constrain([])
    assert W.observed(F, both(p, host_engines, curve)) == m.expect() and m.expect()[4] == 0
    # only One with a non-zero coefficient: violated, the residual is the coefficient
    rec.constrain([(GD.ONE, F.w(9))])
    rep = both(p, host_engines, curve)
    assert W.observed(F, rep) == m.expect()
    assert (rep.bad_constraints, rep.first_bad_constraint, F.i(rep.first_bad_residual)) == (1, 1, 9)
    # only committed variables (v0 = r - 1: a term with coefficient r - 1 is +1, one with coefficient 1 is -1; v2 = 0)
    p, m, rec, v = fresh()
    rec.constrain([(v[0], F.w(r1)), (v[0], F.w(1)), (v[0], F.w(1)), (v[1], F.w(0)), (v[2], F.w(77)), (v[0], F.w(r1))])   # 1 - 1 - 1 + 0 + 0 + 1
    assert W.observed(F, both(p, host_engines, curve)) == m.expect() and m.expect()[4] == 0
    W.poke(E, p, m, 3, 2, 1)
    rep = both(p, host_engines, curve)
    assert W.observed(F, rep) == m.expect() and F.i(rep.first_bad_residual) == 77
    # coefficient r - 1 with value r - 1 (a product of 1), against One
    p, m, rec, v = fresh()
    rec.constrain([((1, 0), F.w(r1)), (GD.ONE, F.w(r1))])
    rec.constrain([((2, 0), F.w(r1)), (v[0], F.w(r1)), (GD.ONE, F.w(F.p - 2))])
    assert W.observed(F, both(p, host_engines, curve)) == m.expect() and m.expect()[4] == 0
    rec.constrain([((1, 0), F.w(r1)), (GD.ONE, F.w(1))])
    rep = both(p, host_engines, curve)
    assert W.observed(F, rep) == m.expect() and (rep.first_bad_constraint, F.i(rep.first_bad_residual)) == (2, 2)


def test_piece_length(E):
    assert E.witness_check_piece() >= 2


def test_refused_calls(E, L, oracle, host_engines):
    F = GD.Field(oracle, 0)
    lib = L.lib()
    rep = E._WitnessReportC()
    rep.gates_checked = 12345
    p, m, _, _ = W.random_prover(E, 0, F, 23, 6, False)
    t = E.HostTranscript(b"v")
    v = E.VerifierCS(0, t)
    on = C.c_int(-7)
    # null and verifier handles
    assert lib.bp_prover_check(None, None, C.byref(rep)) == L.BP_E_ARG
    assert lib.bp_prover_check(None, v.h, C.byref(rep)) == L.BP_E_ARG
    assert lib.bp_prover_check(None, p.h, None) == L.BP_E_ARG
    assert lib.bp_prover_set_check(None, 1) == L.BP_E_ARG
    assert lib.bp_prover_set_check(v.h, 1) == L.BP_E_ARG
    assert lib.bp_prover_checking(v.h, C.byref(on)) == L.BP_E_ARG and on.value == -7
    # the wrong curve
    assert lib.bp_prover_check(host_engines[1].ctx, p.h, C.byref(rep)) == L.BP_E_ARG
    hs = (C.c_void_p * 1)(p.h)
    reps = (E._WitnessReportC * 2)()
    reps[0].gates_checked = reps[1].gates_checked = 777
    assert lib.bp_prover_check_batch(host_engines[1].ctx, C.c_size_t(1), hs, reps) == L.BP_E_ARG
    assert lib.bp_prover_check_batch(None, C.c_size_t(1), hs, reps) == L.BP_E_ARG
    # a handle twice
    hs2 = (C.c_void_p * 2)(p.h, p.h)
    assert lib.bp_prover_check_batch(host_engines[0].ctx, C.c_size_t(2), hs2, reps) == L.BP_E_ARG
    # a verifier among the provers
    hs3 = (C.c_void_p * 2)(p.h, v.h)
    assert lib.bp_prover_check_batch(host_engines[0].ctx, C.c_size_t(2), hs3, reps) == L.BP_E_ARG
    # the poke hook: bad vector, bad index, an unreduced value
    one = F.w(1)
    assert lib.bp_debug_prover_poke_witness(p.h, 4, C.c_size_t(0), L.ptr(one)) == L.BP_E_ARG
    assert lib.bp_debug_prover_poke_witness(p.h, 0, C.c_size_t(10 ** 6), L.ptr(one)) == L.BP_E_ARG
    assert lib.bp_debug_prover_poke_witness(p.h, 3, C.c_size_t(3), L.ptr(one)) == L.BP_E_ARG
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    assert lib.bp_debug_prover_poke_witness(p.h, 0, C.c_size_t(0), L.ptr(big)) == L.BP_E_ARG
    assert lib.bp_debug_prover_poke_witness(v.h, 0, C.c_size_t(0), L.ptr(one)) == L.BP_E_ARG
    # a refused call changes nothing: the reports are untouched, the guard is still off, the prover still checks clean
    assert rep.gates_checked == 12345 and reps[0].gates_checked == 777 and reps[1].gates_checked == 777
    assert p.checking() is False
    assert W.observed(F, p.check()) == m.expect()
    # the guard flag reads back; check_batch on a host-only ctx is the twin per prover
    p.set_check(True)
    assert p.checking() is True
    p.set_check(False)
    assert p.checking() is False
    p2, m2, _, _ = W.random_prover(E, 0, F, 24, 7, True)
    W.poke(E, p2, m2, 0, 1, 99)
    got = host_engines[0].check_batch([p, p2])
    assert [W.observed(F, r) for r in got] == [m.expect(), m2.expect(deferred=1)]
    assert host_engines[0].last_unsatisfied() == []


def test_statement_handles_check_too(E, host_engines):
    """a scenario Statement through bp_stmt_as_prover: satisfiable square chain, then its unsatisfiable variant (the public output
    is one off, so the last constraint fails)"""
    s = E.Statement(0, 3, [6, 0], bytes([1]) * 32)
    rep = s.check()
    assert rep.satisfied and (rep.gates_checked, rep.constraints_checked) == (6, 13)
    s.set_check(True)
    assert s.checking() is True
    bad = E.Statement(0, 3, [6, 1], bytes([1]) * 32)
    rep = bad.check(host_engines[0])
    assert (rep.bad_gates, rep.bad_constraints, rep.first_bad_constraint) == (0, 1, 12)
    assert int(rep.first_bad_residual.any()) == 1
