"""The witness check on the GPU (csrc/witness_check.cuh; include/arkbp.h bp_prover_check, bp_prover_set_check):
(a) device report == host twin == Python integers on the smallest shapes where the kernels can go wrong;
(b) the guard on the single-proof routes: same bytes for a satisfiable statement, BP_E_UNSATISFIED for the reference's own failure
    case (a shuffle whose output is no permutation of its input: only phase-2 constraints are violated);
(c) the guard in bp_prover_prove_batch with and without front groups; (d) bp_prover_check_batch == the single calls."""
import pytest

import gadgets as GD
import wcheck as W

pytestmark = pytest.mark.gpu
GENS = 256
TUNE_DIRECT_MAX, TUNE_PROVE_BATCH_FRONT = 12, 14   # include/arkbp.h BP_TUNE_DIRECT_MAX, BP_TUNE_PROVE_BATCH_FRONT


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def engines(E):
    out = {}
    for cv in (0, 1):
        e = E.Engine(curve=cv, device=0)
        e.gens_derive(GENS)
        out[cv] = e
    yield out
    for e in out.values():
        e.close()


def three(F, p, m, eng, deferred=0):
    """device report == host twin == Python"""
    dev, host, exp = p.check(eng), p.check(), m.expect(deferred)
    assert W.observed(F, host) == exp, "host twin differs from Python"
    assert W.observed(F, dev) == exp, "device report differs from Python"
    assert dev == host
    return dev


def gates_prover(E, curve, F, n):
    """n multipliers with random inputs; rows: v0 - c0, then one per gate (c * a_O[i] - c * l_i * r_i), then c1 - v1"""
    import random

    rs = random.Random(1000 + n)
    vals = [rs.randrange(F.p), rs.randrange(F.p)]
    p, m, rec, v, _ = W.new_prover(E, curve, F, vals, [3, 4])
    rec.constrain([(v[0], F.w(1)), (GD.ONE, F.w(F.p - vals[0]))])
    for i in range(n):
        a, b, c = rs.randrange(F.p), rs.randrange(F.p), rs.randrange(1, F.p)
        _, _, o = rec.allocate_multiplier((F.w(a), F.w(b)))
        rec.constrain([(o, F.w(c)), (GD.ONE, F.w((-c * a * b) % F.p))])
    rec.constrain([(v[1], F.w(F.p - 1)), (GD.ONE, F.w(vals[1]))])
    return p, m


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gates_and_rows_at_the_block_edges(E, engines, oracle, curve, n):
    F, eng = GD.Field(oracle, curve), engines[curve]
    p, m = gates_prover(E, curve, F, n)
    rep = three(F, p, m, eng)
    assert rep.satisfied and (rep.gates_checked, rep.constraints_checked) == (n, n + 2)
    # gate n - 1 (its row with it), then gate 0 as well: the count and the minimum
    W.poke(E, p, m, 2, n - 1, m.val[(3, n - 1)] + 1)
    rep = three(F, p, m, eng)
    assert (rep.bad_gates, rep.first_bad_gate, rep.bad_constraints, rep.first_bad_constraint) == (1, n - 1, 1, n)
    W.poke(E, p, m, 0, 0, m.val[(1, 0)] + 1)
    rep = three(F, p, m, eng)
    assert (rep.bad_gates, rep.first_bad_gate) == ((2, 0) if n > 1 else (1, 0))
    # rows alone: the last row, then row 0 too
    p, m = gates_prover(E, curve, F, n)
    W.poke(E, p, m, 3, 1, m.val[(0, 1)] + 5)
    rep = three(F, p, m, eng)
    assert (rep.bad_gates, rep.bad_constraints, rep.first_bad_constraint, F.i(rep.first_bad_residual)) == (0, 1, n + 1, F.p - 5)
    W.poke(E, p, m, 3, 0, m.val[(0, 0)] + 1)
    rep = three(F, p, m, eng)
    assert (rep.bad_constraints, rep.first_bad_constraint, F.i(rep.first_bad_residual)) == (2, 0, 1)
    # several bad rows and gates at once
    if n >= 255:
        p, m = gates_prover(E, curve, F, n)
        for i in (7, 100, 200, n - 2):
            W.poke(E, p, m, 2, i, m.val[(3, i)] + 3)
        rep = three(F, p, m, eng)
        assert (rep.bad_gates, rep.first_bad_gate, rep.bad_constraints, rep.first_bad_constraint) == (4, 7, 4, 8)


def long_row(F, rec, v, T, off_by_one):
    """a row of exactly T terms: T - 1 terms with coefficient r - 1 on variables whose value is r - 1 (a product of 1 each: committed
    v0, a_L and a_R of the four multipliers in turn), closed by One with coefficient r - (T - 1) — or that plus one"""
    r1 = F.p - 1
    pool = [v[0]] + [(k, i) for i in range(4) for k in (1, 2)]
    lc = [(pool[j % len(pool)], F.w(r1)) for j in range(T - 1)]
    lc.append((GD.ONE, F.w((F.p - (T - 1) + (1 if off_by_one else 0)) % F.p)))
    rec.constrain(lc)


@pytest.mark.parametrize("curve", [0, 1])
def test_long_rows_are_cut_into_pieces(E, engines, oracle, curve):
    F, eng = GD.Field(oracle, curve), engines[curve]
    P = E.witness_check_piece()
    r1 = F.p - 1

    def fresh():
        p, m, rec, v, _ = W.new_prover(E, curve, F, [r1, 0], [1, 2])
        for _ in range(4):
            rec.allocate_multiplier((F.w(r1), F.w(r1)))
        return p, m, rec, v

    for T in (P, P + 1, 3 * P + 5):
        p, m, rec, v = fresh()
        long_row(F, rec, v, T, False)
        assert len(m.rows[0]) == T
        assert three(F, p, m, eng).satisfied
        p, m, rec, v = fresh()
        long_row(F, rec, v, T, True)
        rep = three(F, p, m, eng)
        assert (rep.bad_gates, rep.bad_constraints, rep.first_bad_constraint, F.i(rep.first_bad_residual)) == (0, 1, 0, 1)
    # one long row among one-term rows (v1 = 0 satisfies c * v1 for every c), satisfied; then the long row fails; then one-term rows do
    for bad_long in (False, True):
        p, m, rec, v = fresh()
        for j in range(5):
            rec.constrain([(v[1], F.w(40 + j))])
        long_row(F, rec, v, 2 * P + 1, bad_long)
        for j in range(300):
            rec.constrain([(v[1], F.w(r1 if j % 2 else 7 + j))])
        rep = three(F, p, m, eng)
        assert (rep.bad_constraints, rep.first_bad_constraint) == ((1, 5) if bad_long else (0, W.NONE))
        W.poke(E, p, m, 3, 1, 1)
        rep = three(F, p, m, eng)
        assert (rep.bad_constraints, rep.first_bad_constraint, F.i(rep.first_bad_residual)) == (306 if bad_long else 305, 0, 40)
    # two long rows of different lengths, the second one violated
    p, m, rec, v = fresh()
    long_row(F, rec, v, P + 3, False)
    rec.constrain([(v[1], F.w(3))])
    long_row(F, rec, v, 5 * P, True)
    rep = three(F, p, m, eng)
    assert (rep.bad_constraints, rep.first_bad_constraint) == (1, 2)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("two_phase", [False, True])
def test_random_programs_agree(E, engines, oracle, curve, two_phase):
    F, eng = GD.Field(oracle, curve), engines[curve]
    d = 1 if two_phase else 0
    p, m, _, _ = W.random_prover(E, curve, F, 31, 8, two_phase)
    assert three(F, p, m, eng, d).satisfied
    W.poke(E, p, m, 3, 1, m.val[(0, 1)] + 1)
    W.poke(E, p, m, 1, 4, m.val[(2, 4)] + 1)
    rep = three(F, p, m, eng, d)
    assert rep.bad_gates == 1 and rep.bad_constraints >= 1


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("route", ["direct", "folding", "expanded", "precomputed"])
@pytest.mark.parametrize("two_phase", [False, True])
def test_guard_leaves_a_satisfiable_proof_unchanged(E, oracle, curve, route, two_phase):
    F = GD.Field(oracle, curve)
    eng = E.Engine(curve=curve, device=0)
    try:
        eng.gens_derive(GENS)
        if route == "folding":
            eng.set_tuning(TUNE_DIRECT_MAX, 0)
        proofs = []
        for guard in (False, True):
            p, m, V, pubs = W.random_prover(E, curve, F, 41, 9, two_phase)
            if route == "expanded":
                p.set_blinding(E.BLINDING_EXPANDED)
            if guard:
                p.set_check(True)
            rng = bytes([9]) * 32
            if route == "precomputed":
                p.precompute(rng)
            assert p.check(eng).satisfied            # check does not consume: the prover still proves
            proofs.append(p.prove(eng, rng))
            assert eng.last_unsatisfied() == []
            # a consumed prover is refused by every entry point of the check
            with pytest.raises(E.ArkbpError):
                p.check(eng)
            with pytest.raises(E.ArkbpError):
                p.set_check(True)
            with pytest.raises(E.ArkbpError):
                eng.check_batch([p])
        assert proofs[0] == proofs[1] and len(proofs[0]) > 0
    finally:
        eng.close()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [2, 8])
def test_guard_refuses_the_shuffle_that_is_no_permutation(E, engines, oracle, curve, k):
    from ark_bulletproofs_amd import UnsatisfiedError, _lib

    F, eng = GD.Field(oracle, curve), engines[curve]
    # today's behaviour, pinned: without the guard the prover returns BP_OK and a proof that the verifier rejects
    p, m, V = W.shuffle_prover(E, curve, F, k, permuted=False)
    rep = three(F, p, m, eng, 1)
    assert rep.satisfied and rep.constraints_checked == 0, "phase 1 of a shuffle has no constraint: the report covers nothing yet"
    proof = p.prove(eng, bytes([3]) * 32)
    assert len(proof) > 0
    assert W.shuffle_verifier(E, curve, F, k, V).verify(eng, proof) == _lib.BP_E_VERIFICATION
    # with the guard: BP_E_UNSATISFIED, and the report names the phase-2 constraint Python finds
    p, m, V = W.shuffle_prover(E, curve, F, k, permuted=False)
    p.set_check(True)
    with pytest.raises(UnsatisfiedError) as ei:
        p.prove(eng, bytes([3]) * 32)
    assert ei.value.code == _lib.BP_E_UNSATISFIED == -8
    (inst, rep), = eng.last_unsatisfied()
    exp = m.expect(0)       # the callback has run: the model holds the phase-2 rows
    assert inst == 0 and W.observed(F, rep) == exp
    assert exp[4] == 1 and exp[5] == 4 * (k - 1) == len(m.rows) - 1 and exp[2] == 0
    # the raw call writes no proof bytes
    p, m, V = W.shuffle_prover(E, curve, F, k, permuted=False)
    p.set_check(True)
    import ctypes as C

    buf = C.create_string_buffer(b"\xAA" * 4096, 4096)
    plen = C.c_size_t(4096)
    assert _lib.lib().bp_prover_prove(eng.ctx, p.h, bytes([3]) * 32, buf, C.byref(plen), None) == -8
    assert buf.raw == b"\xAA" * 4096
    # a permutation proves with the guard on, and the verifier accepts; the list of refused instances is empty again
    p, m, V = W.shuffle_prover(E, curve, F, k, permuted=True)
    p.set_check(True)
    proof = p.prove(eng, bytes([3]) * 32)
    assert eng.last_unsatisfied() == []
    assert W.shuffle_verifier(E, curve, F, k, V).verify(eng, proof) == 0


SHAPES = [   # (random_program arguments, two_phase, padded size)
    (dict(n_mul=1, n_alloc=0, n_extra=2), False, 2),
    (dict(n_mul=1, n_alloc=0, n_extra=2), False, 2),
    (dict(n_mul=6, n_alloc=1, n_extra=2, n_mul2=5), True, 16),
    (dict(n_mul=10, n_alloc=3, n_extra=6), False, 16),
    (dict(n_mul=40, n_alloc=3, n_extra=6), False, 64),
]


def five(E, curve, F, spoiled=(), guarded=(), expanded=False):
    out = []
    for j, (kw, two, _) in enumerate(SHAPES):
        p, m, V, pubs = W.random_prover(E, curve, F, 50 + j, 60 + j, two, **kw)
        if expanded:
            p.set_blinding(E.BLINDING_EXPANDED)
        if j in spoiled:
            W.poke(E, p, m, 0, 0, m.val[(1, 0)] + 1)
        if j in guarded:
            p.set_check(True)
        out.append((p, m))
    return out


def padded(n):
    N = 1
    while N < n:
        N *= 2
    return N


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("front", [1, 0])
@pytest.mark.parametrize("expanded", [False, True])
def test_guard_in_prove_batch(E, oracle, curve, front, expanded):
    F = GD.Field(oracle, curve)
    eng = E.Engine(curve=curve, device=0)
    try:
        eng.gens_derive(GENS)
        eng.set_tuning(TUNE_PROVE_BATCH_FRONT, front)
        rngs = [bytes([20 + j]) * 32 for j in range(5)]
        # the reference run: the same five statements, unspoiled, unguarded — its front waits, and its proofs one at a time
        ref = five(E, curve, F, expanded=expanded)
        w0 = eng.prove_batch_front_stats()[2]
        rc, res = eng.prove_batch([p for p, _ in ref], rngs, return_rc=True)
        waits_ref = eng.prove_batch_front_stats()[2] - w0
        assert rc == 0 and [s for s, _ in res] == [0] * 5
        assert [padded(m.n) for _, m in ref] == [s[2] for s in SHAPES]
        single = [p.prove(eng, rngs[j]) for j, (p, _) in enumerate(five(E, curve, F, expanded=expanded))]
        assert [b for _, b in res] == single
        # members 0 and 3 spoiled, all guarded
        run = five(E, curve, F, spoiled=(0, 3), guarded=range(5), expanded=expanded)
        w0 = eng.prove_batch_front_stats()[2]
        rc, res = eng.prove_batch([p for p, _ in run], rngs, return_rc=True)
        waits = eng.prove_batch_front_stats()[2] - w0
        assert [s for s, _ in res] == [-8, 0, 0, -8, 0] and rc == -8
        assert [len(b) for _, b in res][0] == 0 and len(res[3][1]) == 0
        assert [res[j][1] for j in (1, 2, 4)] == [single[j] for j in (1, 2, 4)]
        last = eng.last_unsatisfied()
        assert [i for i, _ in last] == [0, 3]
        for i, rep in last:
            assert W.observed(F, rep) == run[i][1].expect(0)
            assert rep.bad_gates == 1 and rep.first_bad_gate == 0 and rep.first_bad_constraint == 0
        assert waits == waits_ref, "the guard must not add a host wait to the front stages"
        if front == 0:
            assert waits == 0
        else:
            assert waits_ref > 0
        # guarded and unguarded members mixed: only guarded ones are refused (the unguarded spoiled member proves, as it always did)
        run = five(E, curve, F, spoiled=(0, 3), guarded=(1, 3), expanded=expanded)
        rc, res = eng.prove_batch([p for p, _ in run], rngs, return_rc=True)
        assert [s for s, _ in res] == [0, 0, 0, -8, 0] and rc == -8 and len(res[0][1]) > 0
        assert [res[j][1] for j in (1, 2, 4)] == [single[j] for j in (1, 2, 4)]
        assert [i for i, _ in eng.last_unsatisfied()] == [3]
        # a call that refuses none empties the list
        run = five(E, curve, F, guarded=range(5), expanded=expanded)
        rc, res = eng.prove_batch([p for p, _ in run], rngs, return_rc=True)
        assert rc == 0 and [b for _, b in res] == single and eng.last_unsatisfied() == []
    finally:
        eng.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_check_batch_equals_single_checks(E, engines, oracle, curve):
    F, eng = GD.Field(oracle, curve), engines[curve]
    run = five(E, curve, F, spoiled=(0, 3))
    got = eng.check_batch([p for p, _ in run])
    assert got == [p.check(eng) for p, _ in run]
    assert [W.observed(F, r) for r in got] == [m.expect(1 if SHAPES[j][1] else 0) for j, (_, m) in enumerate(run)]
    assert [r.satisfied for r in got] == [False, True, True, False, True]
    # nothing was consumed
    assert all(p.check().gates_checked == m.n for p, m in run)
