"""Front groups of bp_prover_prove_batch (include/arkbp.h "Batch proving", csrc/prove_batch.inc pf_*, csrc/small_batch_front.cuh): the
stages in front of the inner-product argument — witness import, the A / S / T commitments, flatten, t(x), l(x) / r(x) — run for a
whole group in one launch each.  Every proof must be byte-identical to a single prove of the same statement with the same rng bytes
on the same engine (and to the oracle's), every transcript must end where the single path leaves it, and the proofs must verify.
The shapes are the smallest at which each stage can go wrong."""
import threading

import pytest

pytestmark = pytest.mark.gpu
DIRECT_MAX, PROVE_BATCH, FRONT = 12, 13, 14   # BP_TUNE_DIRECT_MAX, BP_TUNE_PROVE_BATCH, BP_TUNE_PROVE_BATCH_FRONT
LABEL = b"GenericGadgetTest"


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(4096)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng256(request):
    """256 generators: a two-phase gadget can outgrow them in its randomized phase"""
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(256)
    yield e
    e.close()


def _seed(tag, j):
    return bytes([tag & 255, j & 255, (j >> 8) & 255]) + bytes(29)


def _stmts(eng, sc, prm, count, tag):
    from ark_bulletproofs_amd.engine import Statement

    return [Statement(eng.curve, sc, prm, _seed(tag, j), eng) for j in range(count)]


def _singles(eng, sc, prm, count, tag):
    return [s.prove(eng)[0] for s in _stmts(eng, sc, prm, count, tag)]


def _check_scenarios(eng, oracle, sc, prm, count, tag, mcap, proofs, at=None):
    """instance `at` (default: the last) against the oracle's prover, and all the proofs through batch_verify once"""
    at = count - 1 if at is None else at
    ref = oracle.r1cs_prove(eng.curve, sc, prm, _seed(tag, at), 4096, m_cap=mcap)
    assert ref.rc == 0 and ref.proof == proofs[at]
    insts = []
    for j, s in enumerate(_stmts(eng, sc, prm, count, tag)):
        cm, pubs, _, _ = s.info(mcap)
        insts.append((sc, prm, proofs[j], cm, pubs))
    assert eng.batch_verify(insts, bytes([5]) * 32)[0] == 0


# (scenario, params, count, m_cap).  k-shuffles: k = 2 has n1 = 0 and n = N = 2 (one round), in groups of 1, 3 and 70 (more than one
# 64-proof host-pool chunk); k = 4 pads 6 to 8; k = 256 has n = 510 of 512: more than one workgroup per proof in t(x), flatten and the
# table sums (per-proof reductions, k_dt_finish).  The range proof is single-phase with n1 = n = N = 64.
SCENARIOS = [
    (0, [2], 1, 16), (0, [2], 3, 16), (0, [2], 70, 16), (0, [4], 3, 16), (0, [256], 3, 520), (1, [64, 12345], 5, 8),
]


@pytest.mark.parametrize("sc,prm,count,mcap", SCENARIOS)
def test_scenarios_byte_identical_through_front_groups(eng, oracle, sc, prm, count, mcap):
    tag = 101 + sc * 5 + prm[0] % 97 + count
    want = _singles(eng, sc, prm, count, tag)
    f0 = eng.prove_batch_front_stats()
    l0, s0, g0 = eng.prove_batch_stats()
    got = eng.prove_batch(_stmts(eng, sc, prm, count, tag))
    f1 = eng.prove_batch_front_stats()
    l1, s1, g1 = eng.prove_batch_stats()
    assert [st for st, _ in got] == [0] * count
    assert [p for _, p in got] == want
    assert f1[0] - f0[0] == count and f1[1] - f0[1] == 1 and f1[2] > f0[2]     # one front group, every instance in it
    assert l1 - l0 == count and s1 == s0 and g1 - g0 == 1
    _check_scenarios(eng, oracle, sc, prm, count, tag, mcap, [p for _, p in got])


def _gadget(eng, F, kind, seed, **kw):
    """a recorded prover (tests/gadgets.py); returns (prover, transcript, V, publics)"""
    from ark_bulletproofs_amd import engine as A

    import gadgets as GD

    vals, blinds = GD.make_witness(F, seed, 3)
    t = A.HostTranscript(LABEL)
    t.append_message(b"dom-sep", b"generic gadget v1")
    p = A.ProverCS(eng.curve, t)
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    publics = []
    GD.random_program(p, F, seed, wit, vars_, publics=publics, **kw)
    if kind == "raise":          # a randomized-phase callback that raises: the thunk returns -100
        def boom(cs):
            raise RuntimeError("callback failure inside a batch")

        p.specify_randomized_constraints(boom)
    return p, t, V, publics


def _oracle_gadget(O, curve, F, seed, gens, rng, **kw):
    import gadgets as GD

    vals, blinds = GD.make_witness(F, seed, 3)
    p = O.ProverCS(curve, LABEL)
    p.transcript().append_message(b"dom-sep", b"generic gadget v1")
    p.start()
    _, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    GD.random_program(p, F, seed, wit, vars_, publics=[], **kw)
    return p.prove(gens, rng)


def _batch_verify_gadgets(eng, F, items):
    """items: (seed, V, publics, proof, random_program arguments); one batch_verify over recorded verifiers of all of them"""
    import numpy as np

    from ark_bulletproofs_amd import engine as A

    import gadgets as GD

    vs = []
    for seed, V, publics, _, kw in items:
        t = A.HostTranscript(LABEL)
        t.append_message(b"dom-sep", b"generic gadget v1")
        v = A.VerifierCS(eng.curve, t)
        vars_ = v.commit(V)
        GD.random_program(v, F, seed, None, vars_, publics=publics, **kw)
        vs.append(v)
    alphas = np.zeros((len(items), 4), dtype=np.uint64)
    alphas[:, 0] = np.arange(len(items), dtype=np.uint64) * 977 + 3
    alphas[:, 1] = 0x9E3779B97F4A7C15
    return A.batch_verify_cs(eng, vs, [it[3] for it in items], alphas)


def _run_gadgets(eng, oracle, specs, tagbyte):
    """single proves, then one batch of fresh recordings of the same gadgets; returns (want, want_tr, got, made)"""
    from ark_bulletproofs_amd import engine as A

    import gadgets as GD

    F = GD.Field(oracle, eng.curve)
    rngs = [bytes([tagbyte, j]) + bytes(30) for j in range(len(specs))]
    want, want_tr = [], []
    for j, (kind, seed, kw) in enumerate(specs):
        p, t, _, _ = _gadget(eng, F, kind, seed, **kw)
        try:
            want.append((0, p.prove(eng, rngs[j])))
        except A.ArkbpError as e:
            want.append((e.code, b""))
        except RuntimeError:
            want.append((-100, b""))
        want_tr.append(A.transcript_state(t))
    made = [_gadget(eng, F, kind, seed, **kw) for kind, seed, kw in specs]
    rc, got = eng.prove_batch([m[0] for m in made], rng_bytes=rngs, return_rc=True)
    return F, rngs, want, want_tr, rc, got, made


# single phase; both phases non-empty with n1 = 10 of N = 32 (not 0, N / 2 or N)
GADGETS = [
    [("gadget", 31 + j, dict(n_mul=12)) for j in range(3)],
    [("gadget", 41 + j, dict(n_mul=5, two_phase=True, n_mul2=5)) for j in range(3)],
]


@pytest.mark.parametrize("specs", GADGETS, ids=["single_phase", "two_phase"])
def test_recorded_gadgets_through_front_groups(eng, oracle, specs):
    from ark_bulletproofs_amd import engine as A

    f0 = eng.prove_batch_front_stats()
    F, rngs, want, want_tr, rc, got, made = _run_gadgets(eng, oracle, specs, 11)
    f1 = eng.prove_batch_front_stats()
    assert rc == 0 and got == want and all(st == 0 for st, _ in want)
    assert [A.transcript_state(m[1]) for m in made] == want_tr
    assert f1[0] - f0[0] == len(specs) and f1[1] - f0[1] == 1
    kind, seed, kw = specs[-1]
    assert _oracle_gadget(oracle, eng.curve, F, seed, 4096, rngs[-1], **kw) == got[-1][1]
    assert _batch_verify_gadgets(eng, F, [(seed, m[2], m[3], proof, kw) for (kind, seed, kw), m, (_, proof) in zip(specs, made, got)]) == 0


def test_one_front_group_splits_by_padded_size_after_the_randomized_phase(eng, oracle):
    """equal n_mul = 8 (n1 = 13), n_mul2 = 4 and 20: N = 32 and 64 — one group through phase 1, two parts afterwards"""
    from ark_bulletproofs_amd import engine as A

    specs = [("gadget", 51 + j, dict(n_mul=8, two_phase=True, n_mul2=(4 if j % 2 == 0 else 20))) for j in range(4)]
    f0 = eng.prove_batch_front_stats()
    g0 = eng.prove_batch_stats()[2]
    F, rngs, want, want_tr, rc, got, made = _run_gadgets(eng, oracle, specs, 12)
    f1 = eng.prove_batch_front_stats()
    assert rc == 0 and got == want and all(st == 0 for st, _ in want)
    assert len(want[0][1]) != len(want[1][1])                    # different numbers of rounds
    assert [A.transcript_state(m[1]) for m in made] == want_tr
    assert f1[0] - f0[0] == 4 and f1[1] - f0[1] == 2 and eng.prove_batch_stats()[2] - g0 == 2
    for j in (0, 1):
        kind, seed, kw = specs[j]
        assert _oracle_gadget(oracle, eng.curve, F, seed, 4096, rngs[j], **kw) == got[j][1]
    assert _batch_verify_gadgets(eng, F, [(specs[j][1], made[j][2], made[j][3], got[j][1], specs[j][2]) for j in range(4)]) == 0


def test_member_with_phase1_multipliers_leaves_its_group(eng, oracle):
    """n1 = 13 for all; under BP_TUNE_DIRECT_MAX = 32 the one that grows to N = 64 in its randomized phase leaves the front group after
    the phase-1 commitments (in the transcript already) and finishes on the single-proof path: same bytes, same transcript state"""
    from ark_bulletproofs_amd import engine as A

    specs = [("gadget", 55, dict(n_mul=8, two_phase=True, n_mul2=4)), ("gadget", 56, dict(n_mul=8, two_phase=True, n_mul2=20)),
             ("gadget", 57, dict(n_mul=8, two_phase=True, n_mul2=4))]
    eng.set_tuning(DIRECT_MAX, 32)
    try:
        f0, (l0, s0, _) = eng.prove_batch_front_stats(), eng.prove_batch_stats()
        F, rngs, want, want_tr, rc, got, made = _run_gadgets(eng, oracle, specs, 14)
        f1, (l1, s1, _) = eng.prove_batch_front_stats(), eng.prove_batch_stats()
    finally:
        eng.set_tuning(DIRECT_MAX, 8192)
    assert rc == 0 and got == want and all(st == 0 for st, _ in want)
    assert [A.transcript_state(m[1]) for m in made] == want_tr
    assert f1[0] - f0[0] == 2 and f1[1] - f0[1] == 1 and l1 - l0 == 2 and s1 - s0 == 1
    assert _oracle_gadget(oracle, eng.curve, F, 56, 4096, rngs[1], **specs[1][2]) == got[1][1]
    assert _batch_verify_gadgets(eng, F, [(specs[j][1], made[j][2], made[j][3], got[j][1], specs[j][2]) for j in range(3)]) == 0


def test_failing_members_in_the_middle_of_a_front_group(eng256, oracle):
    """a callback that raises and a randomized phase that outgrows the generators, between like gadgets (all n1 = 11)"""
    from ark_bulletproofs_amd import engine as A

    eng = eng256
    ok = dict(n_mul=6, two_phase=True, n_mul2=5)
    specs = [("gadget", 61, ok), ("raise", 62, dict(n_mul=6)), ("gadget", 63, ok), ("gadget", 64, dict(n_mul=6, two_phase=True, n_mul2=300)), ("gadget", 65, ok)]
    f0 = eng.prove_batch_front_stats()
    F, rngs, want, want_tr, rc, got, made = _run_gadgets(eng, oracle, specs, 13)
    f1 = eng.prove_batch_front_stats()
    assert [w[0] for w in want] == [0, -100, 0, -5, 0]
    assert rc == -100 and got == want
    assert [A.transcript_state(m[1]) for m in made] == want_tr
    assert f1[0] - f0[0] == 3 and f1[1] - f0[1] == 1            # the survivors went on as one part
    assert _oracle_gadget(oracle, eng.curve, F, 65, 256, rngs[4], **ok) == got[4][1]
    assert _batch_verify_gadgets(eng, F, [(specs[j][1], made[j][2], made[j][3], got[j][1], ok) for j in (0, 2, 4)]) == 0


def test_group_cap_splits_front_groups(eng, oracle):
    want = _singles(eng, 0, [2], 7, 71)
    eng.set_tuning(PROVE_BATCH, 3)
    try:
        f0, g0 = eng.prove_batch_front_stats(), eng.prove_batch_stats()[2]
        got = eng.prove_batch(_stmts(eng, 0, [2], 7, 71))
        f1, g1 = eng.prove_batch_front_stats(), eng.prove_batch_stats()[2]
    finally:
        eng.set_tuning(PROVE_BATCH, 0)
    assert [p for _, p in got] == want
    assert f1[0] - f0[0] == 7 and f1[1] - f0[1] == 3 and g1 - g0 == 3          # 3 + 3 + 1
    _check_scenarios(eng, oracle, 0, [2], 7, 71, 16, [p for _, p in got], at=3)   # (the first member of the second group)


def test_counters_and_the_knob(eng, oracle):
    want24, want3 = _singles(eng, 0, [16], 24, 81), _singles(eng, 0, [16], 3, 82)
    f0 = eng.prove_batch_front_stats()
    got3 = eng.prove_batch(_stmts(eng, 0, [16], 3, 82))
    f1 = eng.prove_batch_front_stats()
    got24 = eng.prove_batch(_stmts(eng, 0, [16], 24, 81))
    f2 = eng.prove_batch_front_stats()
    assert [p for _, p in got3] == want3 and [p for _, p in got24] == want24
    assert f2[0] - f1[0] == 24 and f2[1] - f1[1] == 1
    assert f1[2] - f0[2] > 0 and f2[2] - f1[2] == f1[2] - f0[2]               # a group's host waits do not depend on its size
    # knob at 0: the stages run one instance at a time, the counters stay put, the bytes are the same
    eng.set_tuning(FRONT, 0)
    try:
        l0 = eng.prove_batch_stats()[0]
        got = eng.prove_batch(_stmts(eng, 0, [16], 24, 81))
        assert eng.prove_batch_front_stats() == f2 and eng.prove_batch_stats()[0] - l0 == 24
    finally:
        eng.set_tuning(FRONT, 1)
    assert [p for _, p in got] == want24
    _check_scenarios(eng, oracle, 0, [16], 24, 81, 40, [p for _, p in got24])
    # a statement above a lowered BP_TUNE_DIRECT_MAX leaves its group after the randomized phase and is proved singly
    w128, w2 = _singles(eng, 0, [128], 1, 83)[0], _singles(eng, 0, [2], 1, 84)[0]
    eng.set_tuning(DIRECT_MAX, 64)
    try:
        s0 = eng.prove_batch_stats()[1]
        got = eng.prove_batch([_stmts(eng, 0, [128], 1, 83)[0], _stmts(eng, 0, [2], 1, 84)[0]])
        f3, s1 = eng.prove_batch_front_stats(), eng.prove_batch_stats()[1]
    finally:
        eng.set_tuning(DIRECT_MAX, 8192)
    assert [p for _, p in got] == [w128, w2]
    _check_scenarios(eng, oracle, 0, [128], 1, 83, 264, [w128])
    assert f3[0] - f2[0] == 1 and f3[1] - f2[1] == 1 and s1 - s0 == 1


def test_two_ctxs_sharing_tables_from_two_threads(eng, oracle):
    import ark_bulletproofs_amd as A

    other = A.Engine(curve=eng.curve)
    try:
        other.share_gens_from(eng)
        want = {t: _singles(eng, 0, [4], 9, t) for t in (91, 92)}
        out = {}

        def run(e, t):
            out[t] = [p for _, p in e.prove_batch(_stmts(e, 0, [4], 9, t))]

        ths = [threading.Thread(target=run, args=(e, t)) for e, t in ((eng, 91), (other, 92))]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert out == want
        assert other.prove_batch_front_stats()[0] == 9
        _check_scenarios(other, oracle, 0, [4], 9, 92, 16, out[92])
    finally:
        other.close()


def test_single_prove_after_a_front_group_equals_a_fresh_ctx(eng, oracle):
    import ark_bulletproofs_amd as A

    f0 = eng.prove_batch_front_stats()[0]
    got = [p for _, p in eng.prove_batch(_stmts(eng, 1, [64, 77], 3, 95) + _stmts(eng, 0, [16], 3, 96))]
    assert eng.prove_batch_front_stats()[0] - f0 == 6
    assert got == _singles(eng, 1, [64, 77], 3, 95) + _singles(eng, 0, [16], 3, 96)
    _check_scenarios(eng, oracle, 1, [64, 77], 3, 95, 8, got[:3])
    _check_scenarios(eng, oracle, 0, [16], 3, 96, 40, got[3:])
    fresh = A.Engine(curve=eng.curve)
    try:
        fresh.gens_derive(4096)
        a = [_stmts(fresh, sc, prm, 1, 97)[0].prove(fresh)[0] for sc, prm in ((0, [16]), (1, [64, 9]))]
    finally:
        fresh.close()
    assert [_stmts(eng, sc, prm, 1, 97)[0].prove(eng)[0] for sc, prm in ((0, [16]), (1, [64, 9]))] == a
