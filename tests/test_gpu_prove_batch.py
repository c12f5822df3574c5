"""bp_prover_prove_batch (include/arkbp.h "Batch proving", csrc/prove_batch.inc, csrc/small_batch.cuh): many statements in one call,
the inner-product arguments of like-sized small statements in lockstep groups.  Every proof must be byte-identical to a single
bp_prover_prove of the same statement with the same rng bytes (and to the oracle's), verify, and leave the ctx's single-proof path
as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PROVE_BATCH, DIRECT_MAX = 13, 12   # BP_TUNE_PROVE_BATCH, BP_TUNE_DIRECT_MAX


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(4096)
    yield e
    e.close()


def _seed(tag, j):
    return bytes([tag & 255, j & 255, (j >> 8) & 255]) + bytes(29)


def _stmts(eng, sc, prm, count, tag):
    from ark_bulletproofs_amd.engine import Statement

    return [Statement(eng.curve, sc, prm, _seed(tag, j), eng) for j in range(count)]


def _singles(eng, sc, prm, count, tag):
    return [s.prove(eng)[0] for s in _stmts(eng, sc, prm, count, tag)]


# (scenario, params, count, m_cap): k-shuffles of the reference bench (k = 1024 kept short) and a range proof
# (k = 2 with 130 instances: more than one chunk of 64 proofs, so the host pool runs the per-chunk transcript work)
LIKE = [
    (0, [2], 130, 16), (0, [16], 9, 40), (0, [128], 9, 264), (0, [1024], 2, 2056), (1, [64, 12345], 9, 8), (0, [16], 1, 40),
]


@pytest.mark.parametrize("sc,prm,count,mcap", LIKE)
def test_like_instances_byte_identical_and_lockstep(eng, oracle, sc, prm, count, mcap):
    tag = 17 + sc * 7 + prm[0] % 251
    want = _singles(eng, sc, prm, count, tag)
    l0, s0, g0 = eng.prove_batch_stats()
    got = eng.prove_batch(_stmts(eng, sc, prm, count, tag))
    l1, s1, g1 = eng.prove_batch_stats()
    assert [st for st, _ in got] == [0] * count
    assert [p for _, p in got] == want
    assert l1 - l0 == count and s1 == s0 and g1 > g0          # every instance's argument ran in a lockstep group
    ref = oracle.r1cs_prove(eng.curve, sc, prm, _seed(tag, count - 1), 4096, m_cap=mcap)
    assert ref.rc == 0 and ref.proof == got[-1][1]
    # every proof is accepted by batch_verify, and a one-byte tamper of any one of them is rejected
    insts = []
    for j, s in enumerate(_stmts(eng, sc, prm, count, tag)):
        cm, pubs, _, _ = s.info(mcap)
        insts.append((sc, prm, got[j][1], cm, pubs))
    assert eng.batch_verify(insts, bytes([3]) * 32)[0] == 0
    j = count // 2
    bad = bytearray(insts[j][2])
    bad[len(bad) - 40] ^= 1
    insts[j] = insts[j][:2] + (bytes(bad),) + insts[j][3:]
    assert eng.batch_verify(insts, bytes([3]) * 32)[0] != 0


def test_several_groups_and_single_prove_afterwards(eng):
    want = _singles(eng, 0, [16], 10, 91)
    eng.set_tuning(PROVE_BATCH, 3)
    try:
        g0 = eng.prove_batch_stats()[2]
        got = eng.prove_batch(_stmts(eng, 0, [16], 10, 91))
        assert eng.prove_batch_stats()[2] - g0 == 4          # 3 + 3 + 3 + 1
    finally:
        eng.set_tuning(PROVE_BATCH, 0)
    assert [p for _, p in got] == want
    # a single prove after a batch gives the bytes of a fresh ctx
    import ark_bulletproofs_amd as A

    fresh = A.Engine(curve=eng.curve)
    try:
        fresh.gens_derive(4096)
        a = _stmts(fresh, 0, [128], 1, 92)[0].prove(fresh)[0]
    finally:
        fresh.close()
    assert _stmts(eng, 0, [128], 1, 92)[0].prove(eng)[0] == a


def test_mixed_sizes_and_an_oversized_statement(eng):
    cases = [(0, [2]), (0, [16]), (1, [64, 5]), (0, [2]), (0, [128]), (3, [40, 0]), (0, [16])]
    want = [_singles(eng, sc, prm, 1, 40 + i)[0] for i, (sc, prm) in enumerate(cases)]
    got = eng.prove_batch([_stmts(eng, sc, prm, 1, 40 + i)[0] for i, (sc, prm) in enumerate(cases)])
    assert [p for _, p in got] == want
    # above a lowered BP_TUNE_DIRECT_MAX: proved one at a time inside the call, same bytes
    eng.set_tuning(DIRECT_MAX, 64)
    try:
        l0, s0, _ = eng.prove_batch_stats()
        got = eng.prove_batch([_stmts(eng, 0, [128], 1, 50)[0], _stmts(eng, 0, [2], 1, 51)[0]])
        l1, s1, _ = eng.prove_batch_stats()
    finally:
        eng.set_tuning(DIRECT_MAX, 8192)
    assert [p for _, p in got] == [_singles(eng, 0, [128], 1, 50)[0], _singles(eng, 0, [2], 1, 51)[0]]
    assert s1 - s0 == 1 and l1 - l0 == 1


def test_two_ctxs_sharing_tables_from_two_threads(eng):
    import threading

    import ark_bulletproofs_amd as A

    other = A.Engine(curve=eng.curve)
    try:
        other.share_gens_from(eng)
        want = {t: _singles(eng, 0, [16], 12, t) for t in (61, 62)}
        out = {}

        def run(e, t):
            out[t] = [p for _, p in e.prove_batch(_stmts(e, 0, [16], 12, t))]

        ths = [threading.Thread(target=run, args=(e, t)) for e, t in ((eng, 61), (other, 62))]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert out == want
    finally:
        other.close()


LABEL = b"GenericGadgetTest"
GENS = 256


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng256(request):
    """an engine with 256 generators: a two-phase gadget can outgrow them in its randomized phase"""
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(GENS)
    yield e
    e.close()


def _gadget(eng, F, kind, seed, commit_engine=None, **kw):
    """a recorded prover (tests/gadgets.py) of one of the kinds the mixed batch holds; returns (prover, transcript)"""
    from ark_bulletproofs_amd import engine as A

    import gadgets as GD

    vals, blinds = GD.make_witness(F, seed, 3)
    t = A.HostTranscript(LABEL)
    t.append_message(b"dom-sep", b"generic gadget v1")
    p = A.ProverCS(eng.curve, t)
    _, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds], engine=commit_engine)
    if kind == "nomul":          # commitments only: no multipliers, no inner-product rounds
        return p, t
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    GD.random_program(p, F, seed, wit, vars_, publics=[], **kw)
    if kind == "raise":          # a randomized-phase callback that raises: the thunk returns -100
        def boom(cs):
            raise RuntimeError("callback failure inside a batch")

        p.specify_randomized_constraints(boom)
    return p, t


# (kind, seed, random_program arguments): padded sizes 16 .. 128, one- and two-phase, and two instances that fail on their own
MIXED = [
    ("gadget", 21, dict(n_mul=12)),
    ("gadget", 22, dict(n_mul=30, two_phase=True, n_mul2=20)),
    ("nomul", 23, {}),
    ("raise", 24, dict(n_mul=6)),
    ("gadget", 25, dict(n_mul=5, two_phase=True, n_mul2=5)),
    ("gadget", 26, dict(n_mul=100)),
    ("gadget", 27, dict(n_mul=8, two_phase=True, n_mul2=300)),   # 300 more multipliers than 256 generators: BP_E_GENS_LENGTH
    ("gadget", 28, dict(n_mul=12)),
]


def test_mixed_recorded_gadgets_with_failing_instances(eng256, oracle):
    from ark_bulletproofs_amd import engine as A

    import gadgets as GD

    eng = eng256
    F = GD.Field(oracle, eng.curve)
    rngs = [bytes([7, j]) + bytes(30) for j in range(len(MIXED))]
    want, want_tr = [], []
    for j, (kind, seed, kw) in enumerate(MIXED):
        p, t = _gadget(eng, F, kind, seed, **kw)
        try:
            want.append((0, p.prove(eng, rngs[j])))
        except A.ArkbpError as e:
            want.append((e.code, b""))
        except RuntimeError:
            want.append((-100, b""))
        want_tr.append(A.transcript_state(t))
    assert [w[0] for w in want] == [0, 0, 0, -100, 0, 0, -5, 0]
    made = [_gadget(eng, F, kind, seed, **kw) for kind, seed, kw in MIXED]
    l0, s0, _ = eng.prove_batch_stats()
    rc, got = eng.prove_batch([p for p, _ in made], rng_bytes=rngs, return_rc=True)
    l1, s1, _ = eng.prove_batch_stats()
    assert rc == -100                                   # the first failing status in instance order
    assert got == want                                  # statuses, proof_lens = 0 for the failures, every other proof's bytes
    assert [A.transcript_state(t) for _, t in made] == want_tr
    assert l1 - l0 == 5 and s1 - s0 == 1                # five gadgets in lockstep groups, the commitments-only statement alone


def test_prover_commit_batch_equals_per_prover_commit(eng, oracle):
    from ark_bulletproofs_amd import engine as A

    rs = np.random.default_rng(5)
    vals = [rs.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64) for m in (1, 3, 2)]
    bls = [rs.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64) for m in (1, 3, 2)]
    for x in vals + bls:
        x[:, 3] = 0
    one = [A.ProverCS(eng.curve, A.HostTranscript(b"cb%d" % j)) for j in range(3)]
    many = [A.ProverCS(eng.curve, A.HostTranscript(b"cb%d" % j)) for j in range(3)]
    ref = [p.commit(v, b, engine=eng) for p, v, b in zip(one, vals, bls)]
    got = eng.prover_commit_batch(many, vals, bls)
    for (V0, v0), (V1, v1) in zip(ref, got):
        assert (V0 == V1).all() and v0 == v1
    for p, q in zip(one, many):
        assert A.transcript_state(p.transcript()) == A.transcript_state(q.transcript())
    # the proofs that follow are identical too
    import gadgets as GD

    F = GD.Field(oracle, eng.curve)
    rngs = [bytes([9, j]) + bytes(30) for j in range(3)]
    for j, (p, q) in enumerate(zip(one, many)):
        for cs, (_, vars_) in ((p, ref[j]), (q, got[j])):
            cs.multiply([(vars_[0], F.w(1))], [(vars_[-1], F.w(3))])
    want = [p.prove(eng, rngs[j]) for j, p in enumerate(one)]
    assert [pr for _, pr in eng.prove_batch(many, rng_bytes=rngs)] == want
