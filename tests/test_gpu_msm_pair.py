"""The L and R MSMs of an inner-product round as two jobs of one launch chain (msm_run_pair, BP_TUNE_MSM_PAIR): through the test
hook bp_debug_msm_pair every pair must equal two single runs (bp_msm_dev) AND the oracle's MSM — sums of the same group elements,
so the affine words are equal exactly — at the sizes where the routing changes, and the prover must keep emitting the oracle's
proof bytes with the knob on and off.  After every case that should pair, the counter of bp_ctx_msm_pair_stats must have advanced:
a silent fallback to two calls does not pass."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes([7]) * 32
K = 4096              # G = P[0:K], H = P[K:2K], Q = P[2K]: one allocation, as the prover's working vectors lie
IDENTITIES = (2, 70, K + 1, K + 300)   # identity bases among the points, inside the runs of every size below


class _Data:
    def __init__(self, eng, O):
        cv = eng.curve
        G, H = O.bp_gens(cv, K)
        Q = O.point_add(cv, G[5], H[9])
        self.P = np.concatenate([G, H, Q.reshape(1, 8)])
        for i in IDENTITIES:
            self.P[i] = 0
        self.dP = eng.upload_points(self.P)
        self.FR = O.fid(cv, True)
        self.r = O.modulus(self.FR)

    def host_bases(self, runs):
        return np.concatenate([self.P[first:first + count] for first, count in runs])

    def dev_runs(self, runs):
        return [(self.dP, first, count) for first, count in runs]


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(eng, oracle):
    return _Data(eng, oracle)


def _round_runs(n):
    """the two three-run descriptors of an un-frozen round over one [G | H | Q] allocation: L = [G_hi | H_lo | Q], R = [G_lo | H_hi | Q]"""
    a = (n - 1) // 2
    b = n - 1 - a
    return [(b, a), (K, b), (2 * K, 1)], [(0, a), (K + a, b), (2 * K, 1)]


def _uniform(O, data, n, seed):
    return O.fe_rand(data.FR, bytes([seed]) * 32, n)


def _check(eng, O, data, n, scalars, runs, expect_pair, redone=0, latency_first=False, canonical=False):
    """scalars: two (n, 4) arrays of ark Montgomery words; with canonical the device gets the integers below r instead"""
    cv = eng.curve
    dev_sc = scalars
    if canonical:
        dev_sc = [np.array([O.int_to_limbs(O.fe_to_int(data.FR, x)) for x in s]) for s in scalars]
    d_s = [eng.upload_scalars(s) for s in dev_sc]
    before = eng.msm_pair_stats()
    got = eng.debug_msm_pair([data.dev_runs(r) for r in runs], d_s, n, canonical=canonical, latency_first=latency_first)
    after = eng.msm_pair_stats()
    assert after[0] - before[0] == (1 if expect_pair else 0), "paired passes %s -> %s" % (before, after)
    assert after[1] - before[1] == redone, "jobs redone %s -> %s" % (before, after)
    for j in range(2):
        B = data.host_bases(runs[j])
        d_b = eng.upload_points(B)
        single = eng.msm_dev(d_b, d_s[j], n, canonical=canonical)
        d_b.free()
        assert (got[j] == single).all(), "job %d differs from the single run" % j
        assert (got[j] == O.msm(cv, B, scalars[j])).all(), "job %d differs from the oracle" % j
    for d in d_s:
        d.free()
    return got


@pytest.mark.parametrize("n", [63, 64, 513, 4097])
def test_pair_at_the_sizes_where_routing_changes(eng, oracle, data, n):
    """63 is below BP_TUNE_MSM_BIN_MIN = 64: two calls, still right.  64 is the first paired size, 513 the frozen shape 2 * 256 + 1,
    4097 more than one bin.  Uniform scalars; the same descriptor twice (the frozen tail) and the two descriptors of an un-frozen
    round; the prover's schedule (latency_first = 0)."""
    O = oracle
    L, R = _round_runs(n)
    sc = [_uniform(O, data, n, 21), _uniform(O, data, n, 22)]
    _check(eng, O, data, n, sc, [L, L], expect_pair=n >= 64)
    _check(eng, O, data, n, sc, [L, R], expect_pair=n >= 64)


@pytest.mark.parametrize("kind", ["job0_zero", "job1_zero", "frozen_supports", "special_values"])
@pytest.mark.parametrize("n", [64, 513])
def test_pair_scalar_patterns(eng, oracle, data, n, kind):
    O = oracle
    L, R = _round_runs(n)
    zero, one, rm1 = O.fe_from_int(data.FR, 0), O.fe_from_int(data.FR, 1), O.fe_from_int(data.FR, data.r - 1)
    sc = [_uniform(O, data, n, 31), _uniform(O, data, n, 32)]
    if kind == "job0_zero":        # the identity beside an ordinary sum
        sc[0][:] = zero
    elif kind == "job1_zero":
        sc[1][:] = zero
    elif kind == "frozen_supports":   # as k_ipa_frozen_scalars writes them: every base belongs to exactly one of L, R; the last term (Q) to both
        own = (np.arange(n - 1) // 4) % 2 == 0
        sc[0][:n - 1][~own] = zero
        sc[1][:n - 1][own] = zero
    else:                          # 0, 1 and r - 1 mixed in, in different places of the two jobs
        for j, s in enumerate(sc):
            s[3 + j::7] = zero
            s[4 + j::11] = one
            s[5 + j::13] = rm1
    got = _check(eng, O, data, n, sc, [L, R] if kind != "frozen_supports" else [L, L], expect_pair=True, canonical=kind == "special_values")
    if kind == "job0_zero":
        assert not got[0].any() and got[1].any()
    if kind == "job1_zero":
        assert got[0].any() and not got[1].any()


def test_pair_declined_by_the_latency_first_route(eng, oracle, data):
    """what the bp_msm* entry points set: on secq256k1 a 513-term MSM then goes through the GLV split, which is not paired — two
    calls, same results; zorro has no endomorphism and pairs with the quad-cooperative trees"""
    O, n = oracle, 513
    L, R = _round_runs(n)
    sc = [_uniform(O, data, n, 41), _uniform(O, data, n, 42)]
    _check(eng, O, data, n, sc, [L, R], expect_pair=eng.curve != 0, latency_first=True)


def test_pair_overflow_redoes_one_job_and_restores_the_zero_invariants(eng, oracle, data):
    """every scalar of a job equal: each window holds one bucket of 513 entries, above the 256 the fixed shape takes, so that job's
    overflow word is raised and it alone is redone on the general path.  The runs directly afterwards on the same ctx — an ordinary
    pair and a single MSM — find hist, the bin cursors and both overflow words all-zero again, or they would be wrong."""
    O, n = oracle, 513
    L, R = _round_runs(n)
    uni = [_uniform(O, data, n, 51), _uniform(O, data, n, 52)]
    same = np.tile(uni[0][17], (n, 1))
    _check(eng, O, data, n, [same, uni[1]], [L, R], expect_pair=True, redone=1)
    _check(eng, O, data, n, uni, [L, R], expect_pair=True)
    _check(eng, O, data, n, [uni[0], same], [L, R], expect_pair=True, redone=1)
    _check(eng, O, data, n, uni, [L, L], expect_pair=True)
    B = data.host_bases(R)
    d_b, d_s = eng.upload_points(B), eng.upload_scalars(uni[1])
    assert (eng.msm_dev(d_b, d_s, n) == O.msm(eng.curve, B, uni[1])).all()
    d_b.free()
    d_s.free()


# ---- the prover ----------------------------------------------------------------------------------------------------------------
N = 1 << 11
PROVE_CASES = [(3, [N, 0]), (0, [N // 2 + 1])]   # square chain; a shuffle of N multipliers (two phases)
M_CAP = N + 16
_refs = {}


def _ref(oracle, cv, sc, prm):
    key = (cv, sc, tuple(prm))
    if key not in _refs:
        _refs[key] = oracle.r1cs_prove(cv, sc, prm, SEED, N, m_cap=M_CAP)
        assert _refs[key].rc == 0
    return _refs[key]


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def gens(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(N)
    yield e
    e.close()


def _prover_engine(gens, freeze, pair):
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E

    e = A.Engine(curve=gens.curve)
    e.share_gens_from(gens)
    e.set_tuning(12, 0)        # BP_TUNE_DIRECT_MAX: not the small-statement path
    e.set_tuning(0, 1)         # BP_TUNE_FOLD_BATCH_MIN
    e.set_tuning(1, 1)         # BP_TUNE_MSM_BIN_MIN: every round's MSMs take the two-level sort
    e.set_tuning(2, freeze)    # BP_TUNE_IPA_FREEZE_LEN
    e.set_tuning(E.TUNE_MSM_PAIR, pair)
    return e


@pytest.mark.parametrize("sc,prm", PROVE_CASES, ids=["square_chain", "shuffle"])
def test_prover_bytes_with_the_knob_on_and_off(gens, oracle, sc, prm):
    """un-frozen rounds to the end (freeze 0) and the frozen tail from length 256 on, paired and not: the oracle's bytes four times,
    and paired passes exactly when the knob is 1"""
    ref = _ref(oracle, gens.curve, sc, prm)
    for freeze in (0, 256):
        for pair in (0, 1):
            e = _prover_engine(gens, freeze, pair)
            got = e.prove_scenario(sc, prm, SEED, m_cap=M_CAP)
            passes, _ = e.msm_pair_stats()
            e.close()
            assert got.proof == ref.proof and (got.commitments == ref.commitments).all(), (freeze, pair)
            assert (passes > 0) == (pair == 1), (freeze, pair, passes)


def test_two_ctxs_prove_concurrently(gens, oracle):
    """per-ctx buffers only: two ctxs over shared generators, one thread each, both statements on both"""
    from ark_bulletproofs_amd import engine as E

    cv = gens.curve
    refs = [_ref(oracle, cv, sc, prm) for sc, prm in PROVE_CASES]
    engs = [_prover_engine(gens, 256, 1) for _ in range(2)]
    stmts = [[E.Statement(cv, sc, prm, SEED) for sc, prm in (PROVE_CASES if t == 0 else PROVE_CASES[::-1])] for t in range(2)]
    out = [[], []]

    def work(t):
        for st in stmts[t]:
            out[t].append(st.prove(engs[t])[0])

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert out[0] == [refs[0].proof, refs[1].proof]
    assert out[1] == [refs[1].proof, refs[0].proof]
    for e in engs:
        assert e.msm_pair_stats()[0] > 0
        e.close()
