"""Blinding vectors from a key on the GPU (include/arkbp.h BP_BLINDING_EXPANDED; csrc/blind.cuh): the kernel against its host twin and
the Python restatement, S1 / S2 of expanded-mode proofs rebuilt from an independent model of the TranscriptRng and the expansion,
validity under the oracle's verifier and the product's, the same bytes on every proving route, the counters, determinism.

The gadget is a chain of multiply() calls on two committed variables: it has exactly the multiplier counts the test names (no
allocate() halves), is satisfiable for every witness, and its randomized phase takes a challenge."""
import random

import numpy as np
import pytest

from test_blinding_cpu import GRID, R_MOD, ark_words, from_ark, kappas, model

pytestmark = pytest.mark.gpu
DIRECT_MAX, FRONT = 12, 14   # BP_TUNE_DIRECT_MAX, BP_TUNE_PROVE_BATCH_FRONT
LABEL = b"BlindingGadgetTest"
GENS = 16384
OGENS = 1024   # what the oracle derives for the small statements (a prefix of the same chain)
ONE = (4, 0)


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(GENS)
    yield e
    e.close()


# ---- 1. the kernel against the host twin and the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("j0,count", GRID + [(0, c) for c in (63, 64, 65, 127, 128, 129, 255, 256, 1025)] + [(5, 128)])
def test_kernel_equals_host_twin_and_model(eng, j0, count):
    """256 lanes per workgroup, 2 count lanes in all: counts around 128 straddle a workgroup, around 32 / 64 a wave, 1025 needs nine"""
    from ark_bulletproofs_amd import engine as A

    r = R_MOD[eng.curve]
    for kappa in kappas(eng.curve):
        k = ark_words(kappa, r)
        dL, dR = eng.debug_blind_expand(k, j0, count)
        hL, hR = A.host_blind_expand(eng.curve, k, j0, count)
        assert (dL == hL).all() and (dR == hR).all()
        if kappa in (0, r - 1) or count <= 65:
            wL, wR = model(eng.curve, kappa, j0, count)
            assert from_ark(dL, r) == wL and from_ark(dR, r) == wR


# ---- the gadget, the model of prove()'s draws -------------------------------------------------------------------------------------
class Case:
    """one statement: n1 multipliers in phase 1, n2 in a randomized phase, witness and rng bytes from `seed`"""

    def __init__(self, oracle, curve, n1, n2, seed):
        import gadgets as GD

        self.O, self.curve, self.n1, self.n2, self.seed = oracle, curve, n1, n2, seed
        self.F = GD.Field(oracle, curve)
        rw = random.Random(seed)
        self.vals = [rw.randrange(self.F.p), rw.randrange(1 << 32)]
        self.blinds = [rw.randrange(self.F.p) for _ in range(2)]
        self.rng = bytes(rw.randrange(256) for _ in range(32))
        self.V = None

    def record(self, cs, vars_):
        F, n2 = self.F, self.n2
        v0, v1 = vars_
        for i in range(self.n1):
            cs.multiply([(v0, F.w(i + 1))], [(v1, F.w(1)), (ONE, F.w(i))])
        if n2:
            def randomized(cs2):
                z = F.i(cs2.challenge_scalar(b"blinding gadget challenge"))
                for i in range(n2):
                    cs2.multiply([(v0, F.w(z + i))], [(v1, F.w(1)), (ONE, F.w(z))])

            cs.specify_randomized_constraints(randomized)

    def prover(self, mode, rng=None):
        """a recorded product prover; returns (prover, transcript)"""
        from ark_bulletproofs_amd import engine as A

        t = A.HostTranscript(LABEL)
        t.append_message(b"dom-sep", b"blinding gadget v1")
        p = A.ProverCS(self.curve, t)
        V, vars_ = p.commit([self.F.w(v) for v in self.vals], [self.F.w(b) for b in self.blinds])
        self.V = V
        self.record(p, vars_)
        p.set_blinding(mode)
        return p, t

    def prove(self, eng, mode, rng=None):
        p, _ = self.prover(mode)
        return p.prove(eng, rng or self.rng)

    def verify_product(self, eng, proof):
        from ark_bulletproofs_amd import engine as A

        t = A.HostTranscript(LABEL)
        t.append_message(b"dom-sep", b"blinding gadget v1")
        v = A.VerifierCS(self.curve, t)
        self.record(v, v.commit(self.V))
        return v.verify(eng, proof)

    def verify_oracle(self, proof):
        v = self.O.VerifierCS(self.curve, LABEL)
        v.transcript().append_message(b"dom-sep", b"blinding gadget v1")
        v.start()
        self.record(v, v.commit(self.V))
        return v.verify(OGENS, proof)

    def model_draws(self, state203):
        """(s_blinding1, kappa1, s_blinding2, kappa2) as ints from the independent TranscriptRng model (tests/pystrobe.py), started at
        the transcript state prove() finds: append_u64("m"), the v_blinding rekeys, the external bytes, then Fr::rand draws in the
        order of the expanded mode"""
        import pystrobe as PS

        p = self.F.p
        s = PS.Strobe128.__new__(PS.Strobe128)
        s.st, s.pos, s.pos_begin, s.cur = bytearray(state203[:200]), state203[200], state203[201], state203[202]
        tm = PS.Transcript.__new__(PS.Transcript)
        tm.s = s
        tm.append_u64(b"m", 2)
        b = tm.build_rng()
        for vb in self.blinds:
            b.rekey_with_witness_bytes(b"v_blinding", vb.to_bytes(32, "little"))
        rng = b.finalize(self.rng)

        def fr_rand():   # ark-ff Fp::rand: raw limbs (top limb masked to the modulus width), accepted iff < p; they are the Montgomery form
            while True:
                limbs = [rng.next_u64() for _ in range(4)]
                limbs[3] &= (1 << (64 - (256 - p.bit_length()))) - 1
                v = sum(l << (64 * i) for i, l in enumerate(limbs))
                if v < p:
                    return v * pow(1 << 256, -1, p) % p

        _, _, s_b1 = fr_rand(), fr_rand(), fr_rand()
        k1 = fr_rand() if self.n1 else None
        s_b2 = k2 = None
        if self.n2:
            _, _, s_b2 = fr_rand(), fr_rand(), fr_rand()
            k2 = fr_rand()
        return s_b1, k1, s_b2, k2

    def model_S(self, s_b, kappa, first, count):
        """s_b * B_blinding + <s_L, G[first ..]> + <s_R, H[first ..]> through the oracle's MSM, compressed"""
        O, F = self.O, self.F
        G, H = O.bp_gens(self.curve, first + count)
        _, Bb = O.pedersen_default(self.curve)
        sL, sR = model(self.curve, kappa, 0, count)
        bases = np.concatenate([np.asarray(Bb, dtype=np.uint64).reshape(1, 8), G[first:first + count], H[first:first + count]])
        scal = np.array([F.w(s_b)] + [F.w(x) for x in sL] + [F.w(x) for x in sR], dtype=np.uint64)
        return O.point_ser(self.curve, O.msm(self.curve, bases, scal), True)


def _state_before_prove(case, mode):
    from ark_bulletproofs_amd import engine as A

    p, t = case.prover(mode)
    return p, A.transcript_state(t)


# ---- 2. S1 from the model, single phase ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", [1, 3, 64, 65])
def test_S1_is_the_models(eng, oracle, n1):
    from ark_bulletproofs_amd import engine as A

    case = Case(oracle, eng.curve, n1, 0, 7000 + n1)
    p, state = _state_before_prove(case, A.BLINDING_EXPANDED)
    assert p.metrics()[0] == n1
    proof = p.prove(eng, case.rng)
    default = case.prove(eng, A.BLINDING_TRANSCRIPT)
    s_b1, k1, _, _ = case.model_draws(state)
    assert proof[66:99] == case.model_S(s_b1, k1, 0, n1)
    assert proof[:66] == default[:66] and proof[66:99] != default[66:99]
    # 4. validity
    assert case.verify_oracle(proof) == 0 and case.verify_product(eng, proof) == 0
    bad = bytearray(proof)
    bad[70] ^= 1
    assert case.verify_product(eng, bytes(bad)) != 0 and case.verify_oracle(bytes(bad)) != 0


# ---- 3. two phases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(3, 2), (5, 70)])
def test_S2_is_the_models(eng, oracle, n1, n2):
    """n1 odd and n2 > 0: kappa2 comes after the three phase-2 scalars, the phase-local index restarts at 0 and the bases at n1"""
    from ark_bulletproofs_amd import engine as A

    case = Case(oracle, eng.curve, n1, n2, 7100 + n1)
    p, state = _state_before_prove(case, A.BLINDING_EXPANDED)
    proof = p.prove(eng, case.rng)
    default = case.prove(eng, A.BLINDING_TRANSCRIPT)
    s_b1, k1, s_b2, k2 = case.model_draws(state)
    assert proof[66:99] == case.model_S(s_b1, k1, 0, n1)
    assert proof[165:198] == case.model_S(s_b2, k2, n1, n2)
    assert proof[:66] == default[:66] and proof[66:99] != default[66:99]
    assert case.verify_oracle(proof) == 0 and case.verify_product(eng, proof) == 0
    bad = bytearray(proof)
    bad[70] ^= 1
    assert case.verify_product(eng, bytes(bad)) != 0


@pytest.mark.parametrize("k", [2, 3, 8])
def test_shuffle_has_no_phase1_key(eng, oracle, k):
    """a k-shuffle has n1 = 0: no kappa1, A_I1 / A_O1 / S1 are the default mode's single Pedersen terms; S2 is not the default's"""
    from ark_bulletproofs_amd import engine as A

    seed = bytes([60 + k]) * 32
    s = A.Statement(eng.curve, 0, [k], seed, eng)
    s.set_blinding(A.BLINDING_EXPANDED)
    cm, pubs, _, _ = s.info(64)
    proof = s.prove(eng)[0]
    default = A.Statement(eng.curve, 0, [k], seed, eng).prove(eng)[0]
    assert default == oracle.r1cs_prove(eng.curve, 0, [k], seed, OGENS, m_cap=64).proof
    assert proof[:165] == default[:165] and proof[165:198] != default[165:198]       # (A_I2, A_O2 come from the same draws too)
    assert eng.verify_scenario(0, [k], proof, cm, pubs) == 0
    assert oracle.r1cs_verify(eng.curve, 0, [k], OGENS, proof, cm, pubs) == 0
    bad = bytearray(proof)
    bad[170] ^= 1
    assert eng.verify_scenario(0, [k], bytes(bad), cm, pubs) != 0


# ---- 5. route independence --------------------------------------------------------------------------------------------------------------
def _routes(eng, case, mode):
    """the proof of `case` through every route: {route name: bytes}"""
    from ark_bulletproofs_amd import engine as A
    from ark_bulletproofs_amd._lib import check, lib
    import ctypes as C

    out = {"direct": case.prove(eng, mode)}
    eng.set_tuning(DIRECT_MAX, 0)
    try:
        out["large"] = case.prove(eng, mode)
    finally:
        eng.set_tuning(DIRECT_MAX, 8192)
    p, _ = case.prover(mode)
    p.precompute(case.rng)
    out["precompute"] = p.prove(eng, case.rng)
    eight = [case.prover(mode)[0] for _ in range(8)]
    for q in eight:
        check(lib().bp_prover_set_rng(q.h, case.rng), "bp_prover_set_rng")
    check(lib().bp_prover_precompute_batch((C.c_void_p * 8)(*[q.h for q in eight]), C.c_size_t(8)), "bp_prover_precompute_batch")
    out["precompute_batch"] = eight[3].prove(eng, case.rng)
    for knob in (1, 0):
        eng.set_tuning(FRONT, knob)
        try:
            got = eng.prove_batch([case.prover(mode)[0] for _ in range(3)], rng_bytes=[case.rng] * 3)
        finally:
            eng.set_tuning(FRONT, 1)
        assert [st for st, _ in got] == [0, 0, 0] and got[0][1] == got[1][1] == got[2][1]
        out["batch_front_%d" % knob] = got[0][1]
    return out


@pytest.mark.parametrize("n1,n2", [(3, 0), (65, 0), (300, 0), (3, 62), (65, 235)])
def test_every_route_gives_the_same_bytes(eng, oracle, n1, n2):
    from ark_bulletproofs_amd import engine as A

    case = Case(oracle, eng.curve, n1, n2, 7200 + n1 + n2)
    f0 = eng.prove_batch_front_stats()
    routes = _routes(eng, case, A.BLINDING_EXPANDED)
    assert eng.prove_batch_front_stats()[0] - f0[0] == 3                      # the front groups did take the batch with the knob at 1
    assert len(set(routes.values())) == 1, {k: v[:8].hex() for k, v in routes.items()}
    assert case.verify_product(eng, routes["direct"]) == 0


def test_mixed_batch(eng, oracle):
    """both modes in one call, equal and different sizes: the default-mode members are the oracle's bytes, the expanded ones those of
    a single prove"""
    from ark_bulletproofs_amd import engine as A

    cases = [Case(oracle, eng.curve, n1, n2, 7300 + j) for j, (n1, n2) in enumerate([(5, 0), (5, 0), (5, 3), (5, 3), (9, 0), (9, 0)])]
    modes = [A.BLINDING_EXPANDED, A.BLINDING_TRANSCRIPT] * 3
    want = [c.prove(eng, m) for c, m in zip(cases, modes)]
    for knob in (1, 0):
        eng.set_tuning(FRONT, knob)
        try:
            got = eng.prove_batch([c.prover(m)[0] for c, m in zip(cases, modes)], rng_bytes=[c.rng for c in cases])
        finally:
            eng.set_tuning(FRONT, 1)
        assert [st for st, _ in got] == [0] * 6 and [p for _, p in got] == want
    for c, m, proof in zip(cases, modes, want):
        if m == A.BLINDING_TRANSCRIPT:
            ref = oracle.ProverCS(eng.curve, LABEL)
            ref.transcript().append_message(b"dom-sep", b"blinding gadget v1")
            ref.start()
            _, vars_ = ref.commit([c.F.w(v) for v in c.vals], [c.F.w(b) for b in c.blinds])
            c.record(ref, vars_)
            assert ref.prove(OGENS, c.rng) == proof
        assert c.verify_product(eng, proof) == 0


def test_above_the_fused_upload_threshold(eng, oracle):
    """8 200 multipliers in one phase: above UPLOAD_FUSED_MAX (the three witness vectors go up as separate copies), 65 workgroups of the
    expansion, the large path whatever the knobs say"""
    from ark_bulletproofs_amd import engine as A

    n = 8200
    case = Case(oracle, eng.curve, n, 0, 7400)
    s0 = eng.blinding_stats()
    p, state = _state_before_prove(case, A.BLINDING_EXPANDED)
    proof = p.prove(eng, case.rng)
    s1 = eng.blinding_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (2 * n, 1)
    q, _ = case.prover(A.BLINDING_EXPANDED)
    q.precompute(case.rng)
    assert q.prove(eng, case.rng) == proof
    got = eng.prove_batch([case.prover(A.BLINDING_EXPANDED)[0]], rng_bytes=[case.rng])
    assert got == [(0, proof)]
    s_b1, k1, _, _ = case.model_draws(state)
    # S1 against the host twin's vectors here (the Python restatement of 16 400 blocks would take a minute; the twin equals it above)
    G, H = oracle.bp_gens(eng.curve, n)
    _, Bb = oracle.pedersen_default(eng.curve)
    sL, sR = A.host_blind_expand(eng.curve, ark_words(k1, case.F.p), 0, n)
    bases = np.concatenate([np.asarray(Bb, dtype=np.uint64).reshape(1, 8), G, H])
    scal = np.concatenate([np.asarray(case.F.w(s_b1), dtype=np.uint64).reshape(1, 4), sL, sR])
    assert proof[66:99] == oracle.point_ser(eng.curve, oracle.msm(eng.curve, bases, scal), True)
    assert case.verify_product(eng, proof) == 0


# ---- 6. counters ------------------------------------------------------------------------------------------------------------------------
def test_stats(eng, oracle):
    from ark_bulletproofs_amd import engine as A

    single = Case(oracle, eng.curve, 37, 0, 7500)
    two = Case(oracle, eng.curve, 5, 12, 7501)
    s0 = eng.blinding_stats()
    single.prove(eng, A.BLINDING_TRANSCRIPT)
    two.prove(eng, A.BLINDING_TRANSCRIPT)
    assert eng.blinding_stats() == s0                                          # the default mode expands nothing
    single.prove(eng, A.BLINDING_EXPANDED)
    s1 = eng.blinding_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (2 * 37, 1)
    two.prove(eng, A.BLINDING_EXPANDED)
    s2 = eng.blinding_stats()
    assert (s2[0] - s1[0], s2[1] - s1[1]) == (2 * 17, 2)                       # one launch per non-empty phase
    eng.set_tuning(DIRECT_MAX, 0)
    try:
        two.prove(eng, A.BLINDING_EXPANDED)
    finally:
        eng.set_tuning(DIRECT_MAX, 8192)
    s3 = eng.blinding_stats()
    assert (s3[0] - s2[0], s3[1] - s2[1]) == (2 * 17, 2)
    # a front group of B members: one launch for the phase-1 stage and one for the whole witness, whatever B is; the phase-1 vectors
    # are expanded for both (include/arkbp.h bp_ctx_blinding_stats)
    for B in (1, 6):
        a = eng.blinding_stats()
        f0 = eng.prove_batch_front_stats()
        got = eng.prove_batch([two.prover(A.BLINDING_EXPANDED)[0] for _ in range(B)], rng_bytes=[two.rng] * B)
        b = eng.blinding_stats()
        assert [st for st, _ in got] == [0] * B and eng.prove_batch_front_stats()[0] - f0[0] == B
        assert b[1] - a[1] == 2 and b[0] - a[0] == B * (2 * 5 + 2 * 17)
    # a default-mode group launches none
    a = eng.blinding_stats()
    eng.prove_batch([two.prover(A.BLINDING_TRANSCRIPT)[0] for _ in range(3)], rng_bytes=[two.rng] * 3)
    assert eng.blinding_stats() == a


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------------
def test_determinism(eng, oracle):
    from ark_bulletproofs_amd import engine as A

    case = Case(oracle, eng.curve, 33, 4, 7600)
    a = case.prove(eng, A.BLINDING_EXPANDED)
    assert case.prove(eng, A.BLINDING_EXPANDED) == a
    other = case.prove(eng, A.BLINDING_EXPANDED, rng=bytes([1]) + case.rng[1:])
    assert other[66:99] != a[66:99] and other[165:198] != a[165:198]
    assert case.verify_product(eng, other) == 0
