"""The verifier front end on the device for TWO-PHASE statements (BP_TUNE_VFY_DEVICE = 2; include/arkbp.h "verifier front end on
the device"): the device derives every challenge of a batch of like-instances — the gadget challenges that
specify_randomized_constraints' callbacks draw included (src/r1cs/verifier.rs:353-376) — the host runs each instance's callbacks
with its challenges preset, and the device evaluates the per-proof coefficient tables they produce.  Checked here, on both curves:
accept / reject and the mega-check POINT against the host replay (knob 0) and the oracle, for the reference's k-shuffle
(benches/r1cs_secq256k1.rs:34-76) through the scenario entry point and for generic gadgets through recorded handles; callbacks
whose structure depends on the challenge make the device decline; knob 1 keeps two-phase batches on the host replay; the class
cache decides its coefficient table per batch (a template rebuilt with other public constants between two device batches)."""
import numpy as np
import pytest

import gadgets as GD

pytestmark = pytest.mark.gpu
OK, E_VERIFICATION, E_FORMAT = 0, -4, -6
SC_SHUFFLE, SC_SQUARE_CHAIN = 0, 3
TUNE_VFY_DEVICE = 11
GENS = 2048
LABEL = b"vfe two-phase gadget"


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(GENS)
    yield e
    e.close()


def make_batch(eng, sc, prm, count, distinct, m_cap):
    base = [eng.prove_scenario(sc, prm, bytes([70 + i]) * 32, m_cap=m_cap) for i in range(distinct)]
    return [(sc, prm, base[i % distinct].proof, base[i % distinct].commitments, base[i % distinct].publics) for i in range(count)]


def run(eng, instances, seed, knob):
    eng.set_tuning(TUNE_VFY_DEVICE, knob)
    try:
        d0, f0 = eng.vfe_stats()
        rc, _, pt = eng.batch_verify(instances, seed, want_point=True)
        d1, f1 = eng.vfe_stats()
    finally:
        eng.set_tuning(TUNE_VFY_DEVICE, 1)
    return rc, pt, (d1 - d0, f1 - f0)


@pytest.mark.parametrize("k,count,distinct", [(2, 600, 3), (3, 20, 4), (64, 9, 3), (1024, 3, 2)])
def test_shuffle_batches_on_the_device(eng, oracle, k, count, distinct):
    O, cv = oracle, eng.curve
    seed = bytes([9]) * 32
    inst = make_batch(eng, SC_SHUFFLE, [k], count, distinct, 2 * k + 8)
    rc, pt, used = run(eng, inst, seed, 2)
    assert used == (1, 0), "the device front end did not take a batch of two-phase like-instances"
    assert rc == OK and not pt.any()
    # knob 1: today's behaviour, the host replay
    rc1, pt1, used1 = run(eng, inst, seed, 1)
    assert used1 == (0, 0) and rc1 == OK and not pt1.any()
    # a wrong t_x in one proof: VerificationError with the host replay's (and the oracle's) point
    bad_at = count - 1
    s, p, proof, cm, pb = inst[bad_at]
    bad = bytearray(proof); bad[363 + 5] ^= 4
    inst_bad = list(inst); inst_bad[bad_at] = (s, p, bytes(bad), cm, pb)
    rc_d, pt_d, used = run(eng, inst_bad, seed, 2)
    rc_h, pt_h, used_h = run(eng, inst_bad, seed, 0)
    assert used == (1, 0) and used_h == (0, 0)
    assert rc_d == E_VERIFICATION and rc_h == E_VERIFICATION and pt_d.any() and (pt_d == pt_h).all()
    if count <= 20 and k <= 64:
        rc_o, pt_o = O.batch_verify_point(cv, inst_bad, GENS, seed)
        assert rc_o != 0 and (np.asarray(pt_o, dtype=np.uint64).reshape(-1) == pt_d).all(), "mega-check point differs from the oracle's MSM"
    # swapped commitments in one instance
    cm2 = np.array(inst[1][3], dtype=np.uint64).reshape(-1, 8).copy()
    cm2[[0, 1]] = cm2[[1, 0]]
    inst_bad = list(inst); inst_bad[1] = (inst[1][0], inst[1][1], inst[1][2], cm2, inst[1][4])
    rc_d, pt_d, used = run(eng, inst_bad, seed, 2)
    rc_h, pt_h, _ = run(eng, inst_bad, seed, 0)
    assert used == (1, 0) and rc_d == E_VERIFICATION and rc_h == E_VERIFICATION and (pt_d == pt_h).all()
    # a malformed point (flag bits the deserializer rejects): the kernels flag it, the host replay reports FormatError
    bad = bytearray(inst[1][2]); bad[4 * 33 + 32] = 0xC0
    inst_bad = list(inst); inst_bad[1] = (inst[1][0], inst[1][1], bytes(bad), inst[1][3], inst[1][4])
    rc_d, _, used = run(eng, inst_bad, seed, 2)
    assert rc_d == E_FORMAT and used == (0, 1)


def test_nonidentity_phase2_points_pass_the_point_kernel(eng):
    """A_I2, A_O2, S2 of a two-phase proof are not the identity (append_point, not validate_and_append_point): k_vfe_points raises
    no status bit for them"""
    from ark_bulletproofs_amd import engine as E

    pr = eng.prove_scenario(SC_SHUFFLE, [4], bytes([3]) * 32, m_cap=16)
    assert any(pr.proof[33 * j + 32] != 0x40 for j in (3, 4, 5))
    t = E.HostTranscript(b"ShuffleBenchmark")
    st = E.transcript_state(t)
    _, _, status = eng.debug_vfe_challenges([pr.proof], np.asarray(pr.commitments, dtype=np.uint64).reshape(1, -1, 8), st, True)
    assert status == 0


# ---- generic two-phase gadgets through recorded handles (bp_verifier_new_like) -------------------------------------------------
KW = dict(n_mul=9, n_extra=1, n_alloc=1, n_mul2=4)   # (n_extra = 1: no public constants, so instances with their own witnesses are like-instances)


def extra_phase2(cs, F, vars_, wit, dependent):
    """a second randomized callback with its own challenge: phase-2 terms on commitments with challenge-dependent coefficients;
    `dependent`: an extra multiplier when the challenge is odd (a structure that depends on the challenge's value)"""
    proving = wit is not None

    def W(lc):
        return [(v, F.w(c)) for v, c in lc]

    def cb(cs2):
        w = F.i(cs2.challenge_scalar(b"second gadget challenge with a longer label"))
        left = [(vars_[0], w), (GD.ONE, 3)]
        right = [(vars_[1], (F.p - w) % F.p), (vars_[2], 1)]
        for _ in range(1 + (w & 1) if dependent else 1):
            l, r, o = cs2.multiply(W(left), W(right))
            if proving:
                wit.val[l], wit.val[r] = wit.eval(left), wit.eval(right)
                wit.val[o] = wit.val[l] * wit.val[r] % F.p

    cs.specify_randomized_constraints(cb)


def program(cs, F, vars_, wit, dependent):
    GD.random_program(cs, F, 23, wit, vars_, two_phase=True, publics=[], **KW)
    extra_phase2(cs, F, vars_, wit, dependent)


def product_prove(E, eng, F, wit_seed, m, dependent):
    vals, blinds = GD.make_witness(F, wit_seed, m)
    t = E.HostTranscript(LABEL)
    p = E.ProverCS(eng.curve, t)
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    program(p, F, vars_, wit, dependent)
    return p.prove(eng, bytes([wit_seed & 255]) * 32), V


def product_verifier(E, curve, F, V, dependent, like=None):
    v = E.VerifierCS(curve, E.HostTranscript(LABEL), like=like)
    vars_ = v.commit(V)
    if like is None:
        program(v, F, vars_, None, dependent)
    return v


def oracle_verifier(O, curve, F, V, dependent):
    v = O.VerifierCS(curve, LABEL)
    v.start()
    vars_ = v.commit(V)
    program(v, F, vars_, None, dependent)
    return v


@pytest.mark.parametrize("dependent", [False, True], ids=["shared-structure", "challenge-dependent-structure"])
@pytest.mark.parametrize("curve", [0, 1])
def test_recorded_two_phase_like_instances(oracle, curve, dependent):
    from ark_bulletproofs_amd import engine as E

    O = oracle
    eng = E.Engine(curve=curve, device=0)
    eng.gens_derive(256)
    try:
        F = GD.Field(O, curve)
        m, count = 3, 16
        items = [product_prove(E, eng, F, 200 + w, m, dependent) for w in range(count)]
        alphas = O.fe_rand(O.fid(curve, True), bytes([8]) * 32, count)

        def build(bad=None):
            pf = [it[0] for it in items]
            if bad is not None:
                b = bytearray(pf[bad]); b[-40] ^= 2; pf[bad] = bytes(b)
            v0 = product_verifier(E, curve, F, items[0][1], dependent)
            vs = [v0] + [product_verifier(E, curve, F, items[i][1], dependent, like=v0) for i in range(1, count)]
            return vs, pf

        plens = {len(it[0]) for it in items}
        for bad in (None, 5):
            vs, pf = build(bad)
            eng.set_tuning(TUNE_VFY_DEVICE, 2)
            d0, f0 = eng.vfe_stats()
            rc_d, pt_d = E.batch_verify_cs(eng, vs, pf, alphas, want_point=True)
            d1, f1 = eng.vfe_stats()
            vs, _ = build(bad)
            eng.set_tuning(TUNE_VFY_DEVICE, 0)
            rc_h, pt_h = E.batch_verify_cs(eng, vs, pf, alphas, want_point=True)
            eng.set_tuning(TUNE_VFY_DEVICE, 1)
            ov = [oracle_verifier(O, curve, F, items[i][1], dependent) for i in range(count)]
            rc_o, pt_o = O.batch_verify_cs(curve, ov, pf, 256, alphas)
            if dependent:
                assert (d1 - d0, f1 - f0) == (0, 0), "the device took a batch whose phase-2 structure differs between instances"
            else:
                assert len(plens) == 1 and (d1 - d0, f1 - f0) == (1, 0)
            assert rc_d == rc_h == (OK if bad is None else E_VERIFICATION)
            assert (rc_o == 0) == (bad is None)
            assert (pt_d == pt_h).all() and (pt_d == np.asarray(pt_o, dtype=np.uint64).reshape(-1)).all()
    finally:
        eng.close()


def test_class_cache_decides_the_coefficient_table_per_batch(eng):
    """A single-phase statement with a public constant (the square chain's output) goes through the device front end; more than
    64 other templates go through the host replay and evict its template; the same structure with OTHER constants rebuilds it;
    then the first statement's batch goes through the device front end again: its valid proofs are accepted and a proof made for
    the other constants is rejected (the device class must not keep the coefficient choice it made against the old template)."""
    seed = bytes([11]) * 32
    a = eng.prove_scenario(SC_SQUARE_CHAIN, [100, 0], bytes([1]) * 32)
    b = eng.prove_scenario(SC_SQUARE_CHAIN, [100, 0], bytes([2]) * 32)
    assert (np.asarray(a.publics) != np.asarray(b.publics)).any()
    inst_a = [(SC_SQUARE_CHAIN, [100, 0], a.proof, a.commitments, a.publics)] * 4
    rc, _, used = run(eng, inst_a, seed, 1)
    assert rc == OK and used == (1, 0)
    others = [eng.prove_scenario(SC_SQUARE_CHAIN, [L, 0], bytes([3]) * 32) for L in range(1, 67)]
    host = [(SC_SQUARE_CHAIN, [L, 0], pr.proof, pr.commitments, pr.publics) for L, pr in zip(range(1, 67), others)]
    for batch in (host, host[:8]):     # the second batch finds > 64 templates and evicts every one it does not use
        rc, _, used = run(eng, batch, seed, 1)
        assert rc == OK and used == (0, 0)
    rc, _, used = run(eng, [(SC_SQUARE_CHAIN, [100, 0], b.proof, b.commitments, b.publics)], seed, 1)   # rebuilds the template from b's constants
    assert rc == OK and used == (0, 0)
    rc, pt, used = run(eng, inst_a, seed, 1)
    assert used == (1, 0) and rc == OK and not pt.any()
    forged = inst_a[:3] + [(SC_SQUARE_CHAIN, [100, 0], b.proof, b.commitments, a.publics)]   # b's valid proof against a's public constant
    rc, pt, used = run(eng, forged, seed, 1)
    assert used == (1, 0) and rc == E_VERIFICATION and pt.any()
