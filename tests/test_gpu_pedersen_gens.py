"""PedersenGens { B, B_blinding } of the caller's choice on the GPU (include/arkbp.h: bp_pedersen_gens_install, bp_ctx_pedersen_gens,
bp_prover_new_gens): every table and every route reads the ctx's pair.  The oracle's C API is fixed to the default pair, so the
independent checks are algebraic (pedersen_gens_common): (I) commitments against the oracle's scalar_mul / point_add and, for the
multiples pair, its default pedersen_commit; (II) the oracle's verification scalars over the caller's pair and the proof's own
points sum to the identity; (III) every route of the engine gives the same bytes.

Check (II) covers the scenario statements.  The oracle computes verification scalars for scenarios only, so the 3-multiplier
bp_cs gadget of test 4 is checked by the engine's verifier under both pairs, the oracle's default verifier and the byte
difference, not by (II)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gadgets as GD
import pedersen_gens_common as PG

pytestmark = pytest.mark.gpu
OK, E_ARG, E_VERIFICATION = 0, -1, -4
SC_SHUFFLE, SC_RANGE, SC_EXAMPLE, SC_SQUARE_CHAIN = 0, 1, 2, 3
T_MSM_FIXED_MIN, T_VFY_DEVICE, T_DIRECT_MAX, T_PB_FRONT = 5, 11, 12, 14      # include/arkbp.h BP_TUNE_*
DIRECT_MAX_DEFAULT = 8192
GENS = 64
SEED = bytes([7]) * 32
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r1cs_golden.json")))
NAMES = {0: "secq256k1", 1: "zorro"}
STATEMENTS = [("shuffle_k2", SC_SHUFFLE, [2], 16), ("shuffle_k5", SC_SHUFFLE, [5], 24), ("range_8bit", SC_RANGE, [8, 200], 8),
              ("example", SC_EXAMPLE, [3, 4, 6, 1, 40, 9], 16)]


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def curve(request):
    return request.param


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import engine

    return engine


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fresh(E, curve, which, cap=GENS):
    e = E.Engine(curve=curve)
    e.gens_derive(cap)
    if which != "default":
        e.pedersen_gens_install(*PG.pair(curve, which))
    return e


@pytest.fixture(scope="module")
def chain(E, curve):
    e = fresh(E, curve, "chain")
    yield e
    e.close()


@pytest.fixture(scope="module")
def dflt(E, curve):
    e = fresh(E, curve, "default")
    yield e
    e.close()


@pytest.fixture(scope="module")
def chain_proofs(chain):
    """the statements of tests 4-6 proved once under the chain pair"""
    return {tag: chain.prove_scenario(sc, prm, SEED, m_cap=mcap) for tag, sc, prm, mcap in STATEMENTS}


def holds(e, curve, which):
    B, Bb, d = e.pedersen_gens()
    wB, wBb = PG.pair(curve, which)
    return (B == wB).all() and (Bb == wBb).all() and d == (which == "default")


def golden_scenarios(e, curve):
    for tag, g in GOLD["curves"][NAMES[curve]]["proofs"].items():
        pr = e.prove_scenario(g["scenario"], g["params"], bytes.fromhex(g["seed"]), m_cap=16)
        assert pr.proof.hex() == g["proof"], tag
        assert e.verify_scenario(g["scenario"], g["params"], pr.proof, pr.commitments, pr.publics) == OK


# ---- 1. install and read back ---------------------------------------------------------------------------------------------------
def test_install_and_read_back(E, oracle, curve):
    from ark_bulletproofs_amd._lib import lib

    O = oracle
    e = fresh(E, curve, "default")
    view = E.Engine(curve=curve)
    try:
        assert holds(e, curve, "default")
        B, Bb = PG.pair(curve, "chain")
        e.pedersen_gens_install(B, Bb)
        assert holds(e, curve, "chain")
        e.pedersen_gens_install()
        assert holds(e, curve, "default")
        e.pedersen_gens_install(*PG.pair(curve, "default"))     # the default pair, spelled out, is the default
        assert holds(e, curve, "default")
        e.pedersen_gens_install(B, Bb)
        e.gens_direct_tables(GENS)
        v, bl = PG.edge_scalars(O, curve, 5, seed=3)
        before = e.pedersen_commit_batch(v, bl)
        chk = e.gens_direct_tables_check()
        assert chk[0] == [0] * 4 and chk[2][E.TABLES_DIRECT] > 0 and chk[2][E.TABLES_PC_DIRECT] > 0
        # refusals: pair and tables stay
        off = B.copy(); off[4] ^= np.uint64(1)
        big = B.copy(); big[:4] = O.int_to_limbs(O.modulus(O.fid(curve, False)))
        ident = np.zeros(8, dtype=np.uint64)
        other = PG.pair(curve, "mult")
        for b, bb in ((off, other[1]), (other[0], off), (ident, other[1]), (other[0], ident), (big, other[1]), (other[0], big), (None, other[1]), (other[0], None)):
            assert lib().bp_pedersen_gens_install(e.ctx, None if b is None else _p(b), None if bb is None else _p(bb)) == E_ARG
            assert holds(e, curve, "chain")
        assert lib().bp_pedersen_gens_install(None, _p(B), _p(Bb)) == E_ARG
        assert e.gens_direct_tables_check() == chk
        assert (e.pedersen_commit_batch(v, bl) == before).all()
        # a view reads the owner's pair and refuses an install
        view.share_gens_from(e)
        assert holds(view, curve, "chain")
        assert lib().bp_pedersen_gens_install(view.ctx, _p(other[0]), _p(other[1])) == E_ARG
        assert lib().bp_pedersen_gens_install(view.ctx, None, None) == E_ARG
        assert holds(view, curve, "chain") and (view.pedersen_commit_batch(v, bl) == before).all()
        # the pair survives bp_gens_derive and bp_gens_upload
        e.gens_derive(128)
        assert holds(e, curve, "chain") and (e.pedersen_commit_batch(v, bl) == before).all()
        G, H = O.bp_gens_party(curve, 32, 1)
        e.gens_upload(G, H)
        assert holds(e, curve, "chain") and (e.pedersen_commit_batch(v, bl) == before).all()
        for i in range(5):
            assert (before[i] == PG.commit_expected(O, curve, "chain", v[i], bl[i])).all()
    finally:
        view.close()
        e.close()


# ---- 2. commit batch: both sides of PC_LATENCY_MAX (table 5 and table 6) -----------------------------------------------------------
@pytest.mark.parametrize("which", ["chain", "mult"])
def test_commit_batch(E, oracle, curve, which):
    O = oracle
    e = fresh(E, curve, which)
    try:
        rs = np.random.RandomState(5)
        for m in (1, 5, 4096, 4097):
            v, bl = PG.edge_scalars(O, curve, m, seed=20 + (m % 7))
            if m > 5:     # the edge pairs at the indices that are compared
                ev, eb = PG.edge_scalars(O, curve, 16, seed=1)
                at = [0, 1, 4095] + ([4096] if m > 4096 else [])
                for j, i in enumerate(at):
                    v[i], bl[i] = ev[2 * j + 1], eb[2 * j + 1]
                idx = at + sorted(int(x) for x in rs.choice(m, 32, replace=False))
            else:
                idx = list(range(m))
            got = e.pedersen_commit_batch(v, bl)
            for i in idx:
                assert (got[i] == PG.commit_expected(O, curve, which, v[i], bl[i])).all(), (m, i)
        zero = np.zeros((2, 4), dtype=np.uint64)
        assert not e.pedersen_commit_batch(zero, zero).any()
    finally:
        e.close()


# ---- 3. install after use -----------------------------------------------------------------------------------------------------
def test_install_after_use(E, oracle, curve):
    O = oracle
    cap = 4096      # (bp_gens_msm_tables and its Pedersen rows included)
    e = fresh(E, curve, "default", cap)
    first = fresh(E, curve, "chain", cap)     # installs the pair before anything is built
    try:
        e.gens_direct_tables(GENS)
        v5, b5 = PG.edge_scalars(O, curve, 5, seed=31)
        vL, bL = PG.edge_scalars(O, curve, 4097, seed=32)
        d5, dL = e.pedersen_commit_batch(v5, b5), e.pedersen_commit_batch(vL, bL)
        assert e.gens_msm_tables(cap) > 0
        golden_scenarios(e, curve)
        chk0 = e.gens_direct_tables_check()
        assert chk0[0] == [0] * 4 and all(c > 0 for c in chk0[2])
        e.pedersen_gens_install(*PG.pair(curve, "chain"))
        chk1 = e.gens_direct_tables_check()     # (tables 5 and 6 were dropped: examined again once they are back)
        assert chk1[0] == [0] * 4 and chk1[2][E.TABLES_DIRECT] == chk0[2][E.TABLES_DIRECT]
        assert e.gens_tables_check() == (0, 0)        # the Pedersen rows of bp_gens_msm_tables follow the resident pair
        c5, cL = e.pedersen_commit_batch(v5, b5), e.pedersen_commit_batch(vL, bL)
        assert (c5 == first.pedersen_commit_batch(v5, b5)).all() and (cL == first.pedersen_commit_batch(vL, bL)).all()
        assert not (c5 == d5).all()
        for i in range(5):
            assert (c5[i] == PG.commit_expected(O, curve, "chain", v5[i], b5[i])).all()
        chk2 = e.gens_direct_tables_check()
        assert chk2[0] == [0] * 4 and chk2[2] == chk0[2]
        pa, pb = e.prove_scenario(SC_SHUFFLE, [2], SEED, m_cap=16), first.prove_scenario(SC_SHUFFLE, [2], SEED, m_cap=16)
        assert pa.proof == pb.proof and (pa.commitments == pb.commitments).all()
        assert not PG.proof_check_point(O, curve, "chain", SC_SHUFFLE, [2], cap, pa.proof, pa.commitments, pa.publics).any()
        # and a statement large enough to read the Pedersen rows
        for x in (e, first):
            x.set_tuning(T_DIRECT_MAX, 0)
            x.set_tuning(T_MSM_FIXED_MIN, 4096)
        runs = e.msm_stats()[0]
        qa, qb = e.prove_scenario(SC_SQUARE_CHAIN, [2048, 0], SEED, m_cap=8), first.prove_scenario(SC_SQUARE_CHAIN, [2048, 0], SEED, m_cap=8)
        assert e.msm_stats()[0] > runs and qa.proof == qb.proof
        e.set_tuning(T_DIRECT_MAX, DIRECT_MAX_DEFAULT)
        # back to the default: the golden bytes again
        e.pedersen_gens_install()
        assert holds(e, curve, "default")
        assert (e.pedersen_commit_batch(v5, b5) == d5).all() and (e.pedersen_commit_batch(vL, bL) == dL).all()
        golden_scenarios(e, curve)
        chk3 = e.gens_direct_tables_check()
        assert chk3[0] == [0] * 4 and chk3[2] == chk0[2]
    finally:
        first.close()
        e.close()


# ---- 4. prove -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,sc,prm,mcap", STATEMENTS, ids=[s[0] for s in STATEMENTS])
def test_prove_scenarios(oracle, curve, chain, dflt, chain_proofs, tag, sc, prm, mcap):
    O = oracle
    pr = chain_proofs[tag]
    assert chain.verify_scenario(sc, prm, pr.proof, pr.commitments, pr.publics) == OK
    assert not PG.proof_check_point(O, curve, "chain", sc, prm, GENS, pr.proof, pr.commitments, pr.publics).any()        # (II)
    assert PG.proof_check_point(O, curve, "default", sc, prm, GENS, pr.proof, pr.commitments, pr.publics).any()
    assert dflt.verify_scenario(sc, prm, pr.proof, pr.commitments, pr.publics) == E_VERIFICATION
    assert O.r1cs_verify(curve, sc, prm, GENS, pr.proof, pr.commitments, pr.publics) != 0
    ref = dflt.prove_scenario(sc, prm, SEED, m_cap=mcap)
    assert ref.proof != pr.proof and not (np.asarray(ref.commitments) == np.asarray(pr.commitments)).all()
    assert (np.asarray(ref.publics) == np.asarray(pr.publics)).all()
    # the statement handle built on the ctx carries the ctx's pair (bp_stmt_prover_create_dev): same bytes
    from ark_bulletproofs_amd import engine as E

    st = E.Statement(curve, sc, prm, SEED, engine=chain)
    assert (st.info()[0] == pr.commitments).all()
    assert st.prove(chain)[0] == pr.proof


def small_gadget(cs, F, vars_, wit):
    """3 multipliers over two commitments: (a + 2) * (b - 1), its output times a, an allocated pair; outputs pinned to allocated variables"""
    proving = wit is not None
    a, b = vars_

    def W(lc):
        return [(v, F.w(c)) for v, c in lc]

    def mul(left, right):
        l, r, o = cs.multiply(W(left), W(right))
        if proving:
            wit.val[l], wit.val[r] = wit.eval(left), wit.eval(right)
            wit.val[o] = wit.val[l] * wit.val[r] % F.p
        return l, r, o

    _, _, o1 = mul([(a, 1), (GD.ONE, 2)], [(b, 1), (GD.ONE, F.p - 1)])
    _, _, o2 = mul([(o1, 1)], [(a, 1)])
    l3, r3, o3 = cs.allocate_multiplier((F.w(wit.val[o2]), F.w(3)) if proving else None)
    if proving:
        wit.val[l3], wit.val[r3], wit.val[o3] = wit.val[o2], 3, wit.val[o2] * 3 % F.p
    cs.constrain(W([(l3, 1), (o2, F.p - 1)]))
    cs.constrain(W([(r3, 1), (GD.ONE, F.p - 3)]))
    cs.constrain(W([(o3, 1), (o2, F.p - 3)]))


def test_prove_own_gadget(E, oracle, curve, chain, dflt):
    O = oracle
    F = GD.Field(O, curve)
    label = b"pedersen gens gadget"
    vals, blinds = [17, 4], [123456789, F.p - 5]

    def prove(eng, pc_gens, on_ctx):
        p = E.ProverCS(curve, E.HostTranscript(label), pc_gens=pc_gens)
        V, vars_ = p.commit([F.w(x) for x in vals], [F.w(x) for x in blinds], engine=eng if on_ctx else None)
        wit = GD.Witness(F)
        for var, x in zip(vars_, vals):
            wit.val[var] = x
        small_gadget(p, F, vars_, wit)
        assert p.metrics()[0] == 3
        return V, p.prove(eng, bytes([5]) * 32)

    def verify(eng, V, proof):
        v = E.VerifierCS(curve, E.HostTranscript(label))
        small_gadget(v, F, v.commit(V), None)
        return v.verify(eng, proof)

    V, proof = prove(chain, PG.pair(curve, "chain"), False)
    V2, proof2 = prove(chain, PG.pair(curve, "chain"), True)          # commitments through the ctx's tables: the same statement
    assert (V == V2).all() and proof == proof2
    for i in range(2):
        assert (V[i] == PG.commit_expected(O, curve, "chain", F.w(vals[i]), F.w(blinds[i]))).all()
    assert verify(chain, V, proof) == OK
    assert verify(dflt, V, proof) == E_VERIFICATION
    ov = O.VerifierCS(curve, label).start()
    small_gadget(ov, F, ov.commit(V), None)
    assert ov.verify(GENS, proof) != 0
    Vd, proofd = prove(dflt, None, False)
    assert proofd != proof and not (Vd == V).all()
    assert verify(dflt, Vd, proofd) == OK
    od = O.VerifierCS(curve, label).start()
    small_gadget(od, F, od.commit(Vd), None)
    assert od.verify(GENS, proofd) == 0       # (the gadget itself is sound under the oracle)


# ---- 5. route agreement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,sc,prm,mcap", [STATEMENTS[1], STATEMENTS[2]], ids=["shuffle_k5", "range_8bit"])
def test_routes_agree(E, curve, chain, chain_proofs, tag, sc, prm, mcap):
    want = chain_proofs[tag].proof
    N = 8
    # not over the direct window tables
    chain.set_tuning(T_DIRECT_MAX, 0)
    try:
        assert chain.prove_scenario(sc, prm, SEED, m_cap=mcap).proof == want
        # ... and with first-round fold tables
        chain.gens_fold_tables(N // 2)
        assert chain.prove_scenario(sc, prm, SEED, m_cap=mcap).proof == want
        chain.gens_fold_tables(0)
    finally:
        chain.set_tuning(T_DIRECT_MAX, DIRECT_MAX_DEFAULT)
    # batch proving, group-wide front stages and not
    seeds = [SEED, bytes([8]) * 32, bytes([9]) * 32, SEED]
    singles = []
    for s in seeds:
        st = E.Statement(curve, sc, prm, s, engine=chain)
        singles.append(st.prove(chain)[0])
    assert singles[0] == want and singles[3] == want and singles[1] != want
    for front in (1, 0):
        chain.set_tuning(T_PB_FRONT, front)
        try:
            f0 = chain.prove_batch_front_stats()[0]
            res = chain.prove_batch([E.Statement(curve, sc, prm, s, engine=chain) for s in seeds])
            assert [r[0] for r in res] == [OK] * 4 and [r[1] for r in res] == singles, front
            assert (chain.prove_batch_front_stats()[0] - f0 > 0) == bool(front)
        finally:
            chain.set_tuning(T_PB_FRONT, 1)


def test_fixed_base_rows_route(E, oracle, curve):
    """one square chain of 2^11 multipliers: the smallest size at which the Pedersen rows of bp_gens_msm_tables are read at all"""
    O = oracle
    cap = 2048
    e = fresh(E, curve, "chain", cap)
    try:
        e.set_tuning(T_DIRECT_MAX, 0)
        e.set_tuning(T_MSM_FIXED_MIN, 4096)
        plain = e.prove_scenario(SC_SQUARE_CHAIN, [cap, 0], SEED, m_cap=8)
        assert e.msm_stats()[0] == 0
        assert e.gens_msm_tables(cap) > 0
        rows = e.prove_scenario(SC_SQUARE_CHAIN, [cap, 0], SEED, m_cap=8)
        assert e.msm_stats()[0] > 0, "the fixed-base schedule did not run"
        assert rows.proof == plain.proof
        e.gens_fold_tables(cap // 2)             # the first fold round from the fold tables (read from padded size 128 on)
        assert e.prove_scenario(SC_SQUARE_CHAIN, [cap, 0], SEED, m_cap=8).proof == plain.proof
        assert e.verify_scenario(SC_SQUARE_CHAIN, [cap, 0], rows.proof, rows.commitments, rows.publics) == OK
        assert not PG.proof_check_point(O, curve, "chain", SC_SQUARE_CHAIN, [cap, 0], cap, rows.proof, rows.commitments, rows.publics).any()
        assert e.gens_tables_check() == (0, 0)
    finally:
        e.close()


# ---- 6. verify routes -------------------------------------------------------------------------------------------------------------
def shuffle_gadget(cs, F, x, y, wit):
    """the reference's k-shuffle gadget (benches/r1cs_secq256k1.rs:34-76) over the trait API: prod (x_i - z) = prod (y_i - z)"""
    k = len(x)
    assert k >= 2

    def W(lc):
        return [(v, F.w(c)) for v, c in lc]

    def randomized(cs2):
        z = F.i(cs2.challenge_scalar(b"shuffle challenge"))
        proving = wit is not None

        def mul(left, right):
            l, r, o = cs2.multiply(W(left), W(right))
            if proving:
                wit.val[l], wit.val[r] = wit.eval(left), wit.eval(right)
                wit.val[o] = wit.val[l] * wit.val[r] % F.p
            return o

        def chain_of(vs):
            out = mul([(vs[k - 1], 1), (GD.ONE, F.p - z)], [(vs[k - 2], 1), (GD.ONE, F.p - z)])
            for i in range(k - 3, -1, -1):
                out = mul([(out, 1)], [(vs[i], 1), (GD.ONE, F.p - z)])
            return out

        cs2.constrain(W([(chain_of(x), 1), (chain_of(y), F.p - 1)]))

    cs.specify_randomized_constraints(randomized)


def range_gadget(cs, F, v, value, n):
    """the reference's range proof gadget (tests/r1cs_secq256k1.rs:361-399): v = sum b_i 2^i with b_i (1 - b_i) = 0"""
    W = lambda lc: [(var, F.w(c)) for var, c in lc]
    lc = [(v, 1)]
    for i in range(n):
        bit = None if value is None else (value >> i) & 1
        a, b, o = cs.allocate_multiplier(None if bit is None else (F.w(1 - bit), F.w(bit)))
        cs.constrain(W([(o, 1)]))
        cs.constrain(W([(a, 1), (b, 1), (GD.ONE, F.p - 1)]))
        lc.append((b, F.p - (1 << i)))
    cs.constrain(W(lc))


def wire_of(O, curve, V):
    return b"".join(O.point_ser(curve, p, True) for p in V)


@pytest.mark.parametrize("kind", ["shuffle_k2", "range_8bit"])
def test_verify_routes(E, oracle, curve, chain, dflt, kind):
    O = oracle
    F = GD.Field(O, curve)
    label = b"pedersen gens routes"
    n = 8
    two_phase = kind == "shuffle_k2"

    def record(cs, vars_, wit, value=None):
        if two_phase:
            shuffle_gadget(cs, F, vars_[:2], vars_[2:], wit)
        else:
            range_gadget(cs, F, vars_[0], value, 8)

    items = []
    for j in range(n):
        vals = [1000 + j, 77 + 3 * j, 77 + 3 * j, 1000 + j] if two_phase else [200 - j]
        blinds = [(j + 2) * 1234567 + i for i in range(len(vals))]
        p = E.ProverCS(curve, E.HostTranscript(label), pc_gens=PG.pair(curve, "chain"))
        V, vars_ = p.commit([F.w(x) for x in vals], [F.w(x) for x in blinds], engine=chain)
        wit = GD.Witness(F)
        for var, x in zip(vars_, vals):
            wit.val[var] = x
        record(p, vars_, wit, vals[0])
        items.append((p.prove(chain, bytes([j + 1]) * 32), V))
    bad_at = 5
    bad = bytearray(items[bad_at][0]); bad[11 * 33] ^= 1          # a flipped bit in t_x
    proofs_ok = [it[0] for it in items]
    proofs_bad = list(proofs_ok); proofs_bad[bad_at] = bytes(bad)
    alphas = O.fe_rand(O.fid(curve, True), bytes([33]) * 32, n)

    def verifiers(wired):
        def commit(v, V):
            return v.commit_compressed(wire_of(O, curve, V), defer=True) if wired else v.commit(V)

        v0 = E.VerifierCS(curve, E.HostTranscript(label))
        record(v0, commit(v0, items[0][1]), None)
        out = [v0]
        for j in range(1, n):
            v = E.VerifierCS(curve, E.HostTranscript(label), like=v0)
            commit(v, items[j][1])
            out.append(v)
        return out

    def batch(eng, proofs, knob, wired):
        eng.set_tuning(T_VFY_DEVICE, knob)
        try:
            d0 = eng.vfe_stats()
            rc, pt = E.batch_verify_cs(eng, verifiers(wired), proofs, alphas, want_point=True)
            d1 = eng.vfe_stats()
        finally:
            eng.set_tuning(T_VFY_DEVICE, 1)
        return rc, pt, (d1[0] - d0[0], d1[1] - d0[1])

    for wired in (False, True):
        for proofs, want in ((proofs_bad, E_VERIFICATION), (proofs_ok, OK)):
            want_each = [OK] * n
            if want != OK:
                want_each[bad_at] = E_VERIFICATION
            rc_d, pt_d, used_d = batch(chain, proofs, 2, wired)
            rc_h, pt_h, used_h = batch(chain, proofs, 0, wired)
            assert used_d == (1, 0), "the device front end did not complete the batch"
            assert used_h == (0, 0)
            assert rc_d == want and rc_h == want and (pt_d == pt_h).all() and pt_d.any() == (want != OK)
            g0 = chain.verify_each_stats()
            rc, st = chain.verify_each(verifiers(wired), proofs)
            g1 = chain.verify_each_stats()
            assert st == want_each and rc == want
            assert g1[0] - g0[0] == n and g1[1] == g0[1], "verify_each left the grouped path"
            rc, st = E.batch_verify_locate_cs(chain, verifiers(wired), proofs, alphas)
            assert st == want_each and rc == want
    # the ctx's pair is the pc_gens of verify: the same valid batch under the default pair fails everywhere
    assert batch(dflt, proofs_ok, 2, False)[0] == E_VERIFICATION and batch(dflt, proofs_ok, 0, False)[0] == E_VERIFICATION
    assert dflt.verify_each(verifiers(False), proofs_ok)[1] == [E_VERIFICATION] * n


def test_verify_routes_scenario_forms(oracle, curve, chain, dflt, chain_proofs):
    n = 8
    for tag, sc, prm in (("shuffle_k2", SC_SHUFFLE, [2]), ("range_8bit", SC_RANGE, [8, 200])):
        pr = chain_proofs[tag]
        inst = [(sc, prm, pr.proof, pr.commitments, pr.publics)] * n
        bad = bytearray(pr.proof); bad[11 * 33] ^= 1
        inst_bad = list(inst); inst_bad[3] = (sc, prm, bytes(bad), pr.commitments, pr.publics)
        for knob in (2, 0):
            chain.set_tuning(T_VFY_DEVICE, knob)
            try:
                rc, _, pt = chain.batch_verify(inst, SEED, want_point=True)
                assert rc == OK and not pt.any()
                rcb, _, ptb = chain.batch_verify(inst_bad, SEED, want_point=True)
                assert rcb == E_VERIFICATION and ptb.any()
            finally:
                chain.set_tuning(T_VFY_DEVICE, 1)
        want_each = [OK] * n; want_each[3] = E_VERIFICATION
        assert chain.verify_each_scenarios(inst_bad)[1] == want_each
        assert chain.batch_verify_locate(inst_bad, SEED)[1] == want_each
        assert chain.verify_each_scenarios(inst)[1] == [OK] * n
        assert dflt.batch_verify(inst, SEED)[0] == E_VERIFICATION
        assert dflt.verify_each_scenarios(inst)[1] == [E_VERIFICATION] * n


# ---- 7. mismatch --------------------------------------------------------------------------------------------------------------
def test_mismatch(E, oracle, curve, chain):
    from ark_bulletproofs_amd._lib import ArkbpError

    O = oracle
    F = GD.Field(O, curve)
    label = b"pedersen gens mismatch"
    mult = fresh(E, curve, "mult")
    try:
        def prover(vals):
            t = E.HostTranscript(label)
            p = E.ProverCS(curve, t, pc_gens=PG.pair(curve, "mult"))
            return p, t

        vals, blinds = [17, 4], [99, 100]
        v, b = [F.w(x) for x in vals], [F.w(x) for x in blinds]
        p, t = prover(vals)
        before = E.transcript_state(t)
        with pytest.raises(ArkbpError) as ei:
            p.commit(v, b, engine=chain)
        assert ei.value.code == E_ARG and "prover 0" in str(ei.value)
        with pytest.raises(ArkbpError) as ei:
            chain.prover_commit_batch([p], [v], [b])
        assert ei.value.code == E_ARG
        assert E.transcript_state(t) == before and p.metrics()[2] == 0
        V, vars_ = p.commit(v, b)                       # on the host, under the handle's pair
        wit = GD.Witness(F)
        for var, x in zip(vars_, vals):
            wit.val[var] = x
        small_gadget(p, F, vars_, wit)
        state = E.transcript_state(t)
        with pytest.raises(ArkbpError) as ei:
            p.prove(chain, bytes([5]) * 32)
        assert ei.value.code == E_ARG and E.transcript_state(t) == state
        # a batch with one such prover among provers of the ctx's pair: refused as a whole, no prover consumed
        others = []
        for j in range(2):
            q = E.ProverCS(curve, E.HostTranscript(label), pc_gens=PG.pair(curve, "chain"))
            Vq, vq = q.commit(v, b, engine=chain)
            wq = GD.Witness(F)
            for var, x in zip(vq, vals):
                wq.val[var] = x
            small_gadget(q, F, vq, wq)
            others.append((q, Vq))
        group = [others[0][0], p, others[1][0]]
        with pytest.raises(ArkbpError) as ei:
            chain.prove_batch(group, rng_bytes=[bytes([5]) * 32] * 3)
        assert ei.value.code == E_ARG and "prover 1" in str(ei.value)
        assert E.transcript_state(t) == state
        # nobody was consumed: each proves where its pair is held
        proof = p.prove(mult, bytes([5]) * 32)
        res = chain.prove_batch([o[0] for o in others], rng_bytes=[bytes([5]) * 32] * 2)
        assert [r[0] for r in res] == [OK, OK]

        def verify(eng, V, pf):
            vr = E.VerifierCS(curve, E.HostTranscript(label))
            small_gadget(vr, F, vr.commit(V), None)
            return vr.verify(eng, pf)

        assert verify(mult, V, proof) == OK and verify(chain, V, proof) == E_VERIFICATION
        assert verify(chain, others[0][1], res[0][1]) == OK
        for i in range(2):
            assert (V[i] == PG.commit_expected(O, curve, "mult", v[i], b[i])).all()
    finally:
        mult.close()


# ---- 8. default untouched -----------------------------------------------------------------------------------------------------------
def test_default_untouched(E, curve, dflt):
    golden_scenarios(dflt, curve)
    e = fresh(E, curve, "chain")
    try:
        pr = e.prove_scenario(SC_SHUFFLE, [2], SEED, m_cap=16)
        assert pr.proof.hex() != GOLD["curves"][NAMES[curve]]["proofs"]["shuffle_k2"]["proof"]
        e.pedersen_gens_install()
        golden_scenarios(e, curve)
    finally:
        e.close()
