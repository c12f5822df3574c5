"""The recorder API and the newer prover / verifier modes on a SHARDED ctx (include/arkbp.h bp_ctx_set_window_shard,
bp_ctx_set_shard_allgather): ranks as threads of this process (tests/shardcommon.py), one ctx each on the same GPU, world 2 (Pippenger
windows partitioned and the inner-product argument index-cyclic), world 3 (not a power of two: windows only, an uneven partition,
folds replicated) and, for the phase shapes, world 4.

Every leg asserts its result on EVERY rank — proof bytes against the CPU oracle's, verdicts, check points and counters against an
unsharded ctx or the header's statement — and, from the ranks' collective logs, that the sharded path ran: every rank made the same
collectives in the same order (shardcommon.run_ranks), an MSM ended in a point-reduce, and a proof made exactly one vector gather
where the cyclic argument applies and none where it does not.  A mode that adds or skips an MSM on one rank ends as a failed wait,
not as a hung suite.  Each leg names the branch it is there for."""
import numpy as np
import pytest

import batchref as BR
import commit_wire_common as CW
import gadgets as GD
import likecommon as LC
import pedersen_gens_common as PG
import shardcommon as SC
import test_gpu_cs_api as CS
import test_gpu_witness_dev as WD
import wcheck as W

pytestmark = pytest.mark.gpu
GENS = 128
OK, E_ARG, E_VERIFICATION, E_FORMAT, E_UNSATISFIED = 0, -1, -4, -6, -8
TUNE_MSM_FIXED_MIN, TUNE_VFY_DEVICE, TUNE_DIRECT_MAX = 5, 11, 12     # include/arkbp.h BP_TUNE_*
CURVES, WORLDS = [0, 1], [2, 3]
_CACHE = {}         # oracle proofs and unsharded results, computed once per module on the main thread


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def singles(E):
    """per curve: an unsharded ctx with the ranks' generators — what the sharded ranks are compared with where the oracle has no say"""
    out = {}
    for cv in CURVES:
        e = E.Engine(curve=cv, device=0)
        e.gens_derive(GENS)
        out[cv] = e
    yield out
    for e in out.values():
        e.close()


def cyclic(world):
    return world & (world - 1) == 0


def span(e, fn):
    """(fn(), the collectives this rank made inside it)"""
    at = len(e.shard_log)
    res = fn()
    return res, list(e.shard_log[at:])


def assert_proof_path(log, world, proofs=1):
    """the sharded prover ran: MSMs met in point-reduces, and one vector gather per proof iff the argument went index-cyclic"""
    assert SC.points(log) >= proofs, log
    assert SC.vectors(log) == (proofs if cyclic(world) else 0), (world, log)


def same_on_all_ranks(res):
    for r in range(1, len(res)):
        assert res[r] == res[0], "rank %d differs from rank 0: %r vs %r" % (r, res[r], res[0])
    return res[0]


def flip_txb(proof):
    b = bytearray(proof)
    b[BR.TXB_BYTE] ^= 1          # the lowest bit of t_x_blinding: still a well-formed proof
    return bytes(b)


def padded_from_proof(proof):
    fixed = 11 * 33 + 3 * 32 + 16 + 2 * 32
    assert (len(proof) - fixed) % 66 == 0
    return 1 << ((len(proof) - fixed) // 66)


def recorder_prove(E, eng, F, struct_seed, wit_seed, two_phase, kw, blinding=None, guard=False, pc_gens=None):
    """test_gpu_cs_api.product_prove with the prover's modes: (proof, V, publics)"""
    vals, blinds = GD.make_witness(F, wit_seed, 3)
    t = E.HostTranscript(CS.LABEL)
    t.append_message(b"dom-sep", b"generic gadget v1")
    p = E.ProverCS(eng.curve, t, pc_gens=pc_gens)
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    publics = []
    GD.random_program(p, F, struct_seed, wit, vars_, two_phase=two_phase, publics=publics, **kw)
    if blinding is not None:
        p.set_blinding(blinding)
    if guard:
        p.set_check(True)
    return p.prove(eng, bytes([wit_seed & 255]) * 32), V, publics


# ---- A. recorder API, phase shapes ------------------------------------------------------------------------------------------------------
SHAPES_A = [(0, 16), (8, 16), (16, 16), (5, 11), (12, 17), (100, 100), (40, 100)]     # (phase-1 multipliers, multipliers)


def program_a(n1, n):
    """random_program arguments for n1 phase-1 multipliers of n (the randomized phase adds n_mul2 products and three allocations: 2 more)"""
    if n1 == n:
        return dict(n_mul=n, n_alloc=0, n_extra=0), False
    return dict(n_mul=n1, n_alloc=0, n_extra=0, n_mul2=n - n1 - 2), True


def refs_a(E, O, curve, F):
    def make():
        out = []
        for n1, n in SHAPES_A:
            kw, two = program_a(n1, n)
            seed = 100 + 7 * n1 + n
            # the counts the shape stands for, from the recorder itself (host only) and from the proof's length
            vals, blinds = GD.make_witness(F, 5, 3)
            p = E.ProverCS(curve, E.HostTranscript(CS.LABEL))
            _, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
            wit = GD.Witness(F)
            for var, v in zip(vars_, vals):
                wit.val[var] = v
            GD.random_program(p, F, seed, wit, vars_, two_phase=two, **kw)
            assert p.metrics()[0] == n1
            ref = CS.oracle_prove(O, curve, F, seed, 5, 3, two, **kw)
            N = 1
            while N < n:
                N *= 2
            assert padded_from_proof(ref[0]) == N
            out.append((seed, kw, two, ref))
        return out

    return cached(("A", curve), make)


def rare_oracle(O, curve, F):
    def make():
        vals, blinds = GD.make_witness(F, 6, 3)
        p = O.ProverCS(curve, CS.LABEL)
        p.start()
        V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
        wit = GD.Witness(F)
        for var, v in zip(vars_, vals):
            wit.val[var] = v
        GD.rare_shapes_program(p, F, wit, vars_, two_phase=True)
        return p.prove(GENS, bytes([6]) * 32), V

    return cached(("A-rare", curve), make)


def rare_product(E, eng, F):
    vals, blinds = GD.make_witness(F, 6, 3)
    p = E.ProverCS(eng.curve, E.HostTranscript(CS.LABEL))
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    GD.rare_shapes_program(p, F, wit, vars_, two_phase=True)
    return p.prove(eng, bytes([6]) * 32), V


def rare_verifier(E, curve, F, V):
    v = E.VerifierCS(curve, E.HostTranscript(CS.LABEL))
    GD.rare_shapes_program(v, F, None, v.commit(V), two_phase=True)
    return v


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("curve", CURVES)
def test_a_recorder_api_phase_shapes(E, oracle, curve, world):
    """csrc/r1cs_host.inc:1059-1066 with ipa_create_cyclic (csrc/arkbp.hip:2434): the factor hint gf_const_halves — true as n1 = 0,
    n1 = N / 2 and n1 >= N, false as n1 < N / 2 and N / 2 < n1 < N — and the per-rank geometric tables (rho_r, rho_mr, kH), for
    recorded gadgets, padded and not; world 4 with (0, 16): n_loc = 4 and S_glob = 4, the smallest argument ipa_cyclic_applies takes.
    ProverCS.prove equals the oracle's Prover byte for byte on every rank; VerifierCS.verify accepts, rejects a flipped t_x_blinding
    bit with -4 and a truncated proof with -6."""
    F = GD.Field(oracle, curve)
    refs = refs_a(E, oracle, curve, F)
    rare_ref, rare_V = rare_oracle(oracle, curve, F)
    assert padded_from_proof(rare_ref) == 32

    def verdicts(e, make_verifier, proof):
        out = []
        for bad, want in ((proof, OK), (flip_txb(proof), E_VERIFICATION), (proof[:-1], E_FORMAT)):
            rc, log = span(e, lambda: make_verifier().verify(e, bad))
            assert rc == want, (rc, want)
            if want != E_FORMAT:
                assert SC.points(log) >= 1 and SC.vectors(log) == 0, log     # the mega-check's MSM met in a point-reduce
            out.append(rc)
        return out

    def body(rank, e):
        for (n1, n), (seed, kw, two, (ref, Vo, pubs_o)) in zip(SHAPES_A, refs):
            (proof, V, pubs), log = span(e, lambda: CS.product_prove(E, e, F, seed, 5, 3, two, **kw))
            assert (V == Vo).all() and pubs == pubs_o
            assert proof == ref, "rank %d: (n1, n) = (%d, %d): proof bytes differ from the oracle's" % (rank, n1, n)
            assert_proof_path(log, world)
            verdicts(e, lambda: CS.product_verifier(E, curve, F, seed, V, pubs, two, **kw), proof)
        (proof, V), log = span(e, lambda: rare_product(E, e, F))
        assert (V == rare_V).all() and proof == rare_ref, "rank %d: rare shapes: proof bytes differ from the oracle's" % rank
        assert_proof_path(log, world)
        verdicts(e, lambda: rare_verifier(E, curve, F, V), proof)
        return True

    assert SC.run_ranks(world, curve, body, GENS) == [True] * world


# ---- B. phase-2 commitments with an offset, per-rank blocks ---------------------------------------------------------------------------
B_N1, B_N2, B_GENS = 100, 4096, 8192


def program_b(cs, F, words, bulk):
    """100 allocated multipliers in phase 1 and 4096 in the randomized phase (N = 8192), one row per phase on the first of them;
    bulk: through allocate_multipliers (the product), else one allocate_multiplier each (the oracle)"""
    L1, R1, L2, R2 = words

    def alloc(c, L, R):
        if bulk:
            return (GD.VAR_MULT_LEFT, c.allocate_multipliers(L, R))
        first = None
        for l, r in zip(L, R):
            v = c.allocate_multiplier((l, r))
            first = v[0] if first is None else first
        return tuple(first)

    l0 = alloc(cs, L1, R1)
    cs.constrain([(l0, F.w(1)), (GD.ONE, F.w(F.p - F.i(L1[0])))])

    def randomized(c):
        z = F.i(c.challenge_scalar(b"leg b challenge"))
        l2 = alloc(c, L2, R2)
        c.constrain([(l2, F.w(z)), (GD.ONE, F.w((F.p - z * F.i(L2[0])) % F.p))])

    cs.specify_randomized_constraints(randomized)


def words_b(O, curve):
    FR = O.fid(curve, True)
    a, b = O.fe_rand(FR, bytes([0xB1]) * 32, 2 * B_N1), O.fe_rand(FR, bytes([0xB2]) * 32, 2 * B_N2)
    return a[:B_N1].copy(), a[B_N1:].copy(), b[:B_N2].copy(), b[B_N2:].copy()


def prove_b(E, eng, F, words):
    t = E.HostTranscript(b"ShardedLegB")
    p = E.ProverCS(eng.curve, t)
    p.commit([F.w(77)], [F.w(99)])
    program_b(p, F, words, True)
    assert p.metrics()[0] == B_N1
    return p.prove(eng, bytes([0xB3]) * 32)


def test_b_phase2_commitments_per_rank_blocks(E, oracle):
    """csrc/r1cs_host.inc:243-260, the per-rank BLOCK of a commitment's terms with off > 0: a recorded statement with 100 phase-1
    and 4096 phase-2 multipliers, fixed-base rows over 8192 generators, BP_TUNE_MSM_FIXED_MIN = 4096, two ranks.  A_I2 and S2
    (8193 terms, 4096 per rank) take the block partition starting at G[100 + lo], H[100 + lo], the blinding term on rank 0 alone;
    the phase-1 commitments and A_O2 stay window-sharded.  Both ranks emit the proof of an unsharded ctx with the same knobs, and
    that proof is the CPU oracle's (the oracle proves N = 8192 in 7 to 8 s on a CPU-only machine, less on the GPU host).  Whether
    the fixed-base schedule itself accepts at this size is not asserted (tests/test_gpu_prove.py documents that it may decline): the
    block partition is what this leg checks.  The one leg that takes more than a second: 3.6 s on the MI355X, generators, fixed-base
    rows and the oracle's proof included."""
    curve, world = 0, 2
    O = oracle
    F = GD.Field(O, curve)
    words = words_b(O, curve)

    def oracle_proof():
        p = O.ProverCS(curve, b"ShardedLegB")
        p.start()
        p.commit([F.w(77)], [F.w(99)])
        program_b(p, F, words, False)
        return p.prove(B_GENS, bytes([0xB3]) * 32)

    single = E.Engine(curve=curve, device=0)
    try:
        single.gens_derive(B_GENS)
        assert single.gens_msm_tables(B_GENS) > 0
        knobs = {TUNE_MSM_FIXED_MIN: 4096, TUNE_DIRECT_MAX: 0}
        for k, v in knobs.items():
            single.set_tuning(k, v)
        want = prove_b(E, single, F, words)
        assert padded_from_proof(want) == B_GENS
        assert want == oracle_proof(), "the unsharded proof differs from the oracle's"

        def body(rank, e):
            proof, log = span(e, lambda: prove_b(E, e, F, words))
            assert proof == want, "rank %d: proof bytes differ from the unsharded ctx's" % rank
            assert e.msm_stats()[1] >= 0
            return log

        res = SC.run_ranks(world, curve, body, knobs=knobs, share_from=single)
        log = same_on_all_ranks(res)
        assert SC.vectors(log) == 1, "the index-cyclic argument was not taken"
        # one point-reduce per MSM: the six commitments (A_I, A_O, S of both phases) and L, R of each of the 11 partitioned rounds
        # (8192 -> 4 elements, gathered at BP_TUNE_IPA_FREEZE_LEN = 4), all before the gather; the frozen tail runs replicated
        gather_at = log.index([x for x in log if x[0] == "vector"][0])
        assert SC.points(log[:gather_at]) == 6 + 2 * 11, log
    finally:
        single.close()


# ---- C. like-provers ----------------------------------------------------------------------------------------------------------------------
SPECS_C = [(("single", 12, 71), [20, 21, 22]), (("shuffle", 9), [20, 21, 22]), (("program2", 9, 72), [11, 11, 11])]
# (program2's randomized callbacks are shared with the recording and hold the source's witness: its like-provers hold that witness
# too and differ in their rng bytes)


def like_run(E, eng, F, curve, specs, refs):
    """3 like-provers per spec on eng against the oracle's proofs; returns the collectives made, when eng is a rank"""
    logs = []
    for (spec, seeds), want in zip(specs, refs):
        src = LC.record(E, curve, F, spec, 11)
        for j, ws in enumerate(seeds):
            lk = LC.like(E, src, LC.record(E, curve, F, spec, ws))
            at = len(getattr(eng, "shard_log", []))
            proof = lk.p.prove(eng, LC.rng(700 + j))
            assert proof == want[j], "%r witness %d: the like-prover's proof differs from the oracle's" % (spec, j)
            logs.append(list(getattr(eng, "shard_log", []))[at:])
    return logs


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_c_like_provers(E, oracle, curve, world):
    """csrc/r1cs_host.inc:890: a like-prover's resident constraint index is off on a sharded ctx (include/arkbp.h: "On a sharded ctx
    nothing is kept resident") — it stages the index per proof.  Three witnesses of one recording, single-phase, the 9-shuffle and a
    two-phase program: every rank's proofs are the oracle's; bp_ctx_prover_like_stats counts no upload, no hit and no resident byte,
    and the gate counters move as on an unsharded ctx."""
    F = GD.Field(oracle, curve)
    refs = cached(("C", curve), lambda: [[LC.oracle_proof(oracle, curve, F, spec, ws, GENS, LC.rng(700 + j)) for j, ws in enumerate(seeds)] for spec, seeds in SPECS_C])

    def unsharded():
        e = E.Engine(curve=curve, device=0)
        try:
            e.gens_derive(GENS)
            like_run(E, e, F, curve, SPECS_C, refs)
            return e.prover_like_stats()
        finally:
            e.close()

    plain = cached(("C-stats", curve), unsharded)
    # what the sharded ctx must NOT do happens here: the single-phase recording's index goes up once and serves two more proofs (its
    # bytes have left again: the recordings are freed).  36 = 3 x 12 products by the gate kernel, 27 = 3 x 9 on the host (two-phase)
    assert plain == (1, 2, 0, 36, 27), plain

    def body(rank, e):
        logs = like_run(E, e, F, curve, SPECS_C, refs)
        for log in logs:
            assert_proof_path(log, world)
        return e.prover_like_stats()

    stats = same_on_all_ranks(SC.run_ranks(world, curve, body, GENS))
    assert stats == (0, 0, 0) + plain[3:], (stats, plain)


# ---- D. witness from device memory ---------------------------------------------------------------------------------------------------------
RANGE_VALUES = [0x0123456789ABCDEF, (1 << 64) - 1]


def range_prover(E, curve, F, values, nbits=64):
    r = LC.Rec()
    r.t = LC.transcript(E)
    r.p = E.ProverCS(curve, r.t)
    r.v, r.b = [F.w(v) for v in values], [F.w(900 + 7 * j) for j in range(len(values))]
    r.V, vars_ = r.p.commit(r.v, r.b)
    for var, v in zip(vars_, values):
        WD.range_gadget(r.p, F, var, v, nbits)
    r.spec = ("range", len(values))
    return r


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_d_witness_from_device_memory(E, oracle, curve, world):
    """csrc/r1cs_host.inc:1144: a device-held witness (bp_prover_assign_multipliers_dev) is taken to the host when shard_world > 1.
    A 33-multiplier program and a 2 x 64-bit range statement built by bp_witness_range_bits_dev: proofs equal the host-assigned
    like-prover's (and the oracle's / the self-recorded prover's); bp_ctx_witness_dev_stats counts the multipliers as downloaded,
    none as imported; a word >= r is refused on every rank alike, the same index named, before any collective."""
    F = GD.Field(oracle, curve)
    spec = ("single", 33, 73)
    ref = cached(("D", curve), lambda: LC.oracle_proof(oracle, curve, F, spec, 23, GENS, LC.rng(710)))

    def body(rank, e):
        src, tw = LC.record(E, curve, F, spec, 11), LC.record(E, curve, F, spec, 23)
        want = LC.like(E, src, tw).p.prove(e, LC.rng(710))
        assert want == ref
        s0 = e.witness_dev_stats()
        lk = WD.dev_like(E, e, src, tw)
        got, log = span(e, lambda: lk.p.prove(e, LC.rng(710)))
        assert got == want, "rank %d: the device-assigned like-prover's proof differs from the host-assigned one's" % rank
        assert_proof_path(log, world)
        assert WD.delta(e, s0) == (1, 0, 33), "one assignment, nothing imported on the device, every multiplier downloaded"
        # a word at or above r
        bad = tw.left.copy()
        bad[5] = WD.raw_words(F.p)
        lk2 = LC.like(E, src, tw, assign=False)
        bl, br = e.upload_scalars(bad), e.upload_scalars(tw.right)
        before = len(e.shard_log)
        try:
            with pytest.raises(E.ArkbpError) as ei:
                lk2.p.assign_multipliers_dev(e, bl, br, 33)
            refusal = (ei.value.code, "left[5]" in str(ei.value))
        finally:
            bl.free()
            br.free()
        assert refusal == (E_ARG, True), str(ei.value)
        assert len(e.shard_log) == before, "a refused assignment made a collective"
        assert WD.delta(e, s0) == (1, 0, 33)
        # the range statement: 2 x 64 bits, the witness built on the GPU
        rsrc = range_prover(E, curve, F, [1, 2])
        rtw = range_prover(E, curve, F, RANGE_VALUES)
        left, right = WD.expected_bits(F, RANGE_VALUES, 64)
        rwant = LC.like(E, rsrc, rtw, left=left, right=right).p.prove(e, LC.rng(711))
        rlk = LC.like(E, rsrc, rtw, assign=False)
        dl, dr = e.witness_range_bits(RANGE_VALUES, 64)
        try:
            rlk.p.assign_multipliers_dev(e, dl, dr, 128)
        finally:
            dl.free()
            dr.free()
        rgot, rlog = span(e, lambda: rlk.p.prove(e, LC.rng(711)))
        assert rgot == rwant == rtw.p.prove(e, LC.rng(711)), "rank %d: the range statement" % rank
        assert_proof_path(rlog, world)
        assert WD.delta(e, s0) == (2, 0, 33 + 128)
        return refusal, rlog

    res = SC.run_ranks(world, curve, body, GENS)
    same_on_all_ranks([r[0] for r in res])


# ---- E. blinding vectors from a key ---------------------------------------------------------------------------------------------------------
CASES_E = [(81, dict(n_mul=20, n_alloc=2, n_extra=4), False), (82, dict(n_mul=9, n_alloc=1, n_extra=2, n_mul2=5), True)]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_e_blinding_vectors_from_a_key(E, oracle, singles, curve, world):
    """bp_prover_set_blinding(BP_BLINDING_EXPANDED) has no shard branch of its own: the GPU-expanded s_L, s_R feed the sharded S
    commitments and the cyclic argument.  Every rank's proof is the unsharded ctx's in the same mode (tests/test_gpu_blinding.py ties
    that to the host model), single- and two-phase, and differs from the default mode's."""
    F = GD.Field(oracle, curve)
    want = cached(("E", curve), lambda: [recorder_prove(E, singles[curve], F, s, 9, two, kw, blinding=E.BLINDING_EXPANDED)[0] for s, kw, two in CASES_E])
    default = cached(("E-default", curve), lambda: [CS.oracle_prove(oracle, curve, F, s, 9, 3, two, **kw)[0] for s, kw, two in CASES_E])

    def body(rank, e):
        for (s, kw, two), w, d in zip(CASES_E, want, default):
            b0 = e.blinding_stats()
            (proof, V, pubs), log = span(e, lambda: recorder_prove(E, e, F, s, 9, two, kw, blinding=E.BLINDING_EXPANDED))
            assert proof == w, "rank %d: the expanded-mode proof differs from the unsharded ctx's" % rank
            assert proof != d and len(proof) == len(d)
            assert e.blinding_stats()[0] > b0[0], "the expansion kernel did not run"
            assert_proof_path(log, world)
            assert CS.product_verifier(E, curve, F, s, V, pubs, two, **kw).verify(e, proof) == OK
            assert recorder_prove(E, e, F, s, 9, two, kw)[0] == d      # the default mode on the same ctx: the oracle's bytes
        return True

    SC.run_ranks(world, curve, body, GENS)


# ---- F. caller-installed Pedersen generators ---------------------------------------------------------------------------------------------
SCENARIOS_F = [(3, [100, 0], 8), (0, [7], 16)]
SEED_F = bytes(range(32))
CASE_F = (83, dict(n_mul=9, n_alloc=1, n_extra=2, n_mul2=5), True)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_f_caller_installed_pedersen_generators(E, oracle, curve, world):
    """bp_pedersen_gens_install has no shard branch of its own: the installed pair feeds the sharded commitments' blinding term and
    the cyclic argument's Q = w * B.  Installed on every rank before sharding is enabled: prove_scenario and ProverCS.prove equal the
    unsharded ctx's bytes under the same pair, every rank's verifier accepts, and a sharded ctx with the DEFAULT pair rejects with -4."""
    F = GD.Field(oracle, curve)
    chain = PG.pair(curve, "chain")
    s, kw, two = CASE_F

    def unsharded():
        e = E.Engine(curve=curve, device=0)
        try:
            e.gens_derive(GENS)
            e.pedersen_gens_install(*chain)
            return [e.prove_scenario(sc, prm, SEED_F, m_cap=mc) for sc, prm, mc in SCENARIOS_F], recorder_prove(E, e, F, s, 9, two, kw, pc_gens=chain)
        finally:
            e.close()

    want_sc, (want_cs, V_cs, pubs_cs) = cached(("F", curve), unsharded)

    def body(rank, e):
        assert not e.pedersen_gens()[2]
        for (sc, prm, mc), w in zip(SCENARIOS_F, want_sc):
            pr, log = span(e, lambda: e.prove_scenario(sc, prm, SEED_F, m_cap=mc))
            assert pr.proof == w.proof and (pr.commitments == w.commitments).all(), "rank %d: scenario %d" % (rank, sc)
            assert_proof_path(log, world)
            assert e.verify_scenario(sc, prm, pr.proof, pr.commitments, pr.publics) == OK
        (proof, V, pubs), log = span(e, lambda: recorder_prove(E, e, F, s, 9, two, kw, pc_gens=chain))
        assert proof == want_cs and (V == V_cs).all() and pubs == pubs_cs
        assert_proof_path(log, world)
        assert CS.product_verifier(E, curve, F, s, V, pubs, two, **kw).verify(e, proof) == OK
        return True

    SC.run_ranks(world, curve, body, GENS, setup=lambda rank, e: e.pedersen_gens_install(*chain))

    def default_pair(rank, e):
        assert e.pedersen_gens()[2]
        out = []
        for (sc, prm, mc), w in zip(SCENARIOS_F, want_sc):
            rc, log = span(e, lambda: e.verify_scenario(sc, prm, w.proof, w.commitments, w.publics))
            assert SC.points(log) >= 1
            out.append(rc)
        out.append(CS.product_verifier(E, curve, F, s, V_cs, pubs_cs, two, **kw).verify(e, want_cs))
        return out

    assert same_on_all_ranks(SC.run_ranks(world, curve, default_pair, GENS)) == [E_VERIFICATION] * 3


# ---- G. witness check and guard ------------------------------------------------------------------------------------------------------------
CASE_G = (84, dict(n_mul=9, n_alloc=1, n_extra=2, n_mul2=5))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_g_witness_check_and_guard(E, oracle, singles, curve, world):
    """csrc/r1cs_host.inc:1195 (the guard's shared row index is not made resident on a sharded ctx) and the sharded witness check of
    DESIGN.md section 5: ProverCS.check on a sharded ctx returns the host twin's report; with the guard on a satisfiable statement
    proves to the same bytes; the 4-shuffle that is no permutation and a poked gate are refused with BP_E_UNSATISFIED and the same
    bp_ctx_last_unsatisfied report on every rank, the ranks' collectives of the refused proofs identical; the same ctxs then prove a
    valid statement to the oracle's bytes — a refused proof leaves no rank out of step."""
    from ark_bulletproofs_amd import UnsatisfiedError

    F = GD.Field(oracle, curve)
    s, kw = CASE_G
    rng = bytes([9]) * 32
    plain = cached(("G", curve), lambda: [W.random_prover(E, curve, F, s, 8, two, **kw)[0].prove(singles[curve], rng) for two in (False, True)])
    valid = cached(("G-valid", curve), lambda: [CS.oracle_prove(oracle, curve, F, s, 5, 3, two, **kw) for two in (False, True)])
    like_src = cached(("G-like", curve), lambda: LC.oracle_proof(oracle, curve, F, ("single", 12, 71), 20, GENS, LC.rng(720)))

    def refused(e, p):
        p.set_check(True)
        at = len(e.shard_log)
        with pytest.raises(UnsatisfiedError) as ei:
            p.prove(e, rng)
        assert ei.value.code == E_UNSATISFIED
        (inst, rep), = e.last_unsatisfied()
        assert inst == 0
        return rep, list(e.shard_log[at:])

    def body(rank, e):
        out = []
        for k, two in enumerate((False, True)):
            p, m, V, pubs = W.random_prover(E, curve, F, s, 8, two, **kw)
            rep, log = span(e, lambda: p.check(e))
            assert W.observed(F, rep) == m.expect(1 if two else 0) and rep.satisfied
            out.append(("check", rep.astuple(), log))
            W.poke(E, p, m, 3, 1, m.val[(0, 1)] + 1)
            W.poke(E, p, m, 1, 4, m.val[(2, 4)] + 1)
            rep = p.check(e)
            assert W.observed(F, rep) == m.expect(1 if two else 0) and rep.bad_gates == 1 and rep.bad_constraints >= 1
            assert rep == p.check()
            # the guard on a satisfiable statement
            p, m, V, pubs = W.random_prover(E, curve, F, s, 8, two, **kw)
            p.set_check(True)
            proof, log = span(e, lambda: p.prove(e, rng))
            assert proof == plain[k], "rank %d: the guarded proof differs from the unguarded unsharded one" % rank
            assert e.last_unsatisfied() == []
            assert_proof_path(log, world)
        # a like-prover under the guard: the shared row index, not resident here
        src = LC.record(E, curve, F, ("single", 12, 71), 11)
        lk = LC.like(E, src, LC.record(E, curve, F, ("single", 12, 71), 20))
        lk.p.set_check(True)
        assert lk.p.prove(e, LC.rng(720)) == like_src
        assert e.prover_like_stats()[:3] == (0, 0, 0)
        # refused: only phase-2 rows violated (the shuffle), then a gate
        p, m, V = W.shuffle_prover(E, curve, F, 4, permuted=False)
        rep, log = refused(e, p)
        exp = m.expect(0)
        assert W.observed(F, rep) == exp and exp[2] == 0 and exp[4] == 1
        out.append(("shuffle", rep.astuple(), log))
        p, m, V, pubs = W.random_prover(E, curve, F, s, 8, False, **kw)
        W.poke(E, p, m, 0, 0, m.val[(1, 0)] + 1)
        rep, log = refused(e, p)
        assert W.observed(F, rep) == m.expect(0) and rep.bad_gates == 1 and rep.first_bad_gate == 0
        out.append(("gate", rep.astuple(), log))
        # the same ctxs, a valid statement, the oracle's bytes
        for two, (ref, Vo, pubs_o) in zip((False, True), valid):
            (proof, V, pubs), log = span(e, lambda: CS.product_prove(E, e, F, s, 5, 3, two, **kw))
            assert proof == ref, "rank %d: after the refused proofs" % rank
            assert_proof_path(log, world)
            assert CS.product_verifier(E, curve, F, s, V, pubs, two, **kw).verify(e, proof) == OK
        assert e.last_unsatisfied() == []
        return out

    same_on_all_ranks(SC.run_ranks(world, curve, body, GENS))


# ---- H. batch entry points of the prover ---------------------------------------------------------------------------------------------------
SPEC_H = ("single", 12, 74)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_h_prover_batch_entry_points(E, oracle, curve, world):
    """csrc/prove_batch.inc:682: front groups are off on a sharded ctx (include/arkbp.h: an instance runs every stage in a group only
    on a ctx that is not sharded).  bp_prover_commit_batch and bp_prover_prove_batch of 5 like-instances: every proof is the oracle's,
    bp_ctx_prove_batch_front_stats shows no front group; one instance with a bad witness and the guard on fails alone with
    BP_E_UNSATISFIED on every rank alike; bp_prover_check_batch equals the single checks."""
    F = GD.Field(oracle, curve)
    rngs = [LC.rng(730 + j) for j in range(5)]
    refs = cached(("H", curve), lambda: [LC.oracle_proof(oracle, curve, F, SPEC_H, 30 + j, GENS, rngs[j]) for j in range(5)])

    def members(e, src, twins, guard=False, bad=None):
        ps = [src.p.new_like(LC.transcript(E)) for _ in twins]
        res, log = span(e, lambda: e.prover_commit_batch(ps, [tw.v for tw in twins], [tw.b for tw in twins]))
        for (V, _), tw in zip(res, twins):
            assert (V == tw.V).all(), "bp_prover_commit_batch: a commitment differs from the host's"
        for j, (p, tw) in enumerate(zip(ps, twins)):
            right = tw.right
            if j == bad:
                right = tw.right.copy()
                right[11] = F.w(F.i(right[11]) + 5)
            p.assign_multipliers(tw.left, right)
            if guard:
                p.set_check(True)
        return ps, log

    def body(rank, e):
        src = LC.record(E, curve, F, SPEC_H, 11)
        twins = [LC.record(E, curve, F, SPEC_H, 30 + j) for j in range(5)]
        ps, commit_log = members(e, src, twins)
        (rc, res), log = span(e, lambda: e.prove_batch(ps, rngs, return_rc=True))
        assert rc == OK and [st for st, _ in res] == [OK] * 5
        assert [pf for _, pf in res] == refs, "rank %d: prove_batch differs from the oracle's proofs" % rank
        assert_proof_path(log, world, proofs=5)
        assert e.prove_batch_front_stats()[:2] == (0, 0), "a front group ran on a sharded ctx"
        # one bad witness, all guarded
        ps, _ = members(e, src, twins, guard=True, bad=2)
        (rc, res), bad_log = span(e, lambda: e.prove_batch(ps, rngs, return_rc=True))
        assert rc == E_UNSATISFIED and [st for st, _ in res] == [OK, OK, E_UNSATISFIED, OK, OK]
        assert res[2][1] == b"" and [res[j][1] for j in (0, 1, 3, 4)] == [refs[j] for j in (0, 1, 3, 4)]
        (inst, rep), = e.last_unsatisfied()
        assert inst == 2 and rep.bad_gates == 0 and rep.bad_constraints >= 1
        assert e.prove_batch_front_stats()[:2] == (0, 0)
        # check_batch
        run = [W.random_prover(E, curve, F, 50 + j, 60 + j, two, **kw)[:2] for j, (kw, two) in enumerate([(dict(n_mul=6, n_alloc=1, n_extra=2, n_mul2=5), True), (dict(n_mul=10, n_alloc=3, n_extra=6), False), (dict(n_mul=40, n_alloc=3, n_extra=6), False)])]
        W.poke(E, run[1][0], run[1][1], 0, 0, run[1][1].val[(1, 0)] + 1)
        got, check_log = span(e, lambda: e.check_batch([p for p, _ in run]))
        assert got == [p.check(e) for p, _ in run]
        assert [W.observed(F, r) for r in got] == [m.expect(1 if j == 0 else 0) for j, (_, m) in enumerate(run)]
        assert [r.satisfied for r in got] == [True, False, True]
        return commit_log, bad_log, rep.astuple(), check_log

    same_on_all_ranks(SC.run_ranks(world, curve, body, GENS))


# ---- I. verification entry points ------------------------------------------------------------------------------------------------------------
SC_MULTI_RANGE = 4
COUNT_I, BAD_I = 9, (2, 7)
SEED_I = bytes([0x42]) * 32
EXPECT_I = [E_VERIFICATION if j in BAD_I else OK for j in range(COUNT_I)]


def scenario_pool(O, curve):
    def make():
        good = []
        for j in range(COUNT_I):
            pr = O.r1cs_prove(curve, SC_MULTI_RANGE, [3, 8, 0], bytes([30 + j]) * 32, GENS, m_cap=8)
            good.append((SC_MULTI_RANGE, [3, 8, 0], pr.proof, pr.commitments, pr.publics))
        bad = [BR.defective(i, j, O, curve) if j in BAD_I else i for j, i in enumerate(good)]
        ref = BR.BatchRef(O, curve, GENS)
        al = ref.alphas(SEED_I, COUNT_I)
        return good, bad, ref.point(ref.units(bad), al), al

    return cached(("I-sc", curve), make)


def recorded_pool(O, curve, F, two_phase):
    def make():
        items = CW.prove_items(O, curve, F, COUNT_I, 2, two_phase)
        proofs = [BR.defect_proof(p, j) if j in BAD_I else p for j, (p, _) in enumerate(items)]
        Vs = [V for _, V in items]
        ref = BR.BatchRef(O, curve, CW.GENS)
        al = O.fe_rand(O.fid(curve, True), bytes([0x43]) * 32, COUNT_I)

        def one(j):
            v = O.VerifierCS(curve, CW.LABEL)
            v.start()
            GD.random_program(v, F, 41, None, v.commit(Vs[j]), two_phase=two_phase, publics=[], **CW.KW)
            return v, proofs[j]

        units = ref.units_cs([("sharded-I", two_phase, j) for j in range(COUNT_I)], one)
        return proofs, Vs, al, ref.point(units, al)

    return cached(("I-cs", curve, two_phase), make)


def verify_run(E, O, eng, curve, F):
    """every verification entry point on eng (a rank, or the unsharded ctx with BP_TUNE_VFY_DEVICE = 0): what it returned"""
    good, bad, _, _ = scenario_pool(O, curve)
    out = {}
    v0 = eng.vfe_stats()
    rc, _, pt = eng.batch_verify(good, SEED_I, want_point=True)
    out["batch valid"] = (rc, pt.tolist())
    rc, _, pt = eng.batch_verify(bad, SEED_I, want_point=True)
    out["batch"] = (rc, pt.tolist())
    out["each"] = eng.verify_each_scenarios(bad)
    out["locate"] = eng.batch_verify_locate(bad, SEED_I)
    for two in (False, True):
        proofs, Vs, al, _ = recorded_pool(O, curve, F, two)
        for wired in (False, True):
            rc, pt = E.batch_verify_cs(eng, CW.verifiers(E, O, curve, F, Vs, two, wired), proofs, al, want_point=True)
            out["cs batch", two, wired] = (rc, pt.tolist())
        out["cs each", two] = eng.verify_each(CW.verifiers(E, O, curve, F, Vs, two, False), proofs)
        out["cs locate", two] = E.batch_verify_locate_cs(eng, CW.verifiers(E, O, curve, F, Vs, two, True), proofs, al)
    out["vfe"] = tuple(a - b for a, b in zip(eng.vfe_stats(), v0))
    return out


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_i_verification_entry_points(E, oracle, curve, world):
    """csrc/r1cs_host.inc:1970 (the device front end is off: include/arkbp.h "A sharded ctx ... keep the host replay"),
    csrc/verify_each.inc:181 (no direct-table reach: every instance of bp_verifier_verify_batch takes the single route) and
    bp_r1cs_batch_verify_locate on a sharded ctx.  Nine instances of the multi-range scenario [3, 8, 0], and nine like-instances of
    one recorded gadget (single- and two-phase, affine and deferred wire commitments), instances 2 and 7 defective: status and check
    point of the batch equal the unsharded ctx's with BP_TUNE_VFY_DEVICE = 0 and batchref's sum of unit points, the verdicts per
    instance equal the unsharded ctx's and name 2 and 7, bp_ctx_vfe_stats does not move."""
    O = oracle
    F = GD.Field(O, curve)
    _, _, point_sc, _ = scenario_pool(O, curve)

    def unsharded():
        e = E.Engine(curve=curve, device=0)
        try:
            e.gens_derive(GENS)
            e.set_tuning(TUNE_VFY_DEVICE, 0)
            return verify_run(E, O, e, curve, F)
        finally:
            e.close()

    want = cached(("I", curve), unsharded)
    # the unsharded ctx against the CPU references first
    assert want["batch valid"] == (OK, [0] * 8)
    assert want["batch"] == (E_VERIFICATION, point_sc.tolist())
    assert want["each"] == (E_VERIFICATION, EXPECT_I) and want["locate"] == (E_VERIFICATION, EXPECT_I)
    for two in (False, True):
        point_cs = recorded_pool(O, curve, F, two)[3]
        assert want["cs batch", two, False] == want["cs batch", two, True] == (E_VERIFICATION, point_cs.tolist())
        assert want["cs each", two] == (E_VERIFICATION, EXPECT_I) and want["cs locate", two] == (E_VERIFICATION, EXPECT_I)
    assert want["vfe"] == (0, 0)

    def body(rank, e):
        got, log = span(e, lambda: verify_run(E, O, e, curve, F))
        for key in want:
            assert got[key] == want[key], "rank %d: %r: %r, unsharded %r" % (rank, key, got[key], want[key])
        assert SC.points(log) >= 1 and SC.vectors(log) == 0, log
        return log

    same_on_all_ranks(SC.run_ranks(world, curve, body, GENS))


# ---- J. stand-alone MSMs ----------------------------------------------------------------------------------------------------------------------
J_GENS = 5008
J_SIZES = [1, 33, 1000, 5000]
J_OFF = 3


def msm_inputs(O, curve):
    """oracle generators as bases; per size n: bases, scalars with the edge cases, and the oracle's results"""
    def make():
        FR = O.fid(curve, True)
        r = O.modulus(FR)
        G, H = O.bp_gens(curve, J_GENS)
        G, H = np.asarray(G, dtype=np.uint64).reshape(-1, 8), np.asarray(H, dtype=np.uint64).reshape(-1, 8)
        extra = np.asarray(O.generator(curve), dtype=np.uint64).reshape(1, 8)
        minus_one = O.fe_from_int(FR, r - 1)

        def oracle_msm(bases, scalars):
            nz = bases.any(axis=1)            # (the identity contributes nothing)
            return np.asarray(O.msm(curve, bases[nz], scalars[nz]), dtype=np.uint64).reshape(8)

        cases = {}
        for n in J_SIZES:
            bases = G[:n].copy()
            sc = O.fe_rand(FR, bytes([0xD0 + (n & 15)]) * 32, 2 * n + 1)
            s = sc[:n].copy()
            if n >= 8:
                s[0], s[1], s[2] = O.fe_from_int(FR, 0), O.fe_from_int(FR, 1), minus_one
                bases[3] = 0                                  # the identity as a base
                bases[5] = bases[4]                           # a duplicated base
                bases[7] = O.scalar_mul(curve, bases[6], minus_one)     # P next to -P with equal scalars
                s[7] = s[6]
            else:
                s[0] = minus_one
            gs = sc[: 2 * n + 1].copy()
            if n >= 8:
                gs[0], gs[n], gs[2 * n] = O.fe_from_int(FR, 0), O.fe_from_int(FR, 1), minus_one
            cases[n] = dict(bases=bases, s=s, msm=oracle_msm(bases, s), gs=gs,
                            gens=oracle_msm(np.concatenate([G[J_OFF:J_OFF + n], H[J_OFF:J_OFF + n], extra]), gs))
        # bp_msm_batch: 6 jobs of 5, 40 and 700 terms — the first three out of the n = 1000 case's terms (scalars 0, 1, r - 1 and the
        # identity base in the first job, the duplicate across the first two, P next to -P in the second), three more of random terms
        pool_b = np.concatenate([cases[1000]["bases"][:745], G[1000:1745]])
        pool_s = np.concatenate([cases[1000]["s"][:745], O.fe_rand(FR, bytes([0xD9]) * 32, 745)])
        jobs, at = [], 0
        for ln in (5, 40, 700, 5, 40, 700):
            jobs.append((pool_b[at:at + ln].copy(), pool_s[at:at + ln].copy()))
            at += ln
        want_jobs = [oracle_msm(b, s) for b, s in jobs]
        v, b = PG.edge_scalars(O, curve, 33, 0xD7)
        commits = np.stack([O.pedersen_commit(curve, v[i], b[i]) for i in range(33)])
        return cases, extra, jobs, want_jobs, (v, b, commits)

    return cached(("J", curve), make)


@pytest.fixture(scope="module")
def wide(E):
    """per curve: an unsharded ctx with 5008 generators, shared by the ranks of leg J"""
    out = {}
    for cv in CURVES:
        e = E.Engine(curve=cv, device=0)
        e.gens_derive(J_GENS)
        out[cv] = e
    yield out
    for e in out.values():
        e.close()


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("curve", CURVES)
def test_j_stand_alone_msms(E, oracle, wide, curve, world):
    """csrc/msm_batch.inc:127-134 (every job of bp_msm_batch takes the single route on a sharded ctx; include/arkbp.h says so) and
    csrc/arkbp.hip:936 (no GLV route there): bp_msm, bp_msm_gens (with an offset and an extra base), bp_msm_batch and
    bp_pedersen_commit_batch called directly on a sharded ctx, 1 to 5000 terms with scalars 0, 1 and r - 1, an identity base, a
    duplicated base and P next to -P.  Every rank gets the oracle's full value, with one point-reduce per MSM;
    bp_pedersen_commit_batch runs on the fixed-base tables of the pair and makes no collective."""
    cases, extra, jobs, want_jobs, (v, b, commits) = msm_inputs(oracle, curve)

    def body(rank, e):
        logs = {}
        for n in J_SIZES:
            c = cases[n]
            got, logs["msm", n] = span(e, lambda: e.msm(c["bases"], c["s"]))
            assert (got == c["msm"]).all(), "rank %d: bp_msm, n = %d" % (rank, n)
            got, logs["gens", n] = span(e, lambda: e.msm_gens(n, c["gs"], off=J_OFF, extra_bases=extra))
            assert (got == c["gens"]).all(), "rank %d: bp_msm_gens, n = %d" % (rank, n)
        s0 = e.msm_batch_stats()
        got, logs["batch"] = span(e, lambda: e.msm_batch(jobs))
        for j in range(6):
            assert (got[j] == want_jobs[j]).all(), "rank %d: bp_msm_batch, job %d" % (rank, j)
        d = tuple(x - y for x, y in zip(e.msm_batch_stats(), s0))
        assert d == (0, 0, 6, 0, 0), d
        got, logs["pedersen"] = span(e, lambda: e.pedersen_commit_batch(v, b))
        assert (got == commits).all(), "rank %d: bp_pedersen_commit_batch" % rank
        return logs

    logs = same_on_all_ranks(SC.run_ranks(world, curve, body, share_from=wide[curve]))
    for n in J_SIZES:
        assert logs["msm", n] == [("point", 8)] and logs["gens", n] == [("point", 8)], (n, logs)
    assert logs["batch"] == [("point", 8)] * 6
    assert logs["pedersen"] == []
