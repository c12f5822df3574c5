"""Every instance of a batch counts: batch_verify's mega-check point against the unit-point reference (tests/batchref.py,
sum_j alpha_j * U_j from the CPU oracle) for batches of DISTINCT proofs, on both curves, through the device front end
(BP_TUNE_VFY_DEVICE 1 / 2) and the host replay (0).  A valid batch is the identity whatever the verifier does with a valid instance;
all-defective batches and single defects at the block / workgroup boundaries are what see an instance that is dropped, repeated,
weighted with another instance's alpha or evaluated with another instance's data.  Boundaries: 64 proofs per workgroup of
k_vfe_sponge / k_vfe_consts, blocks of VFY_BLOCK = 512, chunks of several proofs in k_vfy_batch, the host pool's ranges, the
template groups (`perm`) of a mixed block, alpha windows of proof-sharded batches.  Each call's path is asserted from vfe_stats()."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import batchref as BR
import gadgets as GD

pytestmark = pytest.mark.gpu
OK, E_VERIFICATION = 0, -4
SC_SHUFFLE, SC_RANGE, SC_MULTI_RANGE = 0, 1, 4
TUNE_HOST_THREADS, TUNE_VFY_DEVICE, TUNE_DIRECT_MAX = 6, 11, 12
GENS = 256
POOL = 1025
COUNTS = [1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025]
SWEEP = [0, 1, 63, 64, 65, 255, 256, 511, 512, 513, 767, 1023, 1024]
# name -> (scenario, params, the device knob that takes it)
STATEMENTS = {"multi-range": (SC_MULTI_RANGE, [2, 8, 0], 1), "range": (SC_RANGE, [16, 1234], 1), "shuffle-2": (SC_SHUFFLE, [2], 2), "shuffle-3": (SC_SHUFFLE, [3], 2)}


def wseed(*tag):
    """a 32-byte witness / prover seed of its own per instance"""
    return hashlib.sha256(repr(tag).encode()).digest()


class Pool:
    """POOL distinct proofs of one statement (proved on the GPU) and their defective copies (batchref.defective at position j)"""

    def __init__(self, O, eng, R, name, count=POOL):
        sc, prm, self.knob = STATEMENTS[name]
        self.name, self.R = name, R
        self.valid = []
        for j in range(count):
            pr = eng.prove_scenario(sc, prm, wseed(eng.curve, name, j))
            self.valid.append((sc, prm, pr.proof, pr.commitments, pr.publics))
        self.bad = [BR.defective(inst, j, O, eng.curve) for j, inst in enumerate(self.valid)]
        self.units = R.units(self.bad)
        assert self.units.any(axis=1).all()
        self.cross_checked = False

    def cross_check(self, O, cv):
        """the reference against ONE direct oracle batch over the whole all-defective pool (once per pool)"""
        if not self.cross_checked:
            seed = bytes([0x77]) * 32
            rc, pt = O.batch_verify_point(cv, self.bad, GENS, seed)
            assert rc == O.E_VERIFICATION
            assert (np.asarray(pt, dtype=np.uint64).reshape(-1) == self.R.point(self.units, self.R.alphas(seed, len(self.bad)))).all(), \
                "the unit-point reference differs from the oracle's direct batch point (%s)" % self.name
            self.cross_checked = True


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def env(request, oracle):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(GENS)
    R = BR.BatchRef(oracle, request.param, GENS)
    pools = {}

    def pool(name):
        if name not in pools:
            pools[name] = Pool(oracle, e, R, name)
        pools[name].cross_check(oracle, request.param)
        return pools[name]

    yield e, R, pool
    e.close()


def run(eng, instances, seed, knob, alpha_skip=0):
    eng.set_tuning(TUNE_VFY_DEVICE, knob)
    try:
        d0, f0 = eng.vfe_stats()
        rc, _, pt = eng.batch_verify(instances, seed, alpha_skip=alpha_skip, want_point=True)
        d1, f1 = eng.vfe_stats()
    finally:
        eng.set_tuning(TUNE_VFY_DEVICE, 1)
    return rc, pt, (d1 - d0, f1 - f0)


def used_for(knob):
    return (1, 0) if knob else (0, 0)


def checked_run(eng, R, instances, units, seed, knob, what):
    """one batch through `knob`; its path asserted; its point against the reference (bisected with alpha windows on a mismatch)"""
    rc, pt, used = run(eng, instances, seed, knob)
    assert used == used_for(knob), "%s: the batch took another path (vfe_stats delta %r)" % (what, used)

    def sub(lo, hi):
        return run(eng, instances[lo:hi], seed, knob, alpha_skip=lo)[1]

    R.check(pt, units, R.alphas(seed, len(instances)), run=sub, what=what)
    return rc, pt


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name", list(STATEMENTS))
def test_all_defective_prefixes(env, name, path):
    """prefixes of one pool of distinct, all-defective proofs: the point is sum_j alpha_j * U_j exactly"""
    eng, R, pool = env
    P = pool(name)
    knob = P.knob if path == "device" else 0
    seed = bytes([0x31]) * 32
    for count in COUNTS:
        rc, pt = checked_run(eng, R, P.bad[:count], P.units[:count], seed, knob, "%s, %s, %d instances" % (name, path, count))
        assert rc == E_VERIFICATION and pt.any()


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name", ["multi-range", "shuffle-2"])
def test_single_defect_sweep(env, name, path):
    """a valid batch of POOL distinct proofs is accepted with the identity; one defect at a boundary position gives alpha_j * U_j.
    The host replay runs on a pool of 7 threads (uneven ranges over the blocks)."""
    eng, R, pool = env
    P = pool(name)
    knob = P.knob if path == "device" else 0
    seed = bytes([0x41]) * 32
    alphas = R.alphas(seed, POOL)
    if path == "host":
        eng.set_tuning(TUNE_HOST_THREADS, 7)
    try:
        rc, pt, used = run(eng, P.valid, seed, knob)
        assert used == used_for(knob) and rc == OK and not pt.any()
        for j in SWEEP:
            inst = list(P.valid)
            inst[j] = P.bad[j]
            rc, pt, used = run(eng, inst, seed, knob)
            assert used == used_for(knob), "defect at %d: the batch took another path" % j
            assert rc == E_VERIFICATION, "defect at %d not seen" % j
            assert (pt == R.point(P.units[j:j + 1], alphas[j:j + 1])).all(), "defect at %d: the point is not alpha_j * U_j" % j
    finally:
        eng.set_tuning(TUNE_HOST_THREADS, 0)


def test_mixed_templates_in_the_host_replay(env):
    """three statements interleaved irregularly inside and across blocks (1100 instances: 512 + 512 + 76), every instance distinct
    and defective: the template groups of a block (`perm`) map back to the right instances and alphas"""
    eng, R, pool = env
    pools = [pool(n) for n in ("multi-range", "range", "shuffle-2")]
    at = [0, 0, 0]
    inst, units = [], []
    for j in range(1100):
        t = (j * 5 + j // 7 + (j * j) % 11) % 3
        inst.append(pools[t].bad[at[t]])
        units.append(pools[t].units[at[t]])
        at[t] += 1
    units = np.stack(units)
    seed = bytes([0x51]) * 32
    for knob in (0, 1):    # (a batch of several statements is no like-instance batch: the host replay either way)
        rc, pt, used = run(eng, inst, seed, knob)
        assert used == (0, 0) and rc == E_VERIFICATION
        R.check(pt, units, R.alphas(seed, len(inst)), what="mixed templates, knob %d" % knob)


@pytest.mark.parametrize("name", ["multi-range", "shuffle-2"])
def test_proof_sharded_windows_on_the_device(env, name):
    """a batch cut into windows that are not block-aligned, each with alpha_skip = its offset: the windows' points sum to the whole
    batch's point, and both equal the reference (the device front end takes every window)"""
    eng, R, pool = env
    P = pool(name)
    seed = bytes([0x61]) * 32
    inst = P.bad
    rc, whole, used = run(eng, inst, seed, P.knob)
    assert used == (1, 0) and rc == E_VERIFICATION
    R.check(whole, P.units, R.alphas(seed, POOL), what="whole batch")
    for cuts in ([0, 300, POOL], [0, 1, 601, POOL], [0, 511, 513, POOL]):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            rc, pt, used = run(eng, inst[lo:hi], seed, P.knob, alpha_skip=lo)
            assert used == (1, 0) and rc == E_VERIFICATION
            R.check(pt, P.units[lo:hi], R.alphas(seed, hi - lo, skip=lo), what="window [%d, %d)" % (lo, hi))
            parts.append(pt)
        from ark_bulletproofs_amd import engine as E

        assert (E.host_points_sum(eng.curve, np.stack(parts)) == whole).all(), "windows %r do not sum to the whole batch" % cuts


# ---- recorded handles (bp_r1cs_batch_verify) with explicit weights --------------------------------------------------------------
CS_LABEL = b"every instance counts"
CS_COUNT = 600


def cs_prove(E, eng, F, program, j, m):
    vals, blinds = GD.make_witness(F, 7000 + j, m)
    p = E.ProverCS(eng.curve, E.HostTranscript(CS_LABEL))
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    program(p, F, wit, vars_)
    return p.prove(eng, wseed("cs", eng.curve, j)), V


def cs_oracle_prove(O, curve, F, program, j, m):
    vals, blinds = GD.make_witness(F, 7000 + j, m)
    p = O.ProverCS(curve, CS_LABEL).start()
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    program(p, F, wit, vars_)
    return p.prove(GENS, wseed("cs", curve, j)), V


def cs_verifiers(E, curve, F, program, Vs):
    """one recorded verifier + like-instances (their own transcripts and commitments)"""
    v0 = E.VerifierCS(curve, E.HostTranscript(CS_LABEL))
    program(v0, F, None, v0.commit(Vs[0]))
    out = [v0]
    for V in Vs[1:]:
        v = E.VerifierCS(curve, E.HostTranscript(CS_LABEL), like=v0)
        v.commit(V)
        out.append(v)
    return out


def cs_oracle_verifier(O, curve, F, program, V):
    v = O.VerifierCS(curve, CS_LABEL).start()
    program(v, F, None, v.commit(V))
    return v


def random_gadget(two_phase):
    kw = dict(n_mul=7, n_extra=0, n_alloc=1, n_mul2=3)     # (no public constants: every witness is a like-instance)
    return lambda cs, F, wit, vars_: GD.random_program(cs, F, 91, wit, vars_, two_phase=two_phase, **kw)


def cs_batch(E, O, eng, R, program, tag, count, m):
    """count distinct, all-defective like-instances: (proofs, commitments, unit points)"""
    F = GD.Field(O, eng.curve)
    proofs, Vs = [], []
    for j in range(count):
        pr, V = cs_prove(E, eng, F, program, j, m)
        proofs.append(BR.defect_proof(pr, j))
        Vs.append(BR.defect_commitments(V, j, O, eng.curve))
    units = R.units_cs([(tag, j) for j in range(count)], lambda j: (cs_oracle_verifier(O, eng.curve, F, program, Vs[j]), proofs[j]))
    assert units.any(axis=1).all()
    return F, proofs, Vs, units


@pytest.mark.parametrize("two_phase", [False, True], ids=["one-phase", "two-phase"])
def test_recorded_handles_with_explicit_alphas(env, oracle, two_phase):
    from ark_bulletproofs_amd import engine as E

    eng, R, _ = env
    O = oracle
    program = random_gadget(two_phase)
    F, proofs, Vs, units = cs_batch(E, O, eng, R, program, ("random", two_phase), CS_COUNT, 2)
    alphas = O.fe_rand(O.fid(eng.curve, True), bytes([0x71]) * 32, CS_COUNT)
    # the reference once against the oracle's direct batch over the whole batch
    rc_o, pt_o = O.batch_verify_cs(eng.curve, [cs_oracle_verifier(O, eng.curve, F, program, V) for V in Vs], proofs, GENS, alphas)
    assert rc_o == O.E_VERIFICATION and (np.asarray(pt_o, dtype=np.uint64).reshape(-1) == R.point(units, alphas)).all()
    for knob in ((2, 0) if two_phase else (1, 0)):
        eng.set_tuning(TUNE_VFY_DEVICE, knob)
        try:
            d0, f0 = eng.vfe_stats()
            rc, pt = E.batch_verify_cs(eng, cs_verifiers(E, eng.curve, F, program, Vs), proofs, alphas, want_point=True)
            d1, f1 = eng.vfe_stats()
        finally:
            eng.set_tuning(TUNE_VFY_DEVICE, 1)
        assert (d1 - d0, f1 - f0) == used_for(knob)
        assert rc == E_VERIFICATION
        R.check(pt, units, alphas, what="recorded handles, knob %d" % knob)


# ---- k_vfy_batch with several proofs per chunk (ARKBP_VFY_WGS = 256 in a process of its own) ---------------------------------
CHUNK_STMT = (SC_MULTI_RANGE, [16, 64, 0])    # 1024 multipliers: 4 workgroups per proof, 64 chunks


def _chunks_child(curve):
    """449 proofs in one block: chunks of 8, the last one holding one proof; 513: a full block of 64 chunks of 8, then a block of
    one.  All-defective and valid batches through the device front end and the host replay."""
    import ark_bulletproofs_amd as A
    from oracle import pyoracle as O

    O.lib()
    assert os.environ.get("ARKBP_VFY_WGS") == "256"
    eng = A.Engine(curve=curve)
    eng.gens_derive(1024)
    R = BR.BatchRef(O, curve, 1024)
    sc, prm = CHUNK_STMT
    valid = []
    for j in range(513):
        pr = eng.prove_scenario(sc, prm, wseed("chunks", curve, j))
        valid.append((sc, prm, pr.proof, pr.commitments, pr.publics))
    bad = [BR.defective(inst, j, O, curve) for j, inst in enumerate(valid)]
    units = R.units(bad)
    seed = bytes([0x81]) * 32
    rc, pt = O.batch_verify_point(curve, bad[:100], 1024, seed)     # (the reference once against the oracle's direct batch)
    assert rc == O.E_VERIFICATION and (np.asarray(pt, dtype=np.uint64).reshape(-1) == R.point(units[:100], R.alphas(seed, 100))).all()
    for count in (449, 513):
        for knob in (1, 0):
            rc, pt, used = run(eng, valid[:count], seed, knob)
            assert used == used_for(knob) and rc == OK and not pt.any(), (count, knob)
            rc, pt = checked_run(eng, R, bad[:count], units[:count], seed, knob, "chunks, %d instances, knob %d" % (count, knob))
            assert rc == E_VERIFICATION
    eng.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_chunks_of_several_proofs(curve):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_vfy_every_instance as t; t._chunks_child(%d); print('chunks ok')"
            % (os.path.dirname(here), here, curve))
    env = dict(os.environ, ARKBP_VFY_WGS="256")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "chunks ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- the gadget with the rare shapes (gadgets.rare_shapes_program) -----------------------------------------------------------
def rare_gadget(two_phase, summary=None):
    return lambda cs, F, wit, vars_: GD.rare_shapes_program(cs, F, wit, vars_, two_phase=two_phase, summary=summary)


@pytest.mark.parametrize("two_phase", [False, True], ids=["one-phase", "two-phase"])
def test_rare_shapes_gadget(env, oracle, two_phase):
    from ark_bulletproofs_amd import engine as E

    eng, R, _ = env
    O, cv = oracle, eng.curve
    F = GD.Field(O, cv)
    # the shapes were reached (counted from the recorded terms)
    s = {}
    proof, V = cs_prove(E, eng, F, rare_gadget(two_phase, s), 0, 3)
    cols = s["columns"]
    lanes = [c for c in cols if c[0] >= s["n1"]] if two_phase else cols
    counts = {c[1] for c in lanes}
    assert {0, 6, 7} <= counts and max(counts) >= 20, counts
    assert any(c[1] >= 20 and c[2] == 3 for c in lanes), "no long column spread over W_L, W_R and W_O"
    assert s["constraints"] > 256 and all(any(c[1] >= 7 and q in c[3] for c in cols) for q in (254, 255, 256))
    assert s["constants"] > 2 * s["N"] and s["n"] < s["N"], "need more constant terms than 2N and padding lanes"
    assert s["coefs"] == {"+1", "-1", "general"} and s["twice"] and s["lo_same"] and s["committed_max"] >= 30
    if two_phase:
        assert s["n1"] < s["n"] and s["phase1_constraints"] < s["constraints"]
    # proof bytes equal the oracle's, on direct tables and without them; Verifier::verify accepts
    ref, Vo = cs_oracle_prove(O, cv, F, rare_gadget(two_phase), 0, 3)
    assert (V == Vo).all() and proof == ref, "proof bytes differ from the oracle's Prover"
    eng.set_tuning(TUNE_DIRECT_MAX, 0)
    try:
        assert cs_prove(E, eng, F, rare_gadget(two_phase), 0, 3)[0] == ref, "proof bytes differ without direct tables"
    finally:
        eng.set_tuning(TUNE_DIRECT_MAX, 8192)
    assert cs_verifiers(E, cv, F, rare_gadget(two_phase), [V])[0].verify(eng, proof) == OK
    assert cs_oracle_verifier(O, cv, F, rare_gadget(two_phase), V).verify(GENS, proof) == 0
    # batches of distinct like-instances: accepted through every knob; all-defective: the reference's point
    count = 40
    program = rare_gadget(two_phase)
    good = [cs_prove(E, eng, F, program, j, 3) for j in range(count)]
    proofs, Vs = [g[0] for g in good], [g[1] for g in good]
    _, bproofs, bVs, units = cs_batch(E, O, eng, R, program, ("rare", two_phase), count, 3)
    alphas = O.fe_rand(O.fid(cv, True), bytes([0x91]) * 32, count)
    rc_o, pt_o = O.batch_verify_cs(cv, [cs_oracle_verifier(O, cv, F, program, V) for V in bVs], bproofs, GENS, alphas)
    assert rc_o == O.E_VERIFICATION and (np.asarray(pt_o, dtype=np.uint64).reshape(-1) == R.point(units, alphas)).all()
    for knob in (0, 1, 2):
        device = knob == 2 or (knob == 1 and not two_phase)
        eng.set_tuning(TUNE_VFY_DEVICE, knob)
        try:
            d0, f0 = eng.vfe_stats()
            rc, pt = E.batch_verify_cs(eng, cs_verifiers(E, cv, F, program, Vs), proofs, alphas, want_point=True)
            d1, f1 = eng.vfe_stats()
            rc_b, pt_b = E.batch_verify_cs(eng, cs_verifiers(E, cv, F, program, bVs), bproofs, alphas, want_point=True)
            d2, f2 = eng.vfe_stats()
        finally:
            eng.set_tuning(TUNE_VFY_DEVICE, 1)
        assert (d1 - d0, f1 - f0) == (d2 - d1, f2 - f1) == ((1, 0) if device else (0, 0)), "knob %d took another path" % knob
        assert rc == OK and not pt.any(), "a valid batch of the gadget is rejected (knob %d)" % knob
        assert rc_b == E_VERIFICATION
        R.check(pt_b, units, alphas, what="rare shapes, knob %d" % knob)
