"""The unit-point reference of tests/batchref.py against the oracle's direct batch points (CPU only): for batches of distinct,
defective instances with distinct weights, sum_j alpha_j * U_j equals the mega-check point of batch_verify_point (scenario
statements, single- and two-phase) and of batch_verify_cs (recorded gadgets).  The GPU tests of tests/test_gpu_vfy_every_instance.py
rest on this identity."""
import numpy as np
import pytest

import batchref as BR
import gadgets as GD

SC_SHUFFLE, SC_MULTI_RANGE = 0, 4
GENS = 256
LABEL = b"batchref identity"


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("sc,prm", [(SC_MULTI_RANGE, [2, 8, 0]), (SC_SHUFFLE, [2])])
def test_unit_points_sum_to_the_direct_batch_point(oracle, curve, sc, prm):
    O = oracle
    R = BR.BatchRef(O, curve, GENS)
    base = [O.r1cs_prove(curve, sc, prm, bytes([60 + w]) * 32, GENS) for w in range(3)]
    valid = [(sc, prm, b.proof, b.commitments, b.publics) for b in base]
    count = 24
    inst = [BR.defective(valid[j % 3], j, O, curve) for j in range(count)]
    assert len({BR.scenario_key(i) for i in inst}) == count
    units = R.units(inst)
    assert units.any(axis=1).all(), "a defective instance with an identity unit point"
    assert not R.units(valid).any(), "a valid instance's unit point is not the identity"
    seed = bytes([17]) * 32
    rc, direct = O.batch_verify_point(curve, inst, GENS, seed)
    assert rc == O.E_VERIFICATION
    assert (R.point(units, R.alphas(seed, count)) == np.asarray(direct, dtype=np.uint64).reshape(-1)).all()
    # a batch with valid instances around one defective one: alpha_j * U_j
    mixed = [valid[j % 3] for j in range(count)]
    mixed[13] = inst[13]
    rc, direct = O.batch_verify_point(curve, mixed, GENS, seed)
    assert (R.point(units[13:14], R.alphas(seed, count)[13:14]) == np.asarray(direct, dtype=np.uint64).reshape(-1)).all()
    # an alpha window: the weights of instances 5 .. 5 + count of a longer batch
    al = R.alphas(seed, count, skip=5)
    assert (al == O.fe_rand(O.fid(curve, True), seed, count + 5)[5:]).all()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("two_phase", [False, True])
def test_unit_points_of_recorded_handles(oracle, curve, two_phase):
    O = oracle
    F = GD.Field(O, curve)
    R = BR.BatchRef(O, curve, GENS)
    kw = dict(n_mul=6, n_extra=0, n_alloc=1, n_mul2=3)
    count = 10
    proofs, Vs = [], []
    for w in range(count):
        vals, blinds = GD.make_witness(F, 300 + w, 2)
        p = O.ProverCS(curve, LABEL).start()
        V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
        wit = GD.Witness(F)
        for var, v in zip(vars_, vals):
            wit.val[var] = v
        GD.random_program(p, F, 77, wit, vars_, two_phase=two_phase, **kw)
        proofs.append(BR.defect_proof(p.prove(GENS, bytes([w]) * 32), w))
        Vs.append(BR.defect_commitments(V, w, O, curve))

    def make(j):
        v = O.VerifierCS(curve, LABEL).start()
        GD.random_program(v, F, 77, None, v.commit(Vs[j]), two_phase=two_phase, **kw)
        return v, proofs[j]

    units = R.units_cs([("batchref-cpu", two_phase, j) for j in range(count)], make)
    assert units.any(axis=1).all()
    alphas = O.fe_rand(O.fid(curve, True), bytes([23]) * 32, count)
    rc, direct = O.batch_verify_cs(curve, [make(j)[0] for j in range(count)], proofs, GENS, alphas)
    assert rc == O.E_VERIFICATION
    assert (R.point(units, alphas) == np.asarray(direct, dtype=np.uint64).reshape(-1)).all()
