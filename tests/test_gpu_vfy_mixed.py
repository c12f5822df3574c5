"""Batches of several gadgets (include/arkbp.h "Batches of several gadgets", "A reject flag per proof"): one call whose instances
are like-instances of SEVERAL recordings, in arrival order.  The classes large enough (BP_TUNE_VFY_CLASS_MIN) run the device front
end as one launch chain into one pair of accumulators and one MSM, the rest is one host replay, and the check point is the sum of
the two.  Checked: return value and check POINT against the host replay (BP_TUNE_VFY_DEVICE = 0) and the oracle's single MSM, for
valid batches and for a bad proof in every kind of member; the counters that show which path ran; a flagged proof costs a replay of
the flagged instances only, with the reference's error order; recorded handles (affine and pending wire commitments in one call);
the passes of batch_verify_locate.

Shapes (the smallest that separate the cases): A MULTI_RANGE [2, 8, 0] (N = 16, m = 2), B RANGE [16, 99] (N = 16, m = 1: the same N,
another template and tail length), C MULTI_RANGE [3, 8, 0] (N = 32: another N and proof length), D SHUFFLE [4] (two-phase: remainder)."""
import numpy as np
import pytest

import gadgets as GD

pytestmark = pytest.mark.gpu
OK, E_VERIFICATION, E_FORMAT = 0, -4, -6
SC_SHUFFLE, SC_RANGE, SC_MULTI_RANGE = 0, 1, 4
TUNE_VFY_DEVICE, TUNE_VFY_CLASS_MIN = 11, 24
GENS = 256
SHAPES = {"A": (SC_MULTI_RANGE, [2, 8, 0]), "B": (SC_RANGE, [16, 99]), "C": (SC_MULTI_RANGE, [3, 8, 0]), "D": (SC_SHUFFLE, [4])}
# 76 instances: 70 x A (more than one sponge wavefront), 3 x B, 1 x C, 2 x D, interleaved
WHERE = {5: "B", 9: "D", 17: "C", 30: "B", 44: "D", 60: "B"}
LAYOUT = [WHERE.get(i, "A") for i in range(76)]
SEED = bytes([5]) * 32


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def ctx(request):
    """(engine, {shape name: a few distinct proved instances})"""
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(GENS)
    base = {}
    for name, (sc, prm) in SHAPES.items():
        proved = [e.prove_scenario(sc, prm, bytes([50 + i]) * 32, m_cap=64) for i in range(2)]
        base[name] = [(sc, prm, p.proof, p.commitments, p.publics) for p in proved]
    yield e, base
    e.set_tuning(TUNE_VFY_DEVICE, 1)
    e.set_tuning(TUNE_VFY_CLASS_MIN, 0)
    e.close()


def make(base, layout):
    """make_batch's pattern (tests/test_gpu_vfe.py): a few distinct proofs per shape, repeated"""
    seen = {}
    out = []
    for name in layout:
        i = seen.get(name, 0)
        seen[name] = i + 1
        out.append(base[name][i % len(base[name])])
    return out


def first_of(layout, name, skip=0):
    return [i for i, n in enumerate(layout) if n == name][skip]


def wrong_scalar(inst, at):
    s, p, proof, cm, pb = inst[at]
    bad = bytearray(proof); bad[11 * 33 + 40] ^= 2
    out = list(inst); out[at] = (s, p, bytes(bad), cm, pb)
    return out


def run(eng, inst, knob, device=1):
    """(rc, point, vfe_class_stats delta, vfe_stats delta)"""
    eng.set_tuning(TUNE_VFY_DEVICE, device)
    eng.set_tuning(TUNE_VFY_CLASS_MIN, knob)
    c0, v0 = eng.vfe_class_stats(), eng.vfe_stats()
    rc, _, pt = eng.batch_verify(inst, SEED, want_point=True)
    c1, v1 = eng.vfe_class_stats(), eng.vfe_stats()
    eng.set_tuning(TUNE_VFY_DEVICE, 1)
    return rc, pt, tuple(b - a for a, b in zip(c0, c1)), tuple(b - a for a, b in zip(v0, v1))


def test_interleaved_batch_runs_its_classes_on_the_device(ctx):
    eng, base = ctx
    inst = make(base, LAYOUT)
    rc, pt, cls, vfe = run(eng, inst, 1)
    assert cls == (1, 3, 74, 2, 0), "the classes A, B, C did not run on the device (or D did not stay on the host)"
    assert vfe == (0, 0)
    assert rc == OK and not pt.any()
    rc_h, pt_h, cls_h, vfe_h = run(eng, inst, 1, device=0)
    assert (rc_h, cls_h, vfe_h) == (OK, (0,) * 5, (0, 0)) and not pt_h.any()
    # the knob moves classes to the remainder and changes nothing else
    rc, pt, cls, vfe = run(eng, inst, 2)
    assert cls == (1, 2, 73, 3, 0) and rc == OK and not pt.any()
    rc, pt, cls, vfe = run(eng, inst, 4)
    assert cls == (1, 1, 70, 6, 0) and rc == OK and not pt.any()
    rc, pt, cls, vfe = run(eng, inst, 71)
    assert cls == (0,) * 5 and vfe == (0, 0) and rc == OK and not pt.any()
    # a failing batch: the same non-identity point whatever the knob
    bad = wrong_scalar(inst, first_of(LAYOUT, "A", 3))
    pts = [run(eng, bad, knob)[:2] for knob in (1, 2, 4, 71)]
    assert all(rc == E_VERIFICATION for rc, _ in pts) and pts[0][1].any()
    assert all((p == pts[0][1]).all() for _, p in pts)


@pytest.mark.parametrize("member", ["A", "B", "C", "D"])
def test_wrong_scalar_in_each_kind_of_member(ctx, oracle, member):
    eng, base = ctx
    O, cv = oracle, eng.curve
    bad = wrong_scalar(make(base, LAYOUT), first_of(LAYOUT, member, 1 if member in "ABD" else 0))
    rc, pt, cls, _ = run(eng, bad, 1)
    assert cls == (1, 3, 74, 2, 0)
    rc_h, pt_h, _, _ = run(eng, bad, 1, device=0)
    assert rc == E_VERIFICATION and rc_h == E_VERIFICATION
    assert pt.any() and (pt == pt_h).all(), "the sum of the two check points is not the host replay's point"
    rc_o, pt_o = O.batch_verify_point(cv, bad, GENS, SEED)
    assert rc_o != 0 and (np.asarray(pt_o, dtype=np.uint64).reshape(-1) == pt).all(), "check point differs from the oracle's single MSM"


def test_wrong_commitment_in_a_small_class(ctx, oracle):
    eng, base = ctx
    O, cv = oracle, eng.curve
    inst = make(base, LAYOUT)
    at = first_of(LAYOUT, "B", 2)
    cm = np.array(inst[at][3], dtype=np.uint64).reshape(-1, 8).copy()
    cm[0] = O.generator(cv)
    bad = list(inst); bad[at] = inst[at][:3] + (cm, inst[at][4])
    rc, pt, cls, _ = run(eng, bad, 1)
    rc_h, pt_h, _, _ = run(eng, bad, 1, device=0)
    assert cls == (1, 3, 74, 2, 0)
    assert rc == E_VERIFICATION and rc_h == E_VERIFICATION and pt.any() and (pt == pt_h).all()
    rc_o, pt_o = O.batch_verify_point(cv, bad, GENS, SEED)
    assert rc_o != 0 and (np.asarray(pt_o, dtype=np.uint64).reshape(-1) == pt).all()


def test_a_class_that_crosses_a_block(ctx):
    """513 x A + 2 x B: the second block of A holds one proof, B's slots and tails start behind A's"""
    eng, base = ctx
    layout = ["A"] * 515
    layout[100] = layout[514] = "B"      # A's member 512 is instance 513
    inst = make(base, layout)
    rc, pt, cls, vfe = run(eng, inst, 1)
    assert cls == (1, 2, 515, 0, 0) and vfe == (0, 0) and rc == OK and not pt.any()
    at = [i for i, n in enumerate(layout) if n == "A"][512]
    bad = wrong_scalar(inst, at)
    rc, pt, cls, _ = run(eng, bad, 1)
    rc_h, pt_h, _, _ = run(eng, bad, 1, device=0)
    assert cls == (1, 2, 515, 0, 0)
    assert rc == E_VERIFICATION and rc_h == E_VERIFICATION and pt.any() and (pt == pt_h).all()


def identity_T1(inst, at):
    s, p, proof, cm, pb = inst[at]
    bad = bytearray(proof); bad[6 * 33: 7 * 33] = b"\x00" * 32 + b"\x40"
    out = list(inst); out[at] = (s, p, bytes(bad), cm, pb)
    return out


def both_flag_bits(inst, at):
    s, p, proof, cm, pb = inst[at]
    bad = bytearray(proof); bad[32] = 0xC0
    out = list(inst); out[at] = (s, p, bytes(bad), cm, pb)
    return out


def test_flagged_proofs_in_a_like_instance_batch_are_replayed_alone(ctx, oracle):
    eng, base = ctx
    O, cv = oracle, eng.curve
    inst = make(base, ["A"] * 20)
    bad = identity_T1(inst, 7)
    rc, pt, cls, vfe = run(eng, bad, 0)
    assert rc == E_VERIFICATION and O.batch_verify(cv, bad, GENS, SEED) != 0
    assert cls == (0, 0, 0, 0, 1) and vfe == (0, 1)
    bad = both_flag_bits(bad, 12)      # FormatError wins over the earlier VerificationError (from_bytes runs before batch_verify)
    rc, pt, cls, vfe = run(eng, bad, 0)
    assert rc == E_FORMAT
    assert cls == (0, 0, 0, 0, 2) and vfe == (0, 1)
    assert run(eng, bad, 0, device=0)[0] == E_FORMAT


def test_flagged_proofs_on_the_class_path(ctx):
    eng, base = ctx
    inst = make(base, LAYOUT)
    bad = both_flag_bits(identity_T1(inst, first_of(LAYOUT, "A", 2)), first_of(LAYOUT, "B", 1))   # the malformed B member comes later
    rc, pt, cls, vfe = run(eng, bad, 1)
    rc_h = run(eng, bad, 1, device=0)[0]
    assert rc == rc_h == E_FORMAT
    assert cls[0] == 1 and cls[1:3] == (0, 0) and cls[4] == 2 + 2, "replayed: the two flagged instances and the remainder's two"
    assert vfe == (0, 1)
    # the identity alone: VerificationError, as the host replay says
    bad = identity_T1(inst, first_of(LAYOUT, "A", 2))
    rc, _, cls, _ = run(eng, bad, 1)
    assert rc == run(eng, bad, 1, device=0)[0] == E_VERIFICATION and cls[4] == 1 + 2


def test_batch_verify_locate_takes_the_class_path(ctx):
    eng, base = ctx
    inst = make(base, LAYOUT)
    a, c = first_of(LAYOUT, "A", 40), first_of(LAYOUT, "C")
    bad = wrong_scalar(wrong_scalar(inst, a), c)
    want = [E_VERIFICATION if i in (a, c) else OK for i in range(len(inst))]
    eng.set_tuning(TUNE_VFY_CLASS_MIN, 1)
    eng.set_tuning(TUNE_VFY_DEVICE, 0)
    l0 = eng.verify_locate_stats()
    rc_h, st_h = eng.batch_verify_locate(bad, SEED)
    l1 = eng.verify_locate_stats()
    eng.set_tuning(TUNE_VFY_DEVICE, 1)
    c0 = eng.vfe_class_stats()
    rc, st = eng.batch_verify_locate(bad, SEED)
    l2 = eng.verify_locate_stats()
    c1 = eng.vfe_class_stats()
    assert rc == rc_h == E_VERIFICATION and st == want and st_h == want
    assert l2[1] - l1[1] == l1[1] - l0[1], "the planner made another number of passes"
    assert c1[0] - c0[0] >= 1 and c1[1] - c0[1] >= 3 and c1[2] - c0[2] >= 74, "the passes did not use device classes"


KW = dict(n_mul=9, n_extra=1, n_alloc=1)       # 10 multipliers, padded size 16; n_extra = 1: no public constants
LABEL = b"mixed gadgets"


def gadget_items(E, eng, F, struct_seed, m, distinct):
    out = []
    for w in range(distinct):
        vals, blinds = GD.make_witness(F, 700 + w, m)
        p = E.ProverCS(eng.curve, E.HostTranscript(LABEL))
        V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
        wit = GD.Witness(F)
        for var, v in zip(vars_, vals):
            wit.val[var] = v
        pubs = []
        GD.random_program(p, F, struct_seed, wit, vars_, two_phase=False, publics=pubs, **KW)
        assert pubs == []
        out.append((p.prove(eng, bytes([w + 1]) * 32), V))
    return out


def test_recorded_handles_of_two_gadgets_affine_and_wire(ctx, oracle):
    """two gadgets, each with one recorded verifier and its like-instances, interleaved; one class holds affine commitments, the
    other pending wire commitments, which k_vfe_points decodes"""
    from ark_bulletproofs_amd import engine as E

    eng, _ = ctx
    O, cv = oracle, eng.curve
    F = GD.Field(O, cv)
    gad = {"P": (41, 3, False), "Q": (43, 2, True)}        # struct seed, commitments, wire
    items = {g: gadget_items(E, eng, F, s, m, 2) for g, (s, m, _) in gad.items()}
    layout = ["P" if i % 3 else "Q" for i in range(11)]    # 7 x P, 4 x Q
    alphas = O.fe_rand(O.fid(cv, True), bytes([4]) * 32, len(layout))

    def build(bad=None):
        first, vs, ov, pf, seen = {}, [], [], [], {}
        for i, g in enumerate(layout):
            seed, m, wired = gad[g]
            j = seen.get(g, 0); seen[g] = j + 1
            proof, V = items[g][j % 2]
            v = E.VerifierCS(cv, E.HostTranscript(LABEL), like=first.get(g))
            vars_ = v.commit_compressed(b"".join(O.point_ser(cv, p, True) for p in V), defer=True) if wired else v.commit(V)
            if g not in first:
                GD.random_program(v, F, seed, None, vars_, two_phase=False, publics=[], **KW)
                first[g] = v
            o = O.VerifierCS(cv, LABEL)
            o.start()
            GD.random_program(o, F, seed, None, o.commit(V), two_phase=False, publics=[], **KW)
            if bad == i:
                b = bytearray(proof); b[-40] ^= 2; proof = bytes(b)
            vs.append(v); ov.append(o); pf.append(proof)
        return vs, ov, pf

    for bad in (None, 4, 6):      # 4 is a P (affine) member, 6 a Q (wire) member
        eng.set_tuning(TUNE_VFY_CLASS_MIN, 1)
        vs, ov, pf = build(bad)
        c0, w0, v0 = eng.vfe_class_stats(), eng.commit_wire_stats(), eng.vfe_stats()
        rc_d, pt_d = E.batch_verify_cs(eng, vs, pf, alphas, want_point=True)
        c1, w1, v1 = eng.vfe_class_stats(), eng.commit_wire_stats(), eng.vfe_stats()
        assert tuple(b - a for a, b in zip(c0, c1)) == (1, 2, 11, 0, 0) and v1 == v0
        assert tuple(b - a for a, b in zip(w0, w1)) == (4 * 2, 0, 0), "the wire class was not decoded by the front end"
        vs, _, _ = build(bad)
        eng.set_tuning(TUNE_VFY_DEVICE, 0)
        rc_h, pt_h = E.batch_verify_cs(eng, vs, pf, alphas, want_point=True)
        eng.set_tuning(TUNE_VFY_DEVICE, 1)
        rc_o, pt_o = O.batch_verify_cs(cv, ov, pf, GENS, alphas)
        assert rc_d == rc_h == (OK if bad is None else E_VERIFICATION)
        assert (rc_o == 0) == (bad is None)
        assert (pt_d == pt_h).all() and (pt_d == np.asarray(pt_o).reshape(-1)).all() and pt_d.any() == (bad is not None)
    # the wire class below the knob: its commitments go through the prologue, for its members only
    eng.set_tuning(TUNE_VFY_CLASS_MIN, 5)
    vs, ov, pf = build(None)
    c0, w0 = eng.vfe_class_stats(), eng.commit_wire_stats()
    rc_d, pt_d = E.batch_verify_cs(eng, vs, pf, alphas, want_point=True)
    c1, w1 = eng.vfe_class_stats(), eng.commit_wire_stats()
    assert rc_d == OK and not pt_d.any()
    assert tuple(b - a for a, b in zip(c0, c1)) == (1, 1, 7, 4, 0) and tuple(b - a for a, b in zip(w0, w1)) == (0, 4 * 2, 0)
