"""Shared by test_prover_like_cpu.py and test_gpu_prover_like.py (include/arkbp.h bp_prover_new_like): the gadgets, built with
tests/gadgets.py and mirrored into Python integers by wcheck.Recorder, a prover that records one for itself (the twin every
like-prover is compared with) and a like-prover of a recorded source that holds the same witness.

A spec is ("single", n, seed): a single-phase random program of exactly n multipliers (two rows each) over three commitments and no
public constants, so every witness of it shares one recording; ("public", n, seed): the same with one pinned row and one public
constant, which differs from witness to witness — another recording each; ("program2", n, seed): n phase-1 multipliers and a
randomized phase on top; ("shuffle", k): the reference's k-shuffle, every multiplier and constraint in the randomized phase."""
import numpy as np

import gadgets as GD
import wcheck as W

LABEL = b"ProverLikeTest"


def transcript(E):
    t = E.HostTranscript(LABEL)
    t.append_message(b"dom-sep", b"prover like v1")
    return t


def committed(F, spec, wit_seed):
    """(values, blindings) as ints"""
    if spec[0] == "shuffle":
        k = spec[1]
        ins = [1000 + 17 * i + 1000003 * wit_seed for i in range(k)]
        return ins + ins[1:] + ins[:1], [5 + i + 7 * wit_seed for i in range(2 * k)]
    return GD.make_witness(F, wit_seed, 3)


def run_gadget(cs, F, spec, wit, vars_, publics=None):
    """records spec on cs (a Recorder, a ProverCS, a VerifierCS or an oracle recorder); wit: GD.Witness or None (verifier)"""
    if spec[0] == "shuffle":
        k = spec[1]
        W.shuffle_gadget(cs, F, vars_[:k], vars_[k:])
    elif spec[0] == "single":
        GD.random_program(cs, F, spec[2], wit, vars_, n_mul=spec[1], n_alloc=0, n_extra=0)
    elif spec[0] == "public":
        GD.random_program(cs, F, spec[2], wit, vars_, n_mul=spec[1] - 1, n_alloc=0, n_extra=2, publics=publics)
    else:
        GD.random_program(cs, F, spec[2], wit, vars_, n_mul=spec[1], n_alloc=0, n_extra=0, two_phase=True, n_mul2=3)


class Rec:
    """a prover that recorded spec for itself: p, its transcript t, the Model m, commitments V, what it committed (words), publics, and
    the phase-1 multiplier inputs left / right as (n1, 4) ark words"""


def record(E, curve, F, spec, wit_seed, engine=None, pc_gens=None):
    r = Rec()
    vals, blinds = committed(F, spec, wit_seed)
    r.t = transcript(E)
    r.p = E.ProverCS(curve, r.t, pc_gens=pc_gens)
    r.v, r.b = [F.w(v) for v in vals], [F.w(b) for b in blinds]
    r.V, vars_ = r.p.commit(r.v, r.b, engine=engine)
    r.m = W.Model(F)
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        r.m.val[var] = wit.val[var] = v % F.p
    r.publics = []
    run_gadget(W.Recorder(r.p, r.m), F, spec, wit, vars_, r.publics)
    r.spec, r.n1 = spec, r.p.metrics()[0]
    r.left, r.right = multipliers(F, r.m, r.n1)
    return r


def multipliers(F, m, n):
    """a_L, a_R of multipliers [0, n) from a Model, (n, 4) ark words each (an allocate() without its partner leaves a_R = 0)"""
    left = np.array([F.w(m.val.get((1, i), 0)) for i in range(n)], dtype=np.uint64).reshape(n, 4)
    right = np.array([F.w(m.val.get((2, i), 0)) for i in range(n)], dtype=np.uint64).reshape(n, 4)
    return left, right


def like(E, src, twin, engine=None, assign=True, left=None, right=None):
    """a like-prover of src.p (a Rec) that commits what twin committed and, with assign, takes twin's multiplier inputs (or left / right)"""
    r = Rec()
    r.t = transcript(E)
    r.p = src.p.new_like(r.t)
    r.V, _ = r.p.commit(twin.v, twin.b, engine=engine)
    if assign:
        r.p.assign_multipliers(twin.left if left is None else left, twin.right if right is None else right)
    r.spec = src.spec
    return r


def verifier(E, curve, F, spec, V, publics=None):
    v = E.VerifierCS(curve, transcript(E))
    vars_ = v.commit(V)
    run_gadget(v, F, spec, None, vars_, publics)
    return v


def oracle_proof(O, curve, F, spec, wit_seed, gens, rng):
    """the oracle's Prover on the same statement (transcript-mode blinding, the default Pedersen pair)"""
    vals, blinds = committed(F, spec, wit_seed)
    p = O.ProverCS(curve, LABEL)
    p.transcript().append_message(b"dom-sep", b"prover like v1")
    p.start()
    _, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v % F.p
    run_gadget(p, F, spec, wit, vars_, [])
    return p.prove(gens, rng)


def rng(tag):
    return bytes([tag & 255, (tag >> 8) & 255]) + bytes([0x5A]) * 30
