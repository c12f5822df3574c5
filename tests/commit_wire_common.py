"""Shared by test_commit_wire_cpu.py and test_gpu_commit_wire.py: like-instances of one random_program gadget (tests/gadgets.py) with
their commitments either as affine words (bp_verifier_commit) or as the 33-byte wire encodings (bp_verifier_commit_compressed_batch,
deferred).  The proofs come from the oracle's prover (CPU), the encodings from the oracle's serializer."""
import gadgets as GD

LABEL = b"commit wire gadget"
GENS = 64
KW = dict(n_mul=9, n_extra=1, n_alloc=1, n_mul2=4)   # 10 multipliers (14 two-phase): padded size 16; n_extra = 1: no public constants


def wire(O, cv, V):
    return b"".join(O.point_ser(cv, p, True) for p in V)


def prove_items(O, cv, F, count, m, two_phase, struct_seed=41):
    """[(proof bytes, V (m, 8))] of `count` witnesses of one circuit"""
    items = []
    for w in range(count):
        vals, blinds = GD.make_witness(F, 300 + w, m)
        p = O.ProverCS(cv, LABEL)
        p.start()
        V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
        wit = GD.Witness(F)
        for var, v in zip(vars_, vals):
            wit.val[var] = v
        GD.random_program(p, F, struct_seed, wit, vars_, two_phase=two_phase, publics=[], **KW)
        items.append((p.prove(GENS, bytes([w + 1]) * 32), V))
    return items


def verifier(E, O, cv, F, V, two_phase, like=None, blob=None, struct_seed=41):
    """a recorded verifier (like=None) or a like-instance; blob: the commitments as deferred wire bytes instead of V"""
    v = E.VerifierCS(cv, E.HostTranscript(LABEL), like=like)
    vars_ = v.commit(V) if blob is None else v.commit_compressed(blob, defer=True)
    if like is None:
        GD.random_program(v, F, struct_seed, None, vars_, two_phase=two_phase, publics=[], **KW)
    return v


def verifiers(E, O, cv, F, Vs, two_phase, wired, blobs=None):
    """v0 + like-instances over the commitments Vs[k]; wired: deferred wire commitments (blobs[k] overrides the encoding of Vs[k])"""
    def blob(k):
        if not wired:
            return None
        return blobs[k] if blobs is not None and blobs[k] is not None else wire(O, cv, Vs[k])

    v0 = verifier(E, O, cv, F, Vs[0], two_phase, blob=blob(0))
    return [v0] + [verifier(E, O, cv, F, Vs[k], two_phase, like=v0, blob=blob(k)) for k in range(1, len(Vs))]
