"""Shared by test_pedersen_gens_cpu.py and test_gpu_pedersen_gens.py: the two caller-chosen PedersenGens pairs and the independent
checks of what the engine computes under them.  The oracle's C API is fixed to PedersenGens::default(), so there is no byte-parity
oracle for another pair; the checks are algebraic:

  (I)  commitments: under the multiples pair B' = s*B, Bb' = t*Bb, commit'(v, r) is the oracle's default pedersen_commit(s*v, t*r);
       under any pair it is v*B' + r*Bb' from the oracle's scalar_mul and point_add;
  (II) proofs: Verifier::verification_scalars does not depend on the pair, so the oracle's scalars over
       [B', Bb', G[..N], H[..N], the proof's points] (oracle/protocol.hpp: B, B_blinding, g, h, A_I1, A_O1, S1, A_I2, A_O2, S2, V[m],
       T_1,3,4,5,6, L[k], R[k]) must sum to the identity.  Nothing of that comes from the engine but the proof bytes and commitments."""
import functools

import numpy as np

CHAIN_PARTY = 0x50434731
MULT_S = 3          # B' = 3 * B
MULT_T_BELOW_R = 2  # Bb' = (r - 2) * Bb


@functools.lru_cache(maxsize=None)
def _pairs(curve):
    from ark_bulletproofs_amd import engine as E
    from oracle import pyoracle as O

    FR = O.fid(curve, True)
    r = O.modulus(FR)
    chain = E.host_derive_generators(curve, 0, CHAIN_PARTY, 2)
    B, Bb = O.pedersen_default(curve)
    mult = np.stack([O.scalar_mul(curve, B, O.fe_from_int(FR, MULT_S)), O.scalar_mul(curve, Bb, O.fe_from_int(FR, r - MULT_T_BELOW_R))])
    for p in list(chain) + list(mult):
        assert O.on_curve(curve, p) and p.any()
    return {"chain": (chain[0].copy(), chain[1].copy()), "mult": (mult[0].copy(), mult[1].copy()), "default": (B.copy(), Bb.copy())}


def pair(curve, which):
    """(B, B_blinding) as two arrays of 8 ark words: "chain" = GeneratorsChain 'G' of party 0x50434731, first two points (no known
    relation); "mult" = (3 * B, (r - 2) * B_blinding) of the default pair; "default"."""
    B, Bb = _pairs(curve)[which]
    return B.copy(), Bb.copy()


def edge_scalars(O, curve, count, seed):
    """`count` (v, blind) pairs: the edge values 0, 1, r - 1 in both positions first, random ones among and after them"""
    FR = O.fid(curve, True)
    r = O.modulus(FR)
    edge = [(0, 1), (1, 0), (r - 1, 1), (1, r - 1), (r - 1, r - 1), (0, r - 1), (1, 1)]
    rnd = O.fe_rand(FR, bytes([seed]) * 32, 2 * count)
    v, b = rnd[:count].copy(), rnd[count:].copy()
    for i, (x, y) in enumerate(edge):
        j = 2 * i + 1   # odd positions: random values stay among them
        if j >= count:
            break
        v[j], b[j] = O.fe_from_int(FR, x), O.fe_from_int(FR, y)
    if count >= 3:
        b[2] = O.fe_from_int(FR, 0)      # a random value with a zero blinding
    return np.ascontiguousarray(v), np.ascontiguousarray(b)


def commit_expected(O, curve, which, v, blind):
    """check (I) for one (v, blind): what the oracle says the commitment under pair `which` is"""
    FR = O.fid(curve, True)
    B, Bb = pair(curve, which)
    direct = O.point_add(curve, O.scalar_mul(curve, B, v), O.scalar_mul(curve, Bb, blind))
    if which == "mult":
        r = O.modulus(FR)
        sv = O.fe_op("mul", FR, O.fe_from_int(FR, MULT_S), v)
        tb = O.fe_op("mul", FR, O.fe_from_int(FR, r - MULT_T_BELOW_R), blind)
        assert (O.pedersen_commit(curve, sv, tb) == direct).all()   # the two forms of (I) agree with each other
    return direct


def decode_proof_points(O, curve, proof):
    """the proof's 11 + 2k compressed points (R1CSProof::to_bytes, src/r1cs/proof.rs:74-81: A_I1, A_O1, S1, A_I2, A_O2, S2, T_1, T_3, T_4,
    T_5, T_6; t_x, t_x_blinding, e_blinding; LE64(k), L[k]; LE64(k), R[k]; a, b), decoded by the oracle"""
    fixed = 11 * 33 + 3 * 32 + 16 + 2 * 32
    assert len(proof) >= fixed and (len(proof) - fixed) % 66 == 0
    k = (len(proof) - fixed) // 66

    def pt(off):
        p = O.point_deser_compressed(curve, proof[off:off + 33])
        assert p is not None
        return p

    head = [pt(33 * i) for i in range(11)]
    base = 11 * 33 + 3 * 32
    assert int.from_bytes(proof[base:base + 8], "little") == k
    L = [pt(base + 8 + 33 * j) for j in range(k)]
    base += 8 + 33 * k
    assert int.from_bytes(proof[base:base + 8], "little") == k
    R = [pt(base + 8 + 33 * j) for j in range(k)]
    return head[:6], head[6:], L, R


def proof_check_point(O, curve, which, scenario, params, gens_cap, proof, commitments, publics):
    """check (II): the oracle's verification scalars over the pair `which`, the oracle's G and H and the proof's own points"""
    _, _, L, R = decode_proof_points(O, curve, proof)
    k = len(L)
    N = 1 << k
    m = len(np.asarray(commitments).reshape(-1, 8))
    cap = 2 + 2 * N + 6 + m + 5 + 2 * k
    rc, sc = O.r1cs_verification_scalars(curve, scenario, params, gens_cap, proof, commitments, publics, cap + 8)
    assert rc == 0, rc
    assert len(sc) == cap, (len(sc), cap)
    A, T, L, R = decode_proof_points(O, curve, proof)
    B, Bb = pair(curve, which)
    G, H = O.bp_gens(curve, N)
    bases = np.concatenate([np.stack([B, Bb]), G, H, np.stack(A), np.asarray(commitments, dtype=np.uint64).reshape(-1, 8), np.stack(T)]
                           + ([np.stack(L), np.stack(R)] if k else []))
    return O.msm(curve, bases, sc)
