"""Blinding vectors from a key (include/arkbp.h BP_BLINDING_EXPANDED), the parts that need no GPU: bp_host_blind_expand against a
restatement of the construction in Python — tests/pystrobe.py's ChaCha20 block, the 64 bytes as one little-endian integer, mod r —
and the semantics of bp_prover_set_blinding / bp_prover_blinding."""
import random

import numpy as np
import pytest

R_MOD = [0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F, (1 << 255) - 19]   # the scalar fields of secq256k1 and zorro
GRID = [(0, 1), (0, 2), (1, 1), (3, 5), (0, 257), ((1 << 31) - 3, 3)]
# RFC 7539 section 2.3 with an all-zero key, nonce and counter (the block tests/test_oracle_vectors.py pins for the model)
ZERO_KEY_BLOCK = bytes.fromhex("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586")


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import engine

    return engine


def ark_words(x, r):
    """the ABI's scalar layout: x * 2^256 mod r as four 64-bit words"""
    m = x % r * (1 << 256) % r
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def from_ark(rows, r):
    inv = pow(1 << 256, -1, r)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * inv % r for row in np.asarray(rows).reshape(-1, 4)]


def model(curve, kappa, j0, count):
    """s_L, s_R (ints) of the phase-local indices j0 .. j0 + count - 1"""
    import pystrobe as PS

    r = R_MOD[curve]
    key = (kappa % r).to_bytes(32, "little")

    def W(t):
        return int.from_bytes(PS.chacha20_block(key, t), "little") % r

    return [W(2 * (j0 + i)) for i in range(count)], [W(2 * (j0 + i) + 1) for i in range(count)]


def kappas(curve):
    r = R_MOD[curve]
    return [0, 1, r - 1, random.Random(1000 + curve).randrange(r)]


def test_model_block_is_the_rfc_block():
    import pystrobe as PS

    assert PS.chacha20_block(bytes(32), 0) == ZERO_KEY_BLOCK


@pytest.mark.parametrize("curve", [0, 1])
def test_zero_key_first_scalar_is_the_rfc_block_reduced(E, curve):
    r = R_MOD[curve]
    sL, sR = E.host_blind_expand(curve, ark_words(0, r), 0, 1)
    assert from_ark(sL, r) == [int.from_bytes(ZERO_KEY_BLOCK, "little") % r]
    assert from_ark(sR, r) == model(curve, 0, 0, 1)[1]


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("j0,count", GRID)
def test_host_expansion_equals_the_python_restatement(E, curve, j0, count):
    r = R_MOD[curve]
    for kappa in kappas(curve):
        sL, sR = E.host_blind_expand(curve, ark_words(kappa, r), j0, count)
        wL, wR = model(curve, kappa, j0, count)
        assert from_ark(sL, r) == wL and from_ark(sR, r) == wR
        assert all(sum(int(w) << (64 * i) for i, w in enumerate(row)) < r for row in np.concatenate([sL, sR]))   # reduced ark words


def test_host_expansion_refuses_bad_arguments(E):
    from ark_bulletproofs_amd._lib import ArkbpError

    r = R_MOD[0]
    with pytest.raises(ArkbpError):
        E.host_blind_expand(2, ark_words(1, r), 0, 1)                       # unknown curve
    with pytest.raises(ArkbpError):
        E.host_blind_expand(0, ark_words(1, r), (1 << 31) - 1, 2)           # an index reaches 2^31
    with pytest.raises(ArkbpError):
        E.host_blind_expand(0, np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), 0, 1)   # not a reduced scalar


@pytest.mark.parametrize("curve", [0, 1])
def test_setter_semantics(E, curve):
    from ark_bulletproofs_amd._lib import BP_E_ARG, ArkbpError, lib

    assert (E.BLINDING_TRANSCRIPT, E.BLINDING_EXPANDED) == (0, 1)
    t = E.HostTranscript(b"blinding setter")
    p = E.ProverCS(curve, t)
    assert p.blinding == E.BLINDING_TRANSCRIPT                      # the default
    p.set_blinding(E.BLINDING_EXPANDED)
    assert p.blinding == E.BLINDING_EXPANDED
    p.set_blinding(E.BLINDING_TRANSCRIPT)
    assert p.blinding == E.BLINDING_TRANSCRIPT
    for bad in (2, -1, 7):
        with pytest.raises(ArkbpError) as ei:
            p.set_blinding(bad)
        assert ei.value.code == BP_E_ARG and p.blinding == E.BLINDING_TRANSCRIPT
    assert lib().bp_prover_set_blinding(None, 1) == BP_E_ARG and lib().bp_prover_blinding(None, None) == BP_E_ARG
    v = E.VerifierCS(curve, E.HostTranscript(b"blinding setter"))
    with pytest.raises(ArkbpError) as ei:
        E.ProverCS.set_blinding(v, E.BLINDING_EXPANDED)             # a verifier handle
    assert ei.value.code == BP_E_ARG
    # once the head of prove() has run the mode is fixed
    p.set_blinding(E.BLINDING_EXPANDED)
    p.multiply([(E.ONE_VAR, ark_words(3, R_MOD[curve]))], [(E.ONE_VAR, ark_words(5, R_MOD[curve]))])
    p.precompute(bytes([9]) * 32)
    with pytest.raises(ArkbpError) as ei:
        p.set_blinding(E.BLINDING_TRANSCRIPT)
    assert ei.value.code == BP_E_ARG and p.blinding == E.BLINDING_EXPANDED


@pytest.mark.parametrize("curve", [0, 1])
def test_statement_takes_the_mode_through_its_prover_handle(E, curve):
    from ark_bulletproofs_amd._lib import ArkbpError

    s = E.Statement(curve, 0, [4], bytes([3]) * 32)
    assert s.blinding == E.BLINDING_TRANSCRIPT
    s.set_blinding(E.BLINDING_EXPANDED)
    assert s.blinding == E.BLINDING_EXPANDED
    s.precompute()
    with pytest.raises(ArkbpError):
        s.set_blinding(E.BLINDING_TRANSCRIPT)
    s.free()


@pytest.mark.parametrize("curve", [0, 1])
def test_precompute_batch_of_eight_takes_expanded_heads(E, curve):
    """eight equal shapes (the x8 lockstep pattern) in expanded mode, with one default-mode batch beside them: both complete"""
    for mode in (E.BLINDING_EXPANDED, E.BLINDING_TRANSCRIPT):
        stmts = [E.Statement(curve, 1, [64, 1000 + j], bytes([j + 1]) * 32) for j in range(8)]
        for s in stmts:
            s.set_blinding(mode)
        E.precompute_batch(stmts)
        assert [s.blinding for s in stmts] == [mode] * 8
        for s in stmts:
            s.free()
