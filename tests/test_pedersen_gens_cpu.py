"""PedersenGens { B, B_blinding } of the caller's choice, without a GPU (include/arkbp.h: bp_prover_new_gens,
bp_pedersen_gens_install, bp_ctx_pedersen_gens): a prover handle commits on the host under its own pair through the host's
per-pair fixed-base tables.  Checked against the oracle algebraically (pedersen_gens_common, check (I)): the oracle's C API knows
only the default pair."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import pedersen_gens_common as PG

OK, E_ARG, E_NO_DEVICE = 0, -1, -3
CURVES = pytest.mark.parametrize("curve", [0, 1], ids=["secq256k1", "zorro"])
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r1cs_golden.json")))


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import engine

    return engine


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_exported(E):
    from ark_bulletproofs_amd import _lib

    for name in ("bp_pedersen_gens_install", "bp_ctx_pedersen_gens", "bp_prover_new_gens"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None


@CURVES
@pytest.mark.parametrize("which", ["chain", "mult"])
@pytest.mark.parametrize("m", [1, 3, 4])
def test_host_commit_under_a_callers_pair(E, oracle, curve, which, m):
    O = oracle
    B, Bb = PG.pair(curve, which)
    v, bl = PG.edge_scalars(O, curve, 12, seed=11 + m)
    t = E.HostTranscript(b"pc gens")
    p = E.ProverCS(curve, t, pc_gens=(B, Bb))
    by_hand = E.HostTranscript(b"pc gens")
    by_hand.append_message(b"dom-sep", b"r1cs v1")
    got = []
    for lo in range(0, 12, m):     # several calls of m commitments each: every edge pair is reached for every m
        V, vars_ = p.commit(v[lo:lo + m], bl[lo:lo + m])
        assert [x[1] for x in vars_] == list(range(lo, lo + m))
        got += list(V)
    for i, Vi in enumerate(got):
        assert (Vi == PG.commit_expected(O, curve, which, v[i], bl[i])).all(), i
        by_hand.append_point(curve, b"V", Vi)
    assert E.transcript_state(t) == E.transcript_state(by_hand)
    # (0, 0): the identity, all-zero words
    zero = np.zeros((1, 4), dtype=np.uint64)
    V, _ = p.commit(zero, zero)
    assert not V.any()


@CURVES
def test_two_pairs_from_two_threads(E, oracle, curve):
    """the host's table cache: two handles with different pairs, committing alternately from two threads"""
    O = oracle
    n = 24
    res, err = {}, []
    inputs = {w: PG.edge_scalars(O, curve, n, seed=40 + i) for i, w in enumerate(("chain", "mult"))}
    go = threading.Barrier(2)

    def work(mine, other):
        try:
            hs = {w: E.ProverCS(curve, E.HostTranscript(b"threads"), pc_gens=PG.pair(curve, w)) for w in (mine, other)}
            out = {mine: [], other: []}
            go.wait()
            for i in range(n):
                for w in (mine, other):   # alternate pairs inside the thread, the threads in opposite order
                    v, bl = inputs[w]
                    out[w].append(hs[w].commit(v[i:i + 1], bl[i:i + 1])[0][0])
            res[mine] = out
        except Exception as e:   # pragma: no cover
            err.append(e)

    ts = [threading.Thread(target=work, args=a) for a in (("chain", "mult"), ("mult", "chain"))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not err, err
    expected = {w: [PG.commit_expected(O, curve, w, inputs[w][0][i], inputs[w][1][i]) for i in range(n)] for w in ("chain", "mult")}
    for thread in ("chain", "mult"):
        for w in ("chain", "mult"):
            for i in range(n):
                assert (res[thread][w][i] == expected[w][i]).all(), (thread, w, i)


@CURVES
def test_prover_new_gens_refusals(E, oracle, curve):
    from ark_bulletproofs_amd._lib import lib

    O = oracle
    B, Bb = PG.pair(curve, "chain")
    t = E.HostTranscript(b"refuse")
    before = E.transcript_state(t)
    h = C.c_void_p()
    off = B.copy(); off[4] ^= np.uint64(1)
    assert not O.on_curve(curve, off)
    q = O.modulus(O.fid(curve, False))
    big = B.copy(); big[:4] = O.int_to_limbs(q)                       # x = p
    big2 = B.copy(); big2[4:] = np.uint64(0xFFFFFFFFFFFFFFFF)         # y = 2^256 - 1
    ident = np.zeros(8, dtype=np.uint64)
    for b, bb in ((off, Bb), (B, off), (ident, Bb), (B, ident), (big, Bb), (B, big2)):
        assert lib().bp_prover_new_gens(curve, t.h, _p(b), _p(bb), C.byref(h)) == E_ARG
        assert not h.value
    assert lib().bp_prover_new_gens(curve, t.h, None, _p(Bb), C.byref(h)) == E_ARG
    assert lib().bp_prover_new_gens(curve, t.h, _p(B), None, C.byref(h)) == E_ARG
    assert lib().bp_prover_new_gens(curve, None, _p(B), _p(Bb), C.byref(h)) == E_ARG
    assert lib().bp_prover_new_gens(curve, t.h, _p(B), _p(Bb), None) == E_ARG
    assert lib().bp_prover_new_gens(2, t.h, _p(B), _p(Bb), C.byref(h)) == E_ARG
    assert E.transcript_state(t) == before       # a refused call appends nothing
    # B == B_blinding is a pair like any other
    p = E.ProverCS(curve, t, pc_gens=(B, B))
    FR = O.fid(curve, True)
    V, _ = p.commit(O.fe_from_int(FR, 1).reshape(1, 4), O.fe_from_int(FR, 1).reshape(1, 4))    # B + B: the doubling
    assert (V[0] == O.point_add(curve, B, B)).all()
    V, _ = p.commit(O.fe_from_int(FR, 1).reshape(1, 4), O.fe_from_int(FR, O.modulus(FR) - 1).reshape(1, 4))   # B - B
    assert not V.any()


@CURVES
def test_install_needs_a_device_and_a_ctx(E, curve):
    from ark_bulletproofs_amd._lib import lib

    B, Bb = PG.pair(curve, "chain")
    assert lib().bp_pedersen_gens_install(None, _p(B), _p(Bb)) == E_ARG
    assert lib().bp_pedersen_gens_install(None, None, None) == E_ARG
    assert lib().bp_ctx_pedersen_gens(None, None, None, None) == E_ARG
    eng = E.Engine.host_only(curve, 0)
    try:
        assert lib().bp_pedersen_gens_install(eng.ctx, _p(B), _p(Bb)) == E_NO_DEVICE
        assert lib().bp_pedersen_gens_install(eng.ctx, None, None) == E_NO_DEVICE
        assert lib().bp_pedersen_gens_install(eng.ctx, _p(B), None) == E_ARG      # exactly one null pointer: an argument error first
        b, bb, dflt = eng.pedersen_gens()
        d = E.pedersen_gens(curve)
        assert dflt and (b == d[0]).all() and (bb == d[1]).all()
    finally:
        eng.close()


@pytest.mark.parametrize("curve,name", [(0, "secq256k1"), (1, "zorro")])
def test_default_pair_behaves_as_prover_new(E, oracle, curve, name):
    O, g = oracle, GOLD["curves"][name]
    FR = O.fid(curve, True)
    B, Bb = E.pedersen_gens(curve)
    v = np.array([O.fe_from_int(FR, 5), O.fe_from_int(FR, 9), O.fe_from_int(FR, 0), O.fe_from_int(FR, 1)])
    bl = np.array([O.fe_from_int(FR, 7), O.fe_from_int(FR, 11), O.fe_from_int(FR, 3), O.fe_from_int(FR, 0)])
    ta, tb = E.HostTranscript(b"default"), E.HostTranscript(b"default")
    pa, pb = E.ProverCS(curve, ta, pc_gens=(B, Bb)), E.ProverCS(curve, tb)
    for m in (1, 3, 4):
        Va, _ = pa.commit(v[:m], bl[:m])
        Vb, _ = pb.commit(v[:m], bl[:m])
        assert (Va == Vb).all()
        assert O.point_ser(curve, Va[0], False).hex() == g["pedersen_commit_5_7_uncompressed"]
        for i in range(m):
            assert (Va[i] == O.pedersen_commit(curve, v[i], bl[i])).all()
    assert E.transcript_state(ta) == E.transcript_state(tb)
