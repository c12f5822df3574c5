"""The two routes of the prover's flatten stage (csrc/r1cs_host.inc prove_flatten): the constraint index evaluated on the device
(HostCsc, the default) and the host pass over all terms with three uploads (ARKBP_HOST_FLATTEN set).  Both must give the oracle's
proof bytes.  The library reads the variable once per process, so the host route runs in ONE fresh child process (started from
scratch, under `timeout`), which prints its proofs in hex; this process proves the same statements without the variable.

Statements, on both curves, 8 generators, fixed seeds: a single-phase gadget with 3 multipliers and 2 committed variables, a k = 2
shuffle (no phase-1 multipliers), and a two-phase gadget with 3 + 2 multipliers."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = b"FlattenRoutes"
GENS = 8
SEED = bytes([23]) * 32
GADGETS = [("single-phase 3x2", dict(struct_seed=31, two_phase=False)), ("two-phase 3+2", dict(struct_seed=32, two_phase=True))]
NAMES = [GADGETS[0][0], "shuffle k=2", GADGETS[1][0]]


def _gadget(GD, O, curve, p, commit, struct_seed, two_phase):
    """one of the two gadgets on a recorder of either side; returns nothing: the state is in p"""
    F = GD.Field(O, curve)
    vals, blinds = GD.make_witness(F, struct_seed, 2)
    _, vars_ = commit([F.w(v) for v in vals], [F.w(b) for b in blinds])
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    GD.random_program(p, F, struct_seed, wit, vars_, n_mul=3, n_alloc=0, n_extra=2, two_phase=two_phase, n_mul2=2, publics=[])


def product_proofs(O, curve):
    """the three proofs by the library, in NAMES order"""
    import gadgets as GD
    from ark_bulletproofs_amd import engine as E

    eng = E.Engine(curve=curve, device=0)
    try:
        eng.gens_derive(GENS)
        out = []
        for _, kw in GADGETS:
            p = E.ProverCS(curve, E.HostTranscript(LABEL))
            _gadget(GD, O, curve, p, p.commit, **kw)
            out.append(bytes(p.prove(eng, SEED)))
        out.insert(1, bytes(eng.prove_scenario(E.SC_SHUFFLE, [2], SEED).proof))
        return out
    finally:
        eng.close()


def oracle_proofs(O, curve):
    import gadgets as GD

    out = []
    for _, kw in GADGETS:
        p = O.ProverCS(curve, LABEL).start()
        _gadget(GD, O, curve, p, p.commit, **kw)
        out.append(bytes(p.prove(GENS, SEED)))
    ref = O.r1cs_prove(curve, O.SC_SHUFFLE, [2], SEED, GENS)
    assert ref.rc == 0
    out.insert(1, bytes(ref.proof))
    return out


def _child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from oracle import pyoracle as O

    assert os.environ.get("ARKBP_HOST_FLATTEN")
    for curve in (0, 1):
        for name, proof in zip(NAMES, product_proofs(O, curve)):
            print("proof %d %d %s" % (curve, NAMES.index(name), proof.hex()), flush=True)


@pytest.mark.gpu
def test_host_flatten_and_device_flatten_give_the_oracles_bytes(oracle):
    env = dict(os.environ, ARKBP_HOST_FLATTEN="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    host_route = {}
    for line in r.stdout.splitlines():
        if line.startswith("proof "):
            _, cv, i, hx = line.split()
            host_route[(int(cv), int(i))] = bytes.fromhex(hx)
    assert sorted(host_route) == [(cv, i) for cv in (0, 1) for i in range(3)]
    assert "ARKBP_HOST_FLATTEN" not in os.environ     # (this process runs the device route)
    for curve in (0, 1):
        ref = oracle_proofs(oracle, curve)
        dev = product_proofs(oracle, curve)
        for i, name in enumerate(NAMES):
            assert len(ref[i]) >= 605               # (11 points, 3 scalars, one round or more, a, b)
            assert dev[i] == ref[i], "device flatten: %s on curve %d differs from the oracle" % (name, curve)
            assert host_route[(curve, i)] == ref[i], "host flatten: %s on curve %d differs from the oracle" % (name, curve)


if __name__ == "__main__":
    if "--child" in sys.argv:
        _child()
