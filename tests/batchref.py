"""Reference for the batched mega-check that scales to thousands of instances (test infrastructure, CPU oracle only).

The reference's batch_verify (src/r1cs/verifier.rs:604-691) is linear in its weights: the value of the mega-check MSM of a batch is

    point(batch) = sum_j alpha_j * U_j,

alpha_j the j-th Fr::rand of the seeded ChaCha20 (after `alpha_skip` draws), U_j instance j's mega-check point with weight 1 — the
identity for a valid instance.  U_j comes from the oracle on a batch of ONE: batch_verify_point with the first weight of a fixed seed
divided out (scenario instances), batch_verify_cs with weight 1 (recorded handles).  The unit points are cached at module scope per
(curve, instance), so a pool of proofs pays for them once and any prefix, subset or alpha window of it is one MSM on the CPU.
tests/test_batchref_cpu.py checks the identity against the oracle's direct batch points."""
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

UNIT_SEED = bytes([0xA5]) * 32       # the weight the oracle draws for a batch of one (divided out again)
_UNITS = {}                          # (curve, instance key) -> unit point, uint64[8] (identity = all zero)


def _threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 8)))


def scenario_key(inst):
    sc, prm, proof, cm, pb = inst
    h = hashlib.sha256()
    h.update(np.asarray([sc] + list(prm), dtype=np.int64).tobytes())
    h.update(bytes(proof))
    h.update(np.ascontiguousarray(cm, dtype=np.uint64).tobytes())
    h.update(np.ascontiguousarray(pb, dtype=np.uint64).tobytes())
    return h.digest()


# ---- defects that keep a proof well formed ------------------------------------------------------------------------------------
# Instance j of a defective pool carries one of: a low bit of t_x_blinding flipped (bit j % 8 of its least significant byte; wire
# offset 395 = 11 points + t_x, src/r1cs/proof.rs:74-81), or — at j % 8 in (3, 5) — wrong commitments (5: the first two swapped,
# 3: one replaced by the generator), which reach the check through other buffers (the absorbed V, the W_V terms).
TXB_BYTE = 11 * 33 + 32


def defect_proof(proof, j):
    if j % 8 in (3, 5):
        return bytes(proof)
    b = bytearray(proof)
    b[TXB_BYTE] ^= 1 << (j % 8)
    return bytes(b)


def defect_commitments(V, j, O, curve):
    V = np.array(V, dtype=np.uint64).reshape(-1, 8).copy()
    if j % 8 == 5 and len(V) >= 2:
        V[[0, 1]] = V[[1, 0]]
    elif j % 8 in (3, 5):
        V[(j // 8) % len(V)] = O.generator(curve)
    return V


def defective(inst, j, O, curve):
    """scenario instance (scenario, params, proof, commitments, publics) with the defect of pool position j"""
    sc, prm, proof, cm, pb = inst
    return sc, prm, defect_proof(proof, j), (defect_commitments(cm, j, O, curve) if j % 8 in (3, 5) else cm), pb


class BatchRef:
    """unit points and expected batch points for one curve (gens_cap: the oracle's generator capacity for the statements)"""

    def __init__(self, O, curve, gens_cap):
        self.O, self.curve, self.gens_cap = O, curve, gens_cap
        self.fid = O.fid(curve, True)
        a1 = O.fe_rand(self.fid, UNIT_SEED, 1)[0]
        self._a1_inv = O.fe_op("inv", self.fid, a1)
        self.one = O.fe_from_int(self.fid, 1)

    # ---- unit points ----------------------------------------------------------------------------------------------------------
    def _unit_scenario(self, inst):
        rc, pt = self.O.batch_verify_point(self.curve, [inst], self.gens_cap, UNIT_SEED)
        assert rc in (self.O.OK, self.O.E_VERIFICATION), "the oracle rejects instance %r before the mega-check (rc %d)" % (inst[:2], rc)
        pt = np.asarray(pt, dtype=np.uint64).reshape(8)
        return pt if not pt.any() else self.O.scalar_mul(self.curve, pt, self._a1_inv)

    def units(self, instances):
        """(n, 8) unit points of scenario instances [(scenario, params, proof, commitments, publics)]"""
        keys = [(self.curve, scenario_key(i)) for i in instances]
        todo = {}
        for key, inst in zip(keys, instances):
            if key not in _UNITS and key not in todo:
                todo[key] = inst
        if todo:
            items = list(todo.items())
            _UNITS[items[0][0]] = self._unit_scenario(items[0][1])       # (the oracle's generator tables grow on the first call: alone)
            with ThreadPoolExecutor(_threads()) as ex:               # (the oracle's calls run without the GIL; they share no state)
                for (key, _), pt in zip(items[1:], ex.map(lambda kv: self._unit_scenario(kv[1]), items[1:])):
                    _UNITS[key] = pt
        return np.stack([_UNITS[k] for k in keys])

    def units_cs(self, keys, make):
        """(n, 8) unit points of recorded handles.  keys: hashable per instance; make(j) -> (the oracle's VerifierCS of instance j,
        started and committed, its gadget recorded; the proof bytes), called only for instances not cached yet."""
        out = []
        for j, key in enumerate(keys):
            ck = (self.curve, "cs", key)
            if ck not in _UNITS:
                ov, proof = make(j)
                rc, pt = self.O.batch_verify_cs(self.curve, [ov], [proof], self.gens_cap, self.one.reshape(1, 4))
                assert rc in (self.O.OK, self.O.E_VERIFICATION), "the oracle rejects recorded instance %d before the mega-check (rc %d)" % (j, rc)
                _UNITS[ck] = np.asarray(pt, dtype=np.uint64).reshape(8).copy()
            out.append(_UNITS[ck])
        return np.stack(out)

    # ---- weights and sums -----------------------------------------------------------------------------------------------------
    def alphas(self, seed, count, skip=0):
        """the weights batch_verify draws for instances skip .. skip + count - 1 of a seeded batch"""
        return self.O.fe_rand(self.fid, seed, skip + count)[skip:]

    def point(self, units, alphas):
        """sum_j alphas[j] * units[j] (identity = all zero)"""
        units = np.asarray(units, dtype=np.uint64).reshape(-1, 8)
        alphas = np.asarray(alphas, dtype=np.uint64).reshape(-1, 4)
        assert len(units) == len(alphas)
        nz = units.any(axis=1)
        if not nz.any():
            return np.zeros(8, dtype=np.uint64)
        return np.asarray(self.O.msm(self.curve, units[nz], alphas[nz]), dtype=np.uint64).reshape(8)

    def check(self, got, units, alphas, run=None, what="batch"):
        """asserts got == sum_j alphas[j] * units[j].  On a mismatch with `run` given (run(lo, hi) -> the product's point for the
        sub-batch [lo, hi) weighted by alphas[lo:hi], i.e. alpha_skip = lo), bisects and names the first instance whose
        contribution is wrong."""
        exp = self.point(units, alphas)
        got = np.asarray(got, dtype=np.uint64).reshape(8)
        if (got == exp).all():
            return
        msg = "%s: mega-check point differs from the unit-point reference (%d instances)" % (what, len(units))
        if run is not None:
            msg += "; " + self.locate(run, units, alphas)
        raise AssertionError(msg)

    def locate(self, run, units, alphas):
        lo, hi = 0, len(units)
        if (np.asarray(run(lo, hi)) == self.point(units, alphas)).all():
            return "the whole batch agrees when run again (not reproducible)"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if not (np.asarray(run(lo, mid)) == self.point(units[lo:mid], alphas[lo:mid])).all():
                hi = mid
            elif not (np.asarray(run(mid, hi)) == self.point(units[mid:hi], alphas[mid:hi])).all():
                lo = mid
            else:
                return "the halves [%d, %d) and [%d, %d) agree on their own: the error needs both" % (lo, mid, mid, hi)
        return "the first wrong contribution is instance %d" % lo
