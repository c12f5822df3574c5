"""k_ve_tail alone (bp_debug_msm_each): many short, independent variable-base MSMs in one launch, against bp_msm job by job and
against the CPU oracle, bit-exact, on both curves.  Job lengths 0 / 1 / 2 / 25 / 64 / 300, job counts 1 / 2 / 63 / 64 / 65, the
scalars 0, 1, r - 1, only the top window, only one bit plane, random ones; identity bases, equal and opposite points, running sums
that meet their next addend — every exceptional case of the complete additions; Montgomery and canonical scalar input."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 2, 25, 64, 300]
COUNTS = [1, 2, 63, 64, 65]


class Jobs:
    def __init__(self, O, curve):
        self.O, self.curve = O, curve
        self.fid = O.fid(curve, True)
        self.r = O.modulus(self.fid)
        G, H = O.bp_gens(curve, 160)
        self.pool = np.concatenate([G, H])
        self.rnd = random.Random(77 + curve)
        r, rnd = self.r, self.rnd
        topw = (r.bit_length() - 1) // 4
        self.special = [0, 1, r - 1, (r >> (4 * topw)) << (4 * topw), 1 << (r.bit_length() - 1)] + \
                       [sum((1 << b) << (4 * w) for w in range(topw)) for b in range(4)] + [1 << (4 * 37 + 2), 15 << (4 * 20)]
        # the regular jobs: lengths cycle, every job starts with a few special scalars (rotating), the rest random
        self.regular = []
        for j in range(max(COUNTS)):
            n = LENGTHS[j % len(LENGTHS)]
            idx = [rnd.randrange(len(self.pool)) for _ in range(n)]
            ks = [self.special[(j + t) % len(self.special)] if t < 4 else rnd.randrange(r) for t in range(n)]
            self.regular.append((self.pool[idx], ks))
        P, Q = self.pool[3], self.pool[200]
        nP = np.asarray(O.scalar_mul(curve, P, O.fe_from_int(self.fid, r - 1)), dtype=np.uint64).reshape(8)
        inf = np.zeros(8, dtype=np.uint64)
        s = rnd.randrange(r)
        self.edge = {
            "all identity": (np.stack([inf] * 5), [rnd.randrange(r) for _ in range(5)]),
            "identity among real points": (np.stack([P, inf, Q, inf, inf, self.pool[9]]), [rnd.randrange(r) for _ in range(6)]),
            "identity first": (np.stack([inf, P]), [5, 7]),
            "(P, P) unit scalars": (np.stack([P, P]), [1, 1]),
            "(P, P) one random scalar": (np.stack([P, P]), [s, s]),
            "(P, -P) equal scalars": (np.stack([P, nP]), [s, s]),
            "(P, -P) then a point": (np.stack([P, nP, Q]), [s, s, 3]),
            # planes: pl3 = P, pl2 = P + P (the running sum meets its addend), then 2 pl3 = 2P meets pl2 = 2P in the window's Horner step
            "five times P: 8 4 4 1 1": (np.stack([P] * 5), [8, 4, 4, 1, 1]),
            "five times P: one scalar": (np.stack([P] * 5), [s] * 5),
            "five times P: 1 1 2 4 8 in the top window": (np.stack([P] * 5), [d << (4 * (topw - 1)) for d in (1, 1, 2, 4, 8)]),
            "sums to the identity across windows": (np.stack([P, nP]), [16, 16]),
            "empty": (np.zeros((0, 8), dtype=np.uint64), []),
        }
        self._exp = {}

    def mont(self, ks):
        return np.stack([self.O.fe_from_int(self.fid, k) for k in ks]) if ks else np.zeros((0, 4), dtype=np.uint64)

    def canon(self, ks):
        return np.array([self.O.int_to_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)

    def expected(self, key, job):
        """the oracle's MSM of one job (computed once)"""
        if key not in self._exp:
            b, ks = job
            self._exp[key] = np.asarray(self.O.msm(self.curve, b, self.mont(ks)), dtype=np.uint64).reshape(8) if len(ks) else np.zeros(8, dtype=np.uint64)
        return self._exp[key]


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def env(request, oracle):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    yield e, Jobs(oracle, request.param)
    e.close()


@pytest.mark.parametrize("count", COUNTS)
def test_job_counts_and_lengths(env, count):
    eng, J = env
    jobs = J.regular[:count]
    got = eng.debug_msm_each([(b, J.mont(ks)) for b, ks in jobs])
    assert got.shape == (count, 8)
    for j, job in enumerate(jobs):
        assert (got[j] == J.expected(("regular", j), job)).all(), "job %d of %d (%d terms) differs from the oracle" % (j, count, len(job[1]))


def test_against_bp_msm_job_by_job_and_canonical_input(env):
    eng, J = env
    jobs = J.regular[:13] + list(J.edge.values())
    mont = eng.debug_msm_each([(b, J.mont(ks)) for b, ks in jobs])
    canon = eng.debug_msm_each([(b, J.canon(ks)) for b, ks in jobs], canonical=True)
    for j, (b, ks) in enumerate(jobs):
        ref = eng.msm(b, J.mont(ks)) if len(ks) else np.zeros(8, dtype=np.uint64)
        assert (mont[j] == ref).all(), "job %d: Montgomery input differs from bp_msm" % j
        assert (canon[j] == ref).all(), "job %d: canonical input differs from bp_msm" % j


def test_exceptional_bases(env):
    eng, J = env
    names = list(J.edge)
    got = eng.debug_msm_each([(J.edge[n][0], J.mont(J.edge[n][1])) for n in names])
    for j, n in enumerate(names):
        assert (got[j] == J.expected(("edge", n), J.edge[n])).all(), "%s: differs from the oracle" % n
    ident = ["all identity", "(P, -P) equal scalars", "sums to the identity across windows", "empty"]
    for n in ident:
        assert not got[names.index(n)].any(), "%s: the identity is all-zero" % n
    assert got[names.index("(P, P) unit scalars")].any()
    # a job's neighbours do not matter: every edge job alone, and between two long jobs
    long_job = (J.regular[5][0], J.mont(J.regular[5][1]))
    for j, n in enumerate(names):
        alone = eng.debug_msm_each([(J.edge[n][0], J.mont(J.edge[n][1]))])
        assert (alone[0] == got[j]).all(), "%s: alone it gives another point" % n
    mid = eng.debug_msm_each([long_job, (J.edge[names[7]][0], J.mont(J.edge[names[7]][1])), long_job])
    assert (mid[1] == got[7]).all() and (mid[0] == mid[2]).all() and (mid[0] == J.expected(("regular", 5), J.regular[5])).all()


def test_every_special_scalar_on_one_point(env):
    """one term per job: k * P for each special scalar (0, 1, r - 1, top window, single planes, single bits)"""
    eng, J = env
    P = J.pool[11]
    got = eng.debug_msm_each([(P.reshape(1, 8), J.mont([k])) for k in J.special])
    for j, k in enumerate(J.special):
        exp = np.asarray(J.O.scalar_mul(J.curve, P, J.O.fe_from_int(J.fid, k)), dtype=np.uint64).reshape(8) if k else np.zeros(8, dtype=np.uint64)
        assert (got[j] == exp).all(), "scalar %#x" % k
