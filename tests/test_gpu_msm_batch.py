"""bp_msm_batch / bp_msm_batch_dev on the GPU, both curves, bit for bit against the CPU oracle and against bp_msm of each job alone:
every route (short: k_ve_tail, bucketed: k_msb_accum + k_msb_combine, single: msm_run) and every boundary between them with the
knobs lowered (short 4, slice 8, max 40) and at the defaults; Montgomery and canonical input, canonical scalars >= r; every
exceptional operand of the complete additions in a bucket, in the running sum and in the combine step; resident operands left as
they were; the cut into groups; a ctx that goes on working afterwards."""
import contextlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROUTE_LENGTHS = [0, 1, 4, 5, 8, 9, 16, 17, 40, 41, 64]


@contextlib.contextmanager
def knobs(eng, short, slice_terms, batch_max, min_jobs=1):
    """the knobs lowered; min_jobs = 1: a call of any size forms groups"""
    from ark_bulletproofs_amd import engine as E

    ids = (E.TUNE_MSM_BATCH_SHORT, E.TUNE_MSM_BATCH_SLICE, E.TUNE_MSM_BATCH_MAX, E.TUNE_MSM_BATCH_MIN_JOBS)
    for k, v in zip(ids, (short, slice_terms, batch_max, min_jobs)):
        eng.set_tuning(k, v)
    try:
        yield
    finally:
        for k in ids:
            eng.set_tuning(k, 0)


class Jobs:
    def __init__(self, O, curve):
        self.O, self.curve = O, curve
        self.fid = O.fid(curve, True)
        self.r = O.modulus(self.fid)
        G, H = O.bp_gens(curve, 160)
        self.pool = np.concatenate([G, H])
        self.rnd = random.Random(1808 + curve)
        self._exp = {}
        self._long = {}
        r, rnd = self.r, self.rnd
        special = [0, 1, r - 1, 15 << 252 if r >> 255 else 7 << 252, sum(15 << (4 * w) for w in range(62)), 1 << (4 * 37 + 3)]
        # the route jobs: one per length, every job starts with a few special scalars (rotating), the rest random
        self.route = []
        for j, n in enumerate(ROUTE_LENGTHS):
            idx = [rnd.randrange(len(self.pool)) for _ in range(n)]
            ks = [special[(j + t) % len(special)] % r if t < 3 else rnd.randrange(r) for t in range(n)]
            self.route.append((self.pool[idx], ks))

    def neg(self, P):
        return np.asarray(self.O.scalar_mul(self.curve, P, self.O.fe_from_int(self.fid, self.r - 1)), dtype=np.uint64).reshape(8)

    def mont(self, ks):
        return np.stack([self.O.fe_from_int(self.fid, k % self.r) for k in ks]) if len(ks) else np.zeros((0, 4), dtype=np.uint64)

    def canon(self, ks):
        return np.array([self.O.int_to_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)

    def expected(self, key, job):
        """the oracle's MSM of one job, scalars taken mod r (computed once per key)"""
        if key not in self._exp:
            b, ks = job
            self._exp[key] = np.asarray(self.O.msm(self.curve, b, self.mont(ks)), dtype=np.uint64).reshape(8) if len(ks) else np.zeros(8, dtype=np.uint64)
        return self._exp[key]

    def long_job(self, n):
        """a random job of n terms (made once per length)"""
        if n not in self._long:
            rnd = random.Random(n)
            self._long[n] = (self.pool[[rnd.randrange(len(self.pool)) for _ in range(n)]], [rnd.randrange(self.r) for _ in range(n)])
        return self._long[n]


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def env(request, oracle):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    yield e, Jobs(oracle, request.param)
    e.close()


def _delta(eng, before):
    return tuple(a - b for a, b in zip(eng.msm_batch_stats(), before))


def test_routes_and_boundaries(env):
    eng, J = env
    jobs = J.route
    args = [(b, J.mont(ks)) for b, ks in jobs]
    with knobs(eng, 4, 8, 40):
        s0 = eng.msm_batch_stats()
        got = eng.msm_batch(args)
        # lengths 0 1 4 | 5 8 9 16 17 40 | 41 64; the single-route jobs stand at the end: one group, one host wait
        assert _delta(eng, s0) == (3, 6, 2, 1, 1)
        assert got.shape == (len(jobs), 8)
        for j, (b, ks) in enumerate(jobs):
            assert (got[j] == J.expected(("route", j), jobs[j])).all(), "job %d (%d terms) differs from the oracle" % (j, len(ks))
            ref = eng.msm(b, J.mont(ks)) if len(ks) else np.zeros(8, dtype=np.uint64)
            assert (got[j] == ref).all(), "job %d (%d terms) differs from bp_msm" % (j, len(ks))
        # neighbours do not matter: reversed order, and every job alone
        rev = eng.msm_batch(args[::-1])
        assert (rev[::-1] == got).all()
        for j in range(len(jobs)):
            assert (eng.msm_batch([args[j]])[0] == got[j]).all(), "job %d alone gives another point" % j
        # a single-route job between grouped ones ends the group (its terms are not staged)
        s0 = eng.msm_batch_stats()
        mid = eng.msm_batch([args[3], args[9], args[6]])
        assert _delta(eng, s0) == (0, 2, 1, 2, 2) and (mid == got[[3, 9, 6]]).all()
    # the same call at the default knobs: no single route at these lengths, one group
    from ark_bulletproofs_amd import engine as E

    nshort = sum(n <= E.MSM_BATCH_DEFAULTS[0] for n in ROUTE_LENGTHS)
    assert max(ROUTE_LENGTHS) <= E.MSM_BATCH_DEFAULTS[2] and len(jobs) >= E.MSM_BATCH_DEFAULTS[3]
    s0 = eng.msm_batch_stats()
    assert (eng.msm_batch(args) == got).all() and _delta(eng, s0) == (nshort, len(jobs) - nshort, 0, 1, 1)
    # fewer jobs than BP_TUNE_MSM_BATCH_MIN_JOBS: a loop is the faster path, every job takes the single route
    few = E.MSM_BATCH_DEFAULTS[3] - 1
    s0 = eng.msm_batch_stats()
    assert (eng.msm_batch(args[2:2 + few]) == got[2:2 + few]).all() and _delta(eng, s0) == (0, 0, few, 0, 0)


def test_montgomery_and_canonical_input(env):
    eng, J = env
    r, rnd = J.r, J.rnd
    big = [(1 << 256) - 1, r, r + 1, (1 << 256) - r, rnd.randrange(r, 1 << 256), rnd.randrange(r, 1 << 256)]
    with knobs(eng, 4, 8, 40):
        jobs = J.route[:9]
        mont = eng.msm_batch([(b, J.mont(ks)) for b, ks in jobs])
        canon = eng.msm_batch([(b, J.canon(ks)) for b, ks in jobs], canonical=True)
        assert (mont == canon).all()
        # canonical scalars >= r: (k mod r) * P, on the short route (one and three terms) and on the bucketed one
        P = J.pool[21]
        over = [(P.reshape(1, 8), [k]) for k in big] + [(J.pool[30:33], big[:3]), (J.pool[40:46], big), (J.pool[50:67], (big * 3)[:17])]
        got = eng.msm_batch([(b, J.canon(ks)) for b, ks in over], canonical=True)
        for j, (b, ks) in enumerate(over):
            if len(ks) == 1:
                k = ks[0] % r
                exp = np.asarray(J.O.scalar_mul(J.curve, b[0], J.O.fe_from_int(J.fid, k)), dtype=np.uint64).reshape(8) if k else np.zeros(8, dtype=np.uint64)
            else:
                exp = J.expected(("over", j), over[j])
            assert (got[j] == exp).all(), "job %d: canonical scalars >= r" % j


def _edge_jobs(J):
    O, r, rnd = J.O, J.r, J.rnd
    P, Q = J.pool[3], J.pool[200]
    nP = J.neg(P)
    m16P = np.asarray(O.scalar_mul(J.curve, P, O.fe_from_int(J.fid, r - 16)), dtype=np.uint64).reshape(8)
    inf = np.zeros(8, dtype=np.uint64)
    s = rnd.randrange(r)
    fill = [J.pool[60 + i] for i in range(7)]
    return {
        "(P, P) unit scalars": (np.stack([P, P]), [1, 1]),
        "(P, P) one random scalar": (np.stack([P, P]), [s, s]),
        "(P, -P) equal scalars": (np.stack([P, nP]), [s, s]),
        "(P, -P) then a point": (np.stack([P, nP, Q]), [s, s, 3]),           # the bucket becomes the identity and is added to again
        "identity first": (np.stack([inf, P, Q]), [5, 7, s]),
        "identity in the middle": (np.stack([P, inf, Q, inf, inf, J.pool[9]]), [rnd.randrange(r) for _ in range(6)]),
        "all identity": (np.stack([inf] * 10), [rnd.randrange(r) for _ in range(10)]),
        "fifteen times P: 1 .. 15": (np.stack([P] * 15), list(range(1, 16))),
        "fifteen times P: d 16^63": (np.stack([P] * 15), [d << 252 for d in range(1, 16)]),
        "eight (P, s) then eight (-P, s)": (np.stack([P] * 8 + [nP] * 8), [s] * 16),   # slice sums opposite: the combine step meets -X
        "eight (P, s) twice": (np.stack([P] * 16), [s] * 16),                          # slice sums equal: the combine step doubles
        "(P, 16), (-P, 16) in two slices": (np.stack([P] + fill + [nP]), [16] + [0] * 7 + [16]),
        "windows cancel in the Horner pass": (np.stack([P] + fill + [m16P]), [16] + [0] * 7 + [1]),
        "all scalars zero": (J.pool[70:78], [0] * 8),
        "seventeen terms of 2^256 - 1": (J.pool[80:97], [(1 << 256) - 1] * 17),
    }


IDENTITIES = ["(P, -P) equal scalars", "all identity", "eight (P, s) then eight (-P, s)", "(P, 16), (-P, 16) in two slices",
              "windows cancel in the Horner pass", "all scalars zero"]


@pytest.mark.parametrize("slice_terms", [8, 16], ids=["slice8", "slice16"])
def test_exceptional_operands_in_the_bucketed_route(env, slice_terms):
    """short = 1: every job below is bucketed.  slice 8 puts the 15- and 16-term jobs into two slices (the combine step meets equal and
    opposite sums), slice 16 into one (all fifteen buckets of a window hold P: the running sum meets its addend)"""
    eng, J = env
    if not hasattr(J, "edge"):
        J.edge = _edge_jobs(J)
    edge = J.edge
    names = list(edge)
    with knobs(eng, 1, slice_terms, 40):
        s0 = eng.msm_batch_stats()
        got = eng.msm_batch([(edge[n][0], J.canon(edge[n][1])) for n in names], canonical=True)
        assert _delta(eng, s0) == (0, len(names), 0, 1, 1)
        for j, n in enumerate(names):
            assert (got[j] == J.expected(("edge", n), edge[n])).all(), "%s: differs from the oracle" % n
        for n in IDENTITIES:
            assert not got[names.index(n)].any(), "%s: the identity is all-zero" % n
        assert got[names.index("(P, P) unit scalars")].any() and got[names.index("eight (P, s) twice")].any()
        # every job alone
        for j, n in enumerate(names):
            assert (eng.msm_batch([(edge[n][0], J.canon(edge[n][1]))], canonical=True)[0] == got[j]).all(), "%s: alone it gives another point" % n


def test_default_knobs(env):
    from ark_bulletproofs_amd import engine as E

    eng, J = env
    short, _, batch_max, min_jobs = E.MSM_BATCH_DEFAULTS
    slice_terms = 64   # the default slice cap of a call with at most 64 * 128 bucketed terms
    lengths = [short, short + 1, slice_terms - 1, slice_terms, slice_terms + 1, 2 * slice_terms + 1, 3 * slice_terms, 3]
    assert E.msm_batch_default_slice(sum(n for n in lengths if n > short)) == slice_terms
    assert 3 * slice_terms <= batch_max and len(lengths) >= min_jobs and short >= 3
    jobs = [J.long_job(n) for n in lengths]
    s0 = eng.msm_batch_stats()
    got = eng.msm_batch([(b, J.mont(ks)) for b, ks in jobs])
    assert _delta(eng, s0) == (2, 6, 0, 1, 1)
    for j, (b, ks) in enumerate(jobs):
        assert (got[j] == eng.msm(b, J.mont(ks))).all(), "%d terms: differs from bp_msm" % len(ks)
    for j in (0, 1):
        assert (got[j] == J.expected(("default", j), jobs[j])).all()
    # more jobs than one wave of workgroups
    jobs = []
    rnd = random.Random(65)
    for j in range(65):
        n = max(3 * short, 40)
        jobs.append((J.pool[[rnd.randrange(len(J.pool)) for _ in range(n)]], [rnd.randrange(J.r) for _ in range(n)]))
    s0 = eng.msm_batch_stats()
    got = eng.msm_batch([(b, J.mont(ks)) for b, ks in jobs])
    assert _delta(eng, s0) == (0, 65, 0, 1, 1)
    for j, (b, ks) in enumerate(jobs):
        assert (got[j] == eng.msm(b, J.mont(ks))).all(), "job %d of 65 differs from bp_msm" % j


@pytest.mark.parametrize("canonical", [False, True], ids=["montgomery", "canonical"])
def test_resident_operands_stay_as_they_were(env, canonical):
    eng, J = env
    jobs = J.route
    bases = np.concatenate([b.reshape(-1, 8) for b, _ in jobs])
    scal = np.concatenate([(J.canon(ks) if canonical else J.mont(ks)).reshape(-1, 4) for _, ks in jobs])
    lengths = [len(ks) for _, ks in jobs]
    d_b, d_s = eng.upload_points(bases), eng.upload_scalars(scal)
    try:
        b0, s0 = d_b.download(), d_s.download()
        with knobs(eng, 4, 8, 40):
            host = eng.msm_batch([(b, J.canon(ks) if canonical else J.mont(ks)) for b, ks in jobs], canonical=canonical)
            dev = eng.msm_batch_dev(d_b, d_s, lengths, canonical=canonical)
        assert (dev == host).all()
        for j in range(len(jobs)):
            assert (dev[j] == J.expected(("route", j), jobs[j])).all()
        assert (d_b.download() == b0).all(), "bp_msm_batch_dev changed d_bases"
        assert (d_s.download() == s0).all(), "bp_msm_batch_dev changed d_scalars"
    finally:
        d_b.free()
        d_s.free()


def test_groups(env):
    """the arena budget narrowed to 80,000 B: jobs 0 1 4 5 8 9 16 17 (60 terms, 9 slices: 69,120 B) fill the first group, the
    40-term job is the second"""
    eng, J = env
    args = [(b, J.mont(ks)) for b, ks in J.route[:9]]
    with knobs(eng, 4, 8, 40):
        one = eng.msm_batch(args)
        os.environ["ARKBP_MSM_BATCH_ARENA"] = "80000"
        try:
            s0 = eng.msm_batch_stats()
            two = eng.msm_batch(args)
            assert _delta(eng, s0) == (3, 6, 0, 2, 2)
        finally:
            del os.environ["ARKBP_MSM_BATCH_ARENA"]
    assert (one == two).all()
    for j in range(9):
        assert (two[j] == J.expected(("route", j), J.route[j])).all()


def test_leaves_the_ctx_intact(env):
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E

    eng, J = env
    b, ks = J.long_job(300)
    small = [(bb, J.mont(kk)) for bb, kk in J.route[:8]]
    eng.set_profiling(True)
    try:
        eng.reset_profiling()
        with knobs(eng, 4, 8, 40):
            eng.msm_batch(small + [(b[:33], J.mont(ks[:33]))])
        ms, launches = eng.kernel_time(E.K_MSM_BATCH)
        assert ms > 0 and launches == 1
    finally:
        eng.set_profiling(False)
    after = eng.msm(b, J.mont(ks)), eng.debug_msm_each(small)
    fresh = A.Engine(curve=J.curve)
    try:
        assert (fresh.msm(b, J.mont(ks)) == after[0]).all()
        assert (fresh.debug_msm_each(small) == after[1]).all()
    finally:
        fresh.close()
    for j in range(8):
        assert (after[1][j] == J.expected(("route", j), J.route[j])).all()
