"""The group law on the device at every representative and exception.

Part 1: the raw-representative case list of tests/rawcases.py (which the CPU build of the same headers passes with every contract
asserted, tests/test_fp29_host.py) through the hipcc-compiled code: field ops at the contract limits and on every multiple of p,
the lane-per-operation group law, and the quad-cooperative forms on real DPP quads with all four lanes returned.

Part 2: the hot kernels driven into their cold blocks.  Fold rounds of bp_ipa_create over generators that are known multiples of
one base point, with challenges the test chose, so that a chosen round folds equal, opposite or identity points; MSMs whose
buckets hold equal chunk sums, opposite chunk sums and cancellations inside a chunk.  The reference is Python integers
(tests/ipamodel.py, tests/pymodel.py) for the folds and the CPU oracle's MSM for the MSMs."""
import random

import numpy as np
import pytest

import ipamodel as IM
import pymodel as M
import rawcases as RC

pytestmark = pytest.mark.gpu

K_MSM_ACCUM, K_IPA_FOLD, K_FOLD_LADDER, K_FOLD_FINISH, K_MSM_ACCUM_FS = 0, 3, 7, 8, 9      # include/arkbp.h BP_K_*
T_FOLD_BATCH_MIN, T_MSM_BIN_MIN, T_IPA_FREEZE_LEN, T_MSM_WSUM_MIN, T_MSM_GLV_MIN, T_FOLD_QUAD_MAX, T_MSM_CHUNK_CAP = 0, 1, 2, 3, 7, 8, 9   # BP_TUNE_*
# what `knobs` restores: the initial values of the tune_* members of bp_ctx in csrc/arkbp.hip (the C ABI has no getter; a default
# changed there must be changed here, or the later cases of this module run with the stale value)
DEFAULTS = {T_FOLD_BATCH_MIN: 65536, T_MSM_BIN_MIN: 64, T_IPA_FREEZE_LEN: 8192, T_MSM_WSUM_MIN: 1 << 18, T_MSM_GLV_MIN: 256, T_FOLD_QUAD_MAX: 0,
            T_MSM_CHUNK_CAP: 0}


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def eng(request):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    yield e
    e.close()


class knobs:
    """sets tuning knobs for a block and restores the defaults afterwards"""

    def __init__(self, eng, values):
        self.eng, self.values = eng, values

    def __enter__(self):
        for k, v in self.values.items():
            self.eng.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.eng.set_tuning(k, DEFAULTS[k])


# ---- Part 1: raw representatives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_raw_field_cases_on_gpu(eng, fid):
    cases = RC.field_cases(fid)
    for op in sorted({c[0] for c in cases}):
        sel = [c for c in cases if c[0] == op]
        out = eng.debug_field_raw(fid, op, np.array([sum(c[2], []) for c in sel], dtype=np.uint32))
        for (_, name, ins), o in zip(sel, out):
            RC.check_field(fid, op, name, ins, o)


@pytest.mark.parametrize("op", range(7), ids=["jac_add", "jac_madd", "jac_dbl", "jac_madd_fast", "qjac_add", "qjac_madd", "qjac_dbl"])
def test_raw_point_cases_on_gpu(eng, op):
    """every case equals the Python reference; the quad forms in all four lanes, limb for limb (64 different cases per block: the
    quads of a wave diverge); rare is set on every equal / opposite / identity case and the fast result is right where it is not"""
    cv = eng.curve
    sel = [c for c in _point_cases(cv) if c[0] == op]
    assert len(sel) > 64            # more than one 256-thread block of quads
    out = eng.debug_point_raw(op, np.array([c[2] + c[3] for c in sel], dtype=np.uint32))
    for (_, name, _, _, kind, expect), o in zip(sel, out):
        RC.check_point(cv, op, name, kind, expect, o)


_PC = {}


def _point_cases(cv):
    if cv not in _PC:
        _PC[cv] = RC.point_cases(cv)
    return _PC[cv]


# ---- Part 2a: fold rounds ----------------------------------------------------------------------------------------------------------
N = 128      # the round that folds 64 -> 32 has 2 * 32 = 64 lanes: the smallest round the quad form takes
_BASE = {}


def _base_instance(cv):
    """one ordinary instance per curve: random exponents for G and H (the points cost a scalar multiplication each, so they are
    made once and the cases below change a few of them), Q, factors, a, b and the challenges"""
    if cv not in _BASE:
        r = M.CURVES[cv]["r"]
        rnd = random.Random(300 + cv)
        d = dict(g=[rnd.randrange(1, r) for _ in range(N)], h=[rnd.randrange(1, r) for _ in range(N)], qe=rnd.randrange(1, r),
                 Gf=[rnd.randrange(1, r) for _ in range(N)], Hf=[rnd.randrange(1, r) for _ in range(N)],
                 a=[rnd.randrange(r) for _ in range(N)], b=[rnd.randrange(r) for _ in range(N)], us=[rnd.randrange(2, r) for _ in range(7)])
        d["G"] = [IM.mulB(cv, k) for k in d["g"]]
        d["H"] = [IM.mulB(cv, k) for k in d["h"]]
        d["Q"] = IM.mulB(cv, d["qe"])
        _BASE[cv] = d
    return _BASE[cv]


def _scalars(cv, xs):
    r = M.CURVES[cv]["r"]
    return np.array([IM.mont_words(x, r) for x in xs], dtype=np.uint64)


def _points(cv, Ps):
    return np.array([IM.point_words(cv, P) for P in Ps], dtype=np.uint64)


_MODEL_OK = set()


def _validate_model(O, cv):
    """tests/ipamodel.py against the CPU oracle's InnerProductProof::create on the ordinary instance; the challenges of that run
    are recovered by replaying its transcript"""
    if cv in _MODEL_OK:
        return
    d = _base_instance(cv)
    r = M.CURVES[cv]["r"]
    args = (_points(cv, [d["Q"]])[0], _scalars(cv, d["Gf"]), _scalars(cv, d["Hf"]), _points(cv, d["G"]), _points(cv, d["H"]), _scalars(cv, d["a"]), _scalars(cv, d["b"]))
    L, Rr, ao, bo = O.ipa_create(cv, O.Transcript(b"grouplaw"), *args)
    tr = O.Transcript(b"grouplaw")
    tr.append_message(b"dom-sep", b"ipp v1")
    tr.append_u64(b"n", N)
    us = []
    for j in range(len(L)):
        tr.append_point(cv, b"L", L[j])
        tr.append_point(cv, b"R", Rr[j])
        us.append(IM.from_mont_words(tr.challenge_scalar(cv, b"u"), r))
    Ls, Rs, am, bm = IM.ipa_create(cv, d["qe"], d["Gf"], d["Hf"], d["g"], d["h"], d["a"], d["b"], us)
    assert [IM.point_from_words(cv, x) for x in L] == [IM.mulB(cv, k) for k in Ls]
    assert [IM.point_from_words(cv, x) for x in Rr] == [IM.mulB(cv, k) for k in Rs]
    assert IM.from_mont_words(ao, r) == am and IM.from_mont_words(bo, r) == bm
    _MODEL_OK.add(cv)


def _neg(cv, P):
    return None if P is None else (P[0], (-P[1]) % M.CURVES[cv]["q"])


def _round1_case(cv):
    """round 1 (k_ipa_fold_pts / shamir2: s1 * lo + s2 * hi per lane): hi = lo, hi = -lo, identity in lo, in hi, in both — in G at
    lanes 0..4 and in H at lanes 5..9"""
    d = _base_instance(cv)
    g, h, G, H = list(d["g"]), list(d["h"]), list(d["G"]), list(d["H"])
    m = N // 2
    for e, P, o in ((g, G, 0), (h, H, 5)):
        e[m + o], P[m + o] = e[o], P[o]
        e[m + o + 1], P[m + o + 1] = -e[o + 1], _neg(cv, P[o + 1])
        e[o + 2], P[o + 2] = 0, None
        e[m + o + 3], P[m + o + 3] = 0, None
        e[o + 4], P[o + 4], e[m + o + 4], P[m + o + 4] = 0, None, 0, None
    return g, h, G, H


def _uniform_case(cv):
    """the round that folds 64 -> 32 (k_ipa_fold_glv / k_ipa_fold_uniform: hi + t * lo per lane, t = u^-2 for G and u^2 for H).  With
    gamma[j] the exponents of the TRUE generators after round 1, the upper generators of round 1 are solved so that
      lane 0: gamma[32] = -t * gamma[0]   the result is the identity, which travels through the later rounds and the L / R MSMs
      lane 1: gamma[33] = +t * gamma[1]   the final addition is a doubling with Z != 1
      lane 2: gamma[2] = 0                identity in lo          lane 3: gamma[35] = 0   identity in hi
    (independent of how the engine factors out its pending scalar: both halves carry the same one)"""
    d = _base_instance(cv)
    r = M.CURVES[cv]["r"]
    u1, u2 = d["us"][0], d["us"][1]
    g, h, G, H = list(d["g"]), list(d["h"]), list(d["G"]), list(d["H"])
    m = N // 2
    for e, P, f, c1, c2, t in ((g, G, d["Gf"], pow(u1, -1, r), u1, pow(u2, -2, r)), (h, H, d["Hf"], u1, pow(u1, -1, r), u2 * u2 % r)):
        gamma = lambda j: (c1 * f[j] * e[j] + c2 * f[m + j] * e[m + j]) % r     # noqa: E731

        def solve(j, target):
            e[m + j] = (target - c1 * f[j] * e[j]) * pow(c2 * f[m + j], -1, r) % r
            P[m + j] = IM.mulB(cv, e[m + j])
            assert gamma(j) == target % r

        solve(32, -t * gamma(0))
        solve(33, t * gamma(1))
        solve(2, 0)
        solve(35, 0)
    return g, h, G, H


FOLD_SETTINGS = [
    ("shared-inversion epilogue, no frozen tail", {T_FOLD_BATCH_MIN: 1, T_IPA_FREEZE_LEN: 0}),
    ("the same with quad rounds", {T_FOLD_BATCH_MIN: 1, T_IPA_FREEZE_LEN: 0, T_FOLD_QUAD_MAX: 4096}),
    ("defaults", {}),
]


@pytest.mark.parametrize("case", ["round1", "uniform"])
def test_fold_rounds_reach_their_exceptional_blocks(eng, oracle, case):
    cv = eng.curve
    _validate_model(oracle, cv)
    d = _base_instance(cv)
    r = M.CURVES[cv]["r"]
    g, h, G, H = _round1_case(cv) if case == "round1" else _uniform_case(cv)
    Ls, Rs, am, bm = IM.ipa_create(cv, d["qe"], d["Gf"], d["Hf"], g, h, d["a"], d["b"], d["us"])
    exp_L, exp_R = _points(cv, [IM.mulB(cv, k) for k in Ls]), _points(cv, [IM.mulB(cv, k) for k in Rs])
    exp_a, exp_b = IM.mont_words(am, r), IM.mont_words(bm, r)
    args = (_points(cv, [d["Q"]])[0], _scalars(cv, d["Gf"]), _scalars(cv, d["Hf"]), _points(cv, G), _points(cv, H), _scalars(cv, d["a"]), _scalars(cv, d["b"]))
    eng.set_profiling(True)
    try:
        for name, kn in FOLD_SETTINGS:
            it = iter(d["us"])
            with knobs(eng, kn):
                eng.reset_profiling()
                L, R, a, b = eng.ipa_create(*args, lambda Lp, Rp: IM.mont_words(next(it), r))
                counts = {k: eng.kernel_time(k)[1] for k in (K_IPA_FOLD, K_FOLD_LADDER, K_FOLD_FINISH)}
            assert (L == exp_L).all() and (R == exp_R).all(), (name, case)
            assert (a == exp_a).all() and (b == exp_b).all(), (name, case)
            # What the counts show and what they do not: K_IPA_FOLD also counts k_ipa_fold_ab, so it only says that fold rounds ran
            # (round 1's k_ipa_fold_pts runs under every setting by construction of bp_ipa_create, not by this count).  Under the
            # defaults the vectors freeze right after round 1 (n = 64 <= 8192): no ladder runs there, the special points meet the
            # frozen-tail MSMs instead.  With the freeze off the ladders and the shared-inversion epilogue must have run; the count
            # is the same for the lane and the quad form of the ladder (one family), so that the quad kernels answered under the
            # second setting rests on BP_TUNE_FOLD_QUAD_MAX >= 64 lanes, not on a count.  That the cold blocks are ENTERED is shown
            # by fault injection (a final addition without its redo fails both cases), not by these asserts.
            assert counts[K_IPA_FOLD] > 0, name
            if kn:
                assert counts[K_FOLD_LADDER] > 0 and counts[K_FOLD_FINISH] > 0, (name, counts)
    finally:
        eng.set_profiling(False)


# ---- Part 2b: MSM buckets ----------------------------------------------------------------------------------------------------------
def _neg_words(cv, xy):
    q = M.CURVES[cv]["q"]
    P = IM.point_from_words(cv, xy)
    return IM.point_words(cv, (P[0], (-P[1]) % q))


def _msm_inputs(O, cv, n, pattern):
    """n terms (700, 6000: the fixed-shape pipeline, on secq256k1 the GLV split) whose buckets hold equal, opposite and cancelling
    entries.  At these sizes a bucket of a binned window is shared by tens of ordinary terms and the sort places entries with atomic
    cursors, so a block of chosen terms neither fills a bucket alone nor keeps its order: only a pattern that holds for EVERY
    chunking and order is certain to reach the branch it is built for.
      allsame   every base is the same point P: every chunk of every bucket sums to a small signed multiple of P (the digit signs),
                so the reduction's additions meet equal sums (the doubling branch), opposite sums (the cancellation branch) and the
                identity in every window, and the accumulate meets P + P, P - P and the identity at every step.  With the doubling
                or the cancellation branch of qjac_add deleted (fault injection) this pattern fails at both sizes on both curves
    The other patterns put one 16-entry block at index 64 that shares ONE scalar s, so that in every window the block's entries
    meet in one bucket (next to that bucket's ordinary entries):
      equal     eight distinct bases, then the same eight reversed: where the block is chunked alone and in order (chunk cap 8) the
                two chunk sums are the same point under different Jacobian representatives — seen under injection in some windows
                of some runs only
      opposite  the second eight negated: opposite chunk sums, likewise
      cancel    P, P (a doubling), P, -P .. (the accumulator becomes the identity mid-run and continues), and P with s next to P with
                r - s: the GLV split of r - s is the negated split of s, so those entries meet their twins with the sign bit set (the
                lazily negated y).  Without the split about half the windows have a negative digit of s: there -P with the sign bit
                set (y + p) meets P with the sign bit set (2p - y)"""
    r = M.CURVES[cv]["r"]
    G, H = O.bp_gens(cv, n // 2)
    bases = np.concatenate([G, H]).copy()
    sc = O.fe_rand(O.fid(cv, True), bytes([40 + cv]) * 32, n).copy()
    s = random.Random(77 + cv).randrange(1, r)
    sw, nsw = IM.mont_words(s, r), IM.mont_words(r - s, r)
    B = [bases[200 + i].copy() for i in range(8)]
    sc[64:80] = sw
    if pattern == "allsame":
        bases[:] = B[0]
        return bases, sc
    if pattern == "equal":
        blk = B + B[::-1]
    elif pattern == "opposite":
        blk = B + [_neg_words(cv, x) for x in B[::-1]]
    else:
        P, Q, nP = B[0], B[1], _neg_words(cv, B[0])
        blk = [P, P, P, nP, nP, nP, Q, Q, P, P, Q, P, nP, P, Q, Q]
        for i in (7, 9, 15):         # Q - Q = 0, P - P = 0, .. through the negated scalar instead of the negated point
            sc[64 + i] = nsw
    bases[64:80] = np.array(blk)
    return bases, sc


@pytest.mark.parametrize("n", [700, 6000])
@pytest.mark.parametrize("pattern", ["allsame", "equal", "opposite", "cancel"])
def test_msm_buckets_with_equal_opposite_and_cancelling_entries(eng, oracle, pattern, n):
    O, cv = oracle, eng.curve
    bases, sc = _msm_inputs(O, cv, n, pattern)
    exp = O.msm(cv, bases, sc)
    settings = [({T_MSM_CHUNK_CAP: 8}, K_MSM_ACCUM_FS), ({T_MSM_CHUNK_CAP: 16}, K_MSM_ACCUM_FS),
                ({T_MSM_BIN_MIN: 1 << 40}, K_MSM_ACCUM), ({T_MSM_WSUM_MIN: 1}, K_MSM_ACCUM)]    # the last two: the general path, one-pass and two-level sort
    if cv == 0:
        settings += [({T_MSM_CHUNK_CAP: 8, T_MSM_GLV_MIN: 1 << 40}, K_MSM_ACCUM_FS), ({T_MSM_CHUNK_CAP: 16, T_MSM_GLV_MIN: 1 << 40}, K_MSM_ACCUM_FS)]   # no GLV split
    eng.set_profiling(True)
    try:
        for kn, which in settings:
            with knobs(eng, kn):
                eng.reset_profiling()
                got = eng.msm(bases, sc)
                launches = {k: eng.kernel_time(k)[1] for k in (K_MSM_ACCUM, K_MSM_ACCUM_FS)}
            assert (got == exp).all(), (pattern, n, kn)
            other = K_MSM_ACCUM if which == K_MSM_ACCUM_FS else K_MSM_ACCUM_FS
            assert launches[which] > 0 and launches[other] == 0, (pattern, n, kn, launches)    # the pipeline under test is the one that answered
    finally:
        eng.set_profiling(False)
