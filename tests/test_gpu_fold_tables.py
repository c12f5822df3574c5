"""The fold tables T[window][e - 1][i] = e * 2^(w * window) * Gen[i] (csrc/ipa.cuh k_ftab_window / k_ftab_normalize) and the fixed-base
MSM rows 2^(4r) * Gen[i] entry by entry, and the kernels that read the fold tables — k_ipa_fold_tab, k_ipa_fold_tab2 — next to the
ladder kernels, through the prover's own launchers with multipliers the test chose (bp_debug_fold), against the oracle's
double-and-add, bit for bit.

Whole proofs select table entries by whatever digits the transcript produces and fold random generators, so some entries are never
read (zorro's carry window at w = 8, row 64 of the MSM rows), the recoding edges occur by chance and the exceptional redo of the
table folds never meets a finite accumulator.  Here every entry is compared, every entry a multiplier can reach is selected, and
generators of known relation drive the table folds into their cold blocks."""
import random

import numpy as np
import pytest

import ipamodel as IM

pytestmark = pytest.mark.gpu

NG = 512          # generators per vector
NTAB = 384        # bases the fold tables cover: [0, 3 NG / 4), what two rounds from the tables need at N = 512
NENT = 257        # bases of the tables that are compared entry by entry: the second workgroup of k_ftab_window has a lone lane
FB_ROWS = 65
LADDER, LADDER_NAF, TAB, TAB2 = 0, 1, 2, 3                                   # include/arkbp.h BP_DEBUG_FOLD_*
GLV, NAF, QUAD, FINISH, K_TAB, K_TAB2 = 1, 2, 4, 8, 16, 32                   # bits of bp_debug_fold's *took
T_FOLD_BATCH_MIN, T_IPA_FREEZE_LEN, T_MSM_FIXED_MIN, T_FOLD_QUAD_MAX, T_DIRECT_MAX = 0, 2, 5, 8, 12   # BP_TUNE_*
# what `knobs` restores: the initial values of the tune_* members of bp_ctx in csrc/arkbp.hip (the C ABI has no getter)
DEFAULTS = {T_FOLD_BATCH_MIN: 65536, T_FOLD_QUAD_MAX: 0}
SEED = bytes([7]) * 32


class World:
    """an engine with its generators as the oracle sees them, and the products t * Gen[i] already asked for"""


def _world(oracle, cv, eng, G, H):
    w = World()
    w.O, w.cv, w.eng, w.gens = oracle, cv, eng, (G, H)
    w.FR = oracle.fid(cv, True)
    w.r = oracle.modulus(w.FR)
    w.products = {}
    return w


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def T(request, oracle):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=request.param)
    e.gens_derive(NG)
    yield _world(oracle, request.param, e, *oracle.bp_gens(request.param, NG))
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


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def mont(W, k):
    return W.O.fe_from_int(W.FR, k % W.r)


def smul(W, P, k):
    return W.O.scalar_mul(W.cv, P, mont(W, k))


def same(got, exp, what=""):
    got, exp = np.asarray(got).reshape(-1, 8), np.asarray(exp).reshape(-1, 8)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert not len(bad), "%s: %d of %d points differ, first at %s" % (what, len(bad), len(got), bad[:8])


def nwin_of(cv, w):
    return (130 if cv == 0 else 256) // w + 1


def glv(t, r):
    """(k1, k2, lambda) of bp_debug_glv_decompose: t = k1 + lambda * k2 mod r, from the masks it returns"""
    from ark_bulletproofs_amd import _lib

    masks, lam = np.zeros(20, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    assert _lib.lib().bp_debug_glv_decompose(0, _lib.ptr(IM.mont_words(t % r, r)), _lib.ptr(masks), _lib.ptr(lam)) == 0

    def val(m):
        return sum(int(m[i]) << (32 * i) for i in range(5))
    lam = sum(int(lam[i]) << (64 * i) for i in range(4))
    k1, k2 = val(masks[0:5]) - val(masks[5:10]), val(masks[10:15]) - val(masks[15:20])
    assert (k1 + lam * k2 - t) % r == 0
    return k1, k2, lam


def recode(mag, w, nwin):
    """the signed w-bit digits in (-2^(w-1), 2^(w-1)] of a non-negative integer, least significant first (ftab_recode)"""
    out = []
    for _ in range(nwin):
        d = mag & ((1 << w) - 1)
        mag >>= w
        if d > (1 << (w - 1)):
            d -= 1 << w
            mag += 1
        out.append(d)
    assert mag == 0
    return out


def digits(W, t, w):
    """per half (one on zorro; k1 and k2 of the GLV split on secq256k1) the signed digits the table kernels apply for multiplier t:
    |digit| selects the entry, the sign — the digit's own times the half's — negates it"""
    nw = nwin_of(W.cv, w)
    if W.cv == 1:
        return [recode(t % W.r, w, nw)]
    k1, k2, _ = glv(t, W.r)
    return [[(-d if k < 0 else d) for d in recode(abs(k), w, nw)] for k in (k1, k2)]


def products(W, v, t, idx):
    """(t mod r) * Gen_v[i] for i in idx; each is computed once per world"""
    have = W.products.setdefault((v, t % W.r), {})
    for i in idx:
        if i not in have:
            have[i] = smul(W, W.gens[v][i], t)
    return [have[i] for i in idx]


def fold_ref(W, v, t, n, first=0, stride=1):
    """out[i] = Gen[n + i] + t * Gen[i], Gen[j] = generator first + j * stride of vector v"""
    idx = [first + i * stride for i in range(2 * n)]
    tp = products(W, v, t, idx[:n])
    return np.array([W.O.point_add(W.cv, W.gens[v][idx[n + i]], tp[i]) for i in range(n)])


def tab2_ref(W, v, t1, t2, m):
    """out[i] = Gen[3m + i] + t1 * Gen[m + i] + t2 * Gen[2m + i] + t1 t2 * Gen[i]"""
    a = products(W, v, t1, range(m, 2 * m))
    b = products(W, v, t2, range(2 * m, 3 * m))
    c = products(W, v, t1 * t2, range(m))
    add = W.O.point_add
    return np.array([add(W.cv, add(W.cv, W.gens[v][3 * m + i], a[i]), add(W.cv, b[i], c[i])) for i in range(m)])


def fold(W, route, n, tG, tH, t2G=None, t2H=None, first=0, stride=1):
    """bp_debug_fold with integer multipliers; the ladder routes fold the generators themselves, so one reference serves all routes"""
    G = H = None
    if route in (LADDER, LADDER_NAF):
        G, H = W.gens[0][:2 * n], W.gens[1][:2 * n]
    w = [None if t is None else mont(W, t) for t in (tG, tH, t2G, t2H)]
    return W.eng.debug_fold(route, n, w[0], w[1], w[2], w[3], first, stride, G, H)


def table(W, which, nwin, E, n):
    return W.eng.debug_table_points(which).reshape(nwin, E, n, 8)


def check_fold_table(W, tab, gens, w, full, samples):
    """every entry of the bases `full` by the chain e * B = (e - 1) * B + B, next window = 2 * (E * B) with the oracle's addition, and
    the entries `samples` of every base by the oracle's scalar multiplication"""
    nwin, E, n = tab.shape[:3]
    add = W.O.point_add
    for i in full:
        B = gens[i]
        exp = np.zeros((nwin, E, 8), dtype=np.uint64)
        for j in range(nwin):
            acc = B
            exp[j, 0] = acc
            for e in range(2, E + 1):
                acc = add(W.cv, acc, B)
                exp[j, e - 1] = acc
            B = add(W.cv, acc, acc)
        same(smul(W, gens[i], E << (w * (nwin - 1))), exp[nwin - 1, E - 1], "chain of base %d" % i)     # the chain itself, at its far end
        same(tab[:, :, i], exp, "base %d" % i)
    for j, e in samples:
        same(tab[j, e - 1], np.array([smul(W, gens[i], e << (w * j)) for i in range(n)]), "entry (%d, %d) of every base" % (j, e))


def sample_entries(nwin, E):
    return [(0, 1), (0, E), (nwin // 2, E // 2 + 1), (nwin - 1, 1), (nwin - 1, E)]


def search(W, w, targets, tag):
    """multipliers from a seeded stream that between them have every (half, window, digit) of `targets` among their digits"""
    rnd, need, out = random.Random(tag), set(targets), []
    for _ in range(20000):
        if not need:
            break
        t = rnd.randrange(W.r)
        hit = {(h, j, d) for h, ds in enumerate(digits(W, t, w)) for j, d in enumerate(ds)} & need
        if hit:
            out.append(t)
            need -= hit
    assert not need, sorted(need)
    return out


def rand_scalars(W, tag, n):
    rnd = random.Random(1000 * tag + W.cv)
    return [rnd.randrange(2, W.r) for _ in range(n)]


# ---- 1 .. 3: the tables themselves ----------------------------------------------------------------------------------------------------
WIDTHS = {0: (3, 8), 1: (6, 8)}       # per curve: the narrowest width whose digits fit (nwin <= 44) and the widest


@pytest.mark.parametrize("wide", [0, 1], ids=["narrowest", "widest"])
def test_fold_tables_entry_by_entry(T, wide):
    """w = 3 and 8 on secq256k1, 6 and 8 on zorro: every entry of bases 0, 255 and 256 — the last one, the lone lane of the second
    workgroup —, five entries of all 257, in every window including the carry window; size in bytes and window count"""
    e, w, n = T.eng, WIDTHS[T.cv][wide], NENT
    nwin, E = nwin_of(T.cv, w), 1 << (w - 1)
    got_w, nbytes = e.gens_fold_tables(n, window_bits=w)
    assert got_w == w and nbytes == 2 * nwin * E * n * 64
    assert nwin == {(0, 3): 44, (0, 8): 17, (1, 6): 43, (1, 8): 33}[(T.cv, w)]
    for v in (0, 1):
        assert e.debug_tables_ptr(v)[1] == nbytes // 2
        tab = table(T, v, nwin, E, n)
        assert tab.reshape(-1, 8).any(axis=1).all()          # no entry is the identity
        check_fold_table(T, tab, T.gens[v][:n], w, [0, 255, NENT - 1], sample_entries(nwin, E))
    assert e.gens_tables_check() == (0, 0)


def test_fold_tables_of_a_slice(T):
    """rank 1 of 4: column i stands for generator 1 + 4 i (bp_gens_fold_tables_slice) — entries, then a table fold over that slice,
    which reads its upper half from the gathered compact copy"""
    e, w, cols = T.eng, 8, NG // 4
    nwin, E = nwin_of(T.cv, w), 1 << (w - 1)
    got_w, nbytes = e.gens_fold_tables(NG, window_bits=w, rank=1, world=4)
    assert got_w == w and nbytes == 2 * nwin * E * cols * 64
    for v in (0, 1):
        tab = table(T, v, nwin, E, cols)
        assert tab.reshape(-1, 8).any(axis=1).all()
        check_fold_table(T, tab, T.gens[v][1::4], w, [0, cols - 1], sample_entries(nwin, E))
    assert e.gens_tables_check() == (0, 0)
    tG, tH = rand_scalars(T, 2, 2)
    for batch_min in (DEFAULTS[T_FOLD_BATCH_MIN], 1):
        with knobs(e, {T_FOLD_BATCH_MIN: batch_min}):
            Go, Ho, took = fold(T, TAB, 64, tG, tH, first=1, stride=4)
        assert took == K_TAB | (FINISH if batch_min == 1 else 0)
        same(Go, fold_ref(T, 0, tG, 64, 1, 4), "G")
        same(Ho, fold_ref(T, 1, tH, 64, 1, 4), "H")
    # the whole vectors do not lie on this slice's columns, nor does another rank's slice; one element more leaves the generators
    import ark_bulletproofs_amd as A

    for first, stride, n in [(0, 1, 64), (2, 4, 64), (1, 8, 64), (1, 4, 128)]:
        with pytest.raises(A.ArkbpError):
            fold(T, TAB, n, tG, tH, first=first, stride=stride)


def test_msm_rows_entry_by_entry(T):
    """row r of base i is 2^(4r) * Gen[i] for all 65 rows: every row of bases 0, 255, 256 by the chain row r + 1 = 16 * row r, rows 0, 1,
    31, 63 and 64 — 2^256 * Gen[i], which no digit of a reduced scalar but the carry selects — of every base by scalar multiplication"""
    e, n = T.eng, NENT
    assert e.gens_msm_tables(n) == 2 * FB_ROWS * n * 64
    add = T.O.point_add
    for v in (0, 1):
        assert e.debug_tables_ptr(2 + v)[1] == FB_ROWS * n * 64
        rows = e.debug_table_points(2 + v).reshape(FB_ROWS, n, 8)
        assert rows.reshape(-1, 8).any(axis=1).all()
        for i in (0, 255, NENT - 1):
            exp, P = [], T.gens[v][i]
            for _ in range(FB_ROWS):
                exp.append(P)
                for _ in range(4):
                    P = add(T.cv, P, P)
            same(smul(T, T.gens[v][i], 1 << 256), exp[64], "chain of base %d" % i)
            same(rows[:, i], np.array(exp), "base %d" % i)
        for r_ in (0, 1, 31, 63, 64):
            same(rows[r_], np.array([smul(T, T.gens[v][i], 1 << (4 * r_)) for i in range(n)]), "row %d" % r_)
    assert e.gens_tables_check() == (0, 0)
    e.gens_msm_tables(0)
    assert e.debug_tables_ptr(2) == (None, 0)


# ---- 4: every entry a multiplier can reach ----------------------------------------------------------------------------------------------
def pattern(e, w, windows):
    """the integer whose signed digits are e (which may be negative) in the windows [0, windows)"""
    return sum(e << (w * j) for j in range(windows))


def test_every_selectable_entry_is_selected(T):
    """the narrowest usable width per curve (w = 3: 44 windows of 4 entries on secq256k1, w = 6: 43 windows of 32 on zorro), multipliers
    whose digits are one magnitude in every window, in both signs, through k_ipa_fold_tab at n = 64.  What each multiplier reads is
    taken from its digits as the library recodes it — on secq256k1 from the split bp_debug_glv_decompose returns — and the union must
    be every (half, window, entry, sign) a multiplier can reach"""
    e, w, n = T.eng, WIDTHS[T.cv][0], 64
    nwin, E = nwin_of(T.cv, w), 1 << (w - 1)
    assert e.gens_fold_tables(n, window_bits=w)[0] == w
    ts = []
    if T.cv == 1:
        # windows 0 .. 41 hold six bits each; window 42 holds bits 252 .. 254 of a scalar below 2^255 - 19 and the carry: at most 7 + 1
        top = nwin - 1
        assert (7 << (w * top)) < T.r < (8 << (w * top))
        ts += [pattern(d, w, top) for d in range(1, E + 1)]                                    # + d everywhere below the top
        ts += [(1 << (w * top)) + pattern(-d, w, top) for d in range(1, E)]                    # - d everywhere below the top, + 1 there
        ts += [d << (w * top) for d in range(1, 8)] + [(7 << (w * top)) + ((E + 1) << (w * (top - 1)))]   # the top: 1 .. 7, and 7 + carry
        want = {(0, j, d) for j in range(top) for d in range(-E + 1, E + 1) if d} | {(0, top, d) for d in range(1, 9)}
    else:
        # the halves are below 2^129 by contract and below 0xa3 << 120 in fact: windows 0 .. 41 take every digit, window 42 (bits 126 ..
        # 128) 1 and 2, and window 43, which only holds the carry out of window 42, nothing.  Short halves come back from the split as
        # they went in; the digit's sign times the half's sign reaches - E as well.  Window 42 is filled from a seeded stream
        lam = glv(1, T.r)[2]
        low = nwin - 2
        for d in range(1, E + 1):
            for s1, s2 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                ts.append(s1 * pattern(d, w, low) + lam * s2 * pattern(d, w, low))
        for d in range(1, E):
            k = (1 << (w * low)) + pattern(-d, w, low)                                          # digits - d below, + 1 in window 42
            ts += [k + lam * k, -k - lam * k]
        ts += search(T, w, {(h, low, d) for h in (0, 1) for d in (-2, -1, 1, 2)}, 40)
        want = {(h, j, d) for h in (0, 1) for j in range(low) for d in range(-E, E + 1) if d} | {(h, low, d) for h in (0, 1) for d in (-2, -1, 1, 2)}
    ts = [t % T.r for t in ts]
    seen = [set(), set()]
    for k in range(len(ts)):
        tG, tH = ts[k], ts[(k + 1) % len(ts)]
        Go, Ho, took = fold(T, TAB, n, tG, tH)
        assert took == K_TAB
        same(Go, fold_ref(T, 0, tG, n), "G, multiplier %d" % k)
        same(Ho, fold_ref(T, 1, tH, n), "H, multiplier %d" % k)
        for v, t in ((0, tG), (1, tH)):
            seen[v] |= {(h, j, d) for h, ds in enumerate(digits(T, t, w)) for j, d in enumerate(ds) if d}
    for v in (0, 1):
        assert all(abs(d) <= E for _, _, d in seen[v])
        assert want <= seen[v], sorted(want - seen[v])[:8]
    if T.cv == 1:
        assert seen[0] == want           # nothing else exists: - 32, and anything above 8 in the top window, no reduced scalar selects


# ---- 5: edge multipliers through all four routes ---------------------------------------------------------------------------------------
def edge_multipliers(W, w):
    """the multipliers of the edge tests at table width w, with what each is there for"""
    r = W.r
    ts = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, (1 << 128) - 1, 1 << 128, (1 << 255) % r]
    half = 1 << (w - 1)
    run = sum((half + 1) << (w * j) for j in range(2, 8)) + sum(((1 << w) - 1) << (w * j) for j in range(8, 11)) + (1 << (w * 11))
    if W.cv == 0:
        lam = glv(1, r)[2]
        ts += [lam, lam * lam % r, r - lam]
        a, b = 0x9E3779B97F4A7C15F39CC0605CEDC8, 0x1082276BF3A27251F86C6A11D0C18E           # halves short enough to come back as they are
        ts += [(s1 * a + lam * s2 * b) % r for s1, s2 in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
        assert {(k1 < 0, k2 < 0) for k1, k2, _ in (glv(t, r) for t in ts[-4:])} == {(False, False), (False, True), (True, False), (True, True)}
        ts.append(((half << (w * 5)) + 3 + lam * ((half << (w * 9)) + 5)) % r)                  # a digit equal to 2^(w-1) in either half
        ts.append((run + lam * (run << w)) % r)                                                 # runs of 2^(w-1) + 1, then of 2^w - 1: a carry chain
        ds = [digits(W, t, w) for t in ts[-2:]]
        assert half in ds[0][0] and half in ds[0][1]
        assert all(-(half - 1) in h and 0 in h[9:12] for h in ds[1])
        top = 130 // w                                                                          # the last window: bit 128 and the carry out of
        ts += search(W, w, {(1, top, 1), (1, top, -1)}, 50)                                     # the window below (halves above 0x80 << 120)
    else:
        ts.append((half << (w * 5)) + 3)
        ts.append(run)
        top = 256 // w
        ds = [digits(W, t, w)[0] for t in ts[-2:]]
        assert half in ds[0] and -(half - 1) in ds[1] and 0 in ds[1][9:12]
        if w == 8:
            # the last window is only a carry window, and the top byte of a reduced scalar is at most 0x7f: nothing reaches it
            assert all(digits(W, t, w)[0][top] == 0 for t in ts)
        else:
            ts.append(r - 1)      # - 20 in window 0, and its carry runs through the ones above it into the last window
            assert digits(W, r - 1, w)[0][top] == (r >> (w * top)) + 1
    return [t % r for t in ts]


def ladder_bits(W):
    return GLV if W.cv == 0 else NAF


def test_edge_multipliers_single_fold(T):
    """0, 1, 2, r - 1, r - 2, (r -+ 1) / 2, 2^128 - 1, 2^128, 2^255, lambda, lambda^2, r - lambda, the four sign pairs of the GLV halves
    and the recoding edges through the ladders (in-lane inversion, shared-inversion epilogue, quad form; the NAF ladder on both
    curves) and through k_ipa_fold_tab, at n = 64 (one wave per vector) and n = 256 (two workgroups per vector)"""
    e, w = T.eng, 8
    assert e.gens_fold_tables(NTAB, window_bits=w)[0] == w
    ts = edge_multipliers(T, w)
    lb = ladder_bits(T)
    for k in range(len(ts)):
        tG, tH = ts[k], ts[(k + 1) % len(ts)]
        for n in (64, 256):
            exp = fold_ref(T, 0, tG, n), fold_ref(T, 1, tH, n)

            def run(route, knob, took_exp):
                with knobs(e, knob):
                    Go, Ho, took = fold(T, route, n, tG, tH)
                assert took == took_exp, (k, n, route, knob, took)
                same(Go, exp[0], "G, multiplier %d, n %d, route %d, knobs %s" % (k, n, route, knob))
                same(Ho, exp[1], "H, multiplier %d, n %d, route %d, knobs %s" % (k, n, route, knob))
            run(TAB, {}, K_TAB)
            run(TAB, {T_FOLD_BATCH_MIN: 1}, K_TAB | FINISH)
            run(LADDER, {}, lb)
            run(LADDER, {T_FOLD_BATCH_MIN: 1}, lb | FINISH)
            run(LADDER, {T_FOLD_QUAD_MAX: 512}, lb | QUAD)
            run(LADDER_NAF, {T_FOLD_QUAD_MAX: 512 if k & 1 else 0, T_FOLD_BATCH_MIN: 1 if k & 2 else 65536}, NAF | (QUAD if k & 1 else 0) | (FINISH if k & 2 else 0))
    if T.cv == 1:
        # w = 7: the last window holds bits 252 .. 254 and takes the carry of the window below
        assert e.gens_fold_tables(NTAB, window_bits=7)[0] == 7
        ts = edge_multipliers(T, 7)[-3:]
        for k in range(3):
            Go, Ho, took = fold(T, TAB, 64, ts[k], ts[(k + 1) % 3])
            assert took == K_TAB
            same(Go, fold_ref(T, 0, ts[k], 64), "G, w = 7, multiplier %d" % k)
            same(Ho, fold_ref(T, 1, ts[(k + 1) % 3], 64), "H, w = 7, multiplier %d" % k)


def test_edge_multipliers_two_rounds_from_the_tables(T):
    """the same multipliers as first and second multiplier of k_ipa_fold_tab2 at m = 128 (digits of t1, t2 and t1 * t2), the epilogue
    on for every other pair"""
    e, w, m = T.eng, 8, 128
    assert e.gens_fold_tables(NTAB, window_bits=w)[0] == w
    ts = edge_multipliers(T, w)
    L = len(ts)
    for k in range(L):
        tG, t2G, tH, t2H = ts[k], ts[(k + 1) % L], ts[(k + 1) % L], ts[(k + 2) % L]
        with knobs(e, {T_FOLD_BATCH_MIN: 1 if k & 1 else 65536}):
            Go, Ho, took = fold(T, TAB2, m, tG, tH, t2G, t2H)
        assert took == K_TAB2 | (FINISH if k & 1 else 0)
        same(Go, tab2_ref(T, 0, tG, t2G, m), "G, pair %d" % k)
        same(Ho, tab2_ref(T, 1, tH, t2H, m), "H, pair %d" % k)


# ---- 6: which widths take the tables ---------------------------------------------------------------------------------------------------
def test_which_widths_take_the_tables(T):
    """every width builds and passes the chain-rule check; the fold kernels take a multiplier's digits only when the table has at most
    44 windows (FtabDigits) — w >= 3 on secq256k1, w >= 6 on zorro.  Elsewhere the launcher declines and nothing is written"""
    import ark_bulletproofs_amd as A

    e, n = T.eng, 64
    tG, tH = rand_scalars(T, 6, 2)
    exp = fold_ref(T, 0, tG, n), fold_ref(T, 1, tH, n)
    answered = []
    for w in range(2, 9):
        got_w, nbytes = e.gens_fold_tables(128, window_bits=w)
        assert got_w == w and nbytes == 2 * nwin_of(T.cv, w) * (1 << (w - 1)) * 128 * 64
        assert e.gens_tables_check() == (0, 0)
        Go, Ho, took = fold(T, TAB, n, tG, tH)
        assert took in (0, K_TAB)
        assert (took == K_TAB) == (nwin_of(T.cv, w) <= 44), w
        if took:
            answered.append(w)
            same(Go, exp[0], "G, w = %d" % w)
            same(Ho, exp[1], "H, w = %d" % w)
            Go2, Ho2, took2 = fold(T, TAB2, 32, tG, tH, tH, tG)
            assert took2 == K_TAB2
            same(Go2, tab2_ref(T, 0, tG, tH, 32), "G, two rounds, w = %d" % w)
            same(Ho2, tab2_ref(T, 1, tH, tG, 32), "H, two rounds, w = %d" % w)
        else:
            assert not Go.any() and not Ho.any()
            assert fold(T, TAB2, 32, tG, tH, tH, tG)[2] == 0
    assert answered == ([3, 4, 5, 6, 7, 8] if T.cv == 0 else [6, 7, 8])
    # fewer than 64 outputs per vector: the launcher leaves the round to the ladder; without tables the hook refuses
    assert fold(T, TAB, 32, tG, tH)[2] == 0
    with pytest.raises(A.ArkbpError):
        fold(T, TAB, 129, tG, tH)              # column 128 is not tabled
    with pytest.raises(A.ArkbpError):
        fold(T, TAB2, 43, tG, tH, tH, tG)      # ... nor is element 3 * 43 - 1
    e.gens_fold_tables(0)
    assert e.debug_tables_ptr(0) == (None, 0)
    with pytest.raises(A.ArkbpError):
        fold(T, TAB, n, tG, tH)


# ---- 7: exceptional operands in the table folds ------------------------------------------------------------------------------------------
def first_digit(W, t, w):
    """the first digit of t the table kernels apply — windows upwards, k1's half before k2's — as the factor it multiplies the base by"""
    ds = digits(W, t, w)
    lam = glv(1, W.r)[2] if W.cv == 0 else 1
    for j in range(len(ds[0])):
        for h, half in enumerate(ds):
            if half[j]:
                return half[j] * (1 << (w * j)) * (lam if h else 1) % W.r
    raise AssertionError("no digit")


def test_exceptional_operands_in_the_table_folds(T, oracle):
    """the derived generators with a few replaced by known multiples of the base point, solved so that — in G and in H —
    k_ipa_fold_tab2 (m = 128) meets acc == + entry at the first digit of t2 in lane 0 and acc == - entry in lane 1 (ftab_step's redo
    with a finite accumulator), ends in the identity in lane 2 and adds Gen[3m + 3] to itself in lane 3, and k_ipa_fold_tab ends in the
    identity and in a doubling at n = 64 (lanes 10, 11) and n = 256 (lanes 20, 21).  The lanes around them stay ordinary, so the redo
    diverges inside a wave.  With the in-lane inversion and through k_ipa_fold_finish, where the identity arrives with Z = 0"""
    import ark_bulletproofs_amd as A

    cv, r, w, m = T.cv, T.r, 8, 128
    rnd = random.Random(700 + cv)
    t1 = [rnd.randrange(2, r) for _ in range(2)]      # per vector: the first multiplier (k_ipa_fold_tab's, too) and the second
    t2 = [rnd.randrange(2, r) for _ in range(2)]
    gens = [T.gens[0].copy(), T.gens[1].copy()]
    known = [{}, {}]                                   # per vector: index -> exponent
    for v in (0, 1):
        g = known[v]
        c = first_digit(T, t2[v], w)
        inv1 = pow(t1[v], -1, r)
        for lane, sign in ((0, 1), (1, -1)):           # t1 * g[m + i] = +- c * g[2m + i]
            g[2 * m + lane] = rnd.randrange(1, r)
            g[m + lane] = sign * c * g[2 * m + lane] * inv1 % r
        for lane, sign in ((2, -1), (3, 1)):           # g[3m + i] = +- (t1 g[m + i] + t2 g[2m + i] + t1 t2 g[i])
            for base in (0, m, 2 * m):
                g[base + lane] = rnd.randrange(1, r)
            g[3 * m + lane] = sign * (t1[v] * g[m + lane] + t2[v] * g[2 * m + lane] + t1[v] * t2[v] * g[lane]) % r
        for n, lane in ((64, 10), (256, 20)):          # g[n + i] = -+ t1 g[i]
            g[lane], g[lane + 1] = rnd.randrange(1, r), rnd.randrange(1, r)
            g[n + lane], g[n + lane + 1] = -t1[v] * g[lane] % r, t1[v] * g[lane + 1] % r
        for i, x in g.items():
            gens[v][i] = IM.point_words(cv, IM.mulB(cv, x))
            assert oracle.on_curve(cv, gens[v][i])
    e = A.Engine(curve=cv)
    try:
        e.gens_derive(NG)
        e.gens_upload(gens[0], gens[1])
        assert e.gens_fold_tables(NTAB, window_bits=w)[0] == w
        W = _world(oracle, cv, e, gens[0], gens[1])
        exp2 = [tab2_ref(W, v, t1[v], t2[v], m) for v in (0, 1)]
        exp1 = {n: [fold_ref(W, v, t1[v], n) for v in (0, 1)] for n in (64, 256)}
        for v in (0, 1):                               # the oracle's sums are what the exponents say
            g = known[v]
            assert not exp2[v][2].any() and (exp2[v][3] == IM.point_words(cv, IM.mulB(cv, 2 * g[3 * m + 3]))).all()
            assert exp2[v][[0, 1, 3]].any(axis=1).all()
            for n, lane in ((64, 10), (256, 20)):
                assert not exp1[n][v][lane].any() and (exp1[n][v][lane + 1] == IM.point_words(cv, IM.mulB(cv, 2 * g[n + lane + 1]))).all()
        for batch_min in (65536, 1):
            fin = FINISH if batch_min == 1 else 0
            with knobs(e, {T_FOLD_BATCH_MIN: batch_min}):
                Go, Ho, took = fold(W, TAB2, m, t1[0], t1[1], t2[0], t2[1])
                assert took == K_TAB2 | fin
                same(Go, exp2[0], "two rounds, G, BATCH_MIN %d" % batch_min)
                same(Ho, exp2[1], "two rounds, H, BATCH_MIN %d" % batch_min)
                for n in (64, 256):
                    Go, Ho, took = fold(W, TAB, n, t1[0], t1[1])
                    assert took == K_TAB | fin
                    same(Go, exp1[n][0], "one round, G, n %d, BATCH_MIN %d" % (n, batch_min))
                    same(Ho, exp1[n][1], "one round, H, n %d, BATCH_MIN %d" % (n, batch_min))
    finally:
        e.close()


# ---- 8: the tables follow the installed generators ---------------------------------------------------------------------------------------
def test_tables_follow_the_installed_generators(T, oracle):
    """fold tables and MSM rows are multiples of the resident generators: after bp_gens_upload of other points a table fold, a
    fixed-base MSM, a proof and the chain-rule check are right for the NEW generators — the tables are gone, or rebuilt — and again
    once they are built over them.  bp_gens_derive to a larger capacity extends the same chain and keeps them"""
    import ark_bulletproofs_amd as A

    cv, cap, n = T.cv, 2048, 256
    G0, H0 = oracle.bp_gens(cv, cap)
    G1, H1 = oracle.bp_gens_party(cv, cap, 1)
    assert (G0[0] != G1[0]).any()
    tG, tH = rand_scalars(T, 8, 2)
    sc = oracle.fe_rand(T.FR, bytes([81, cv]) + bytes(30), 2 * cap)
    stmt = (3, [512, 0], 8)                                           # a square chain of 512 multipliers: N = 512, folds from the tables
    e, plain = A.Engine(curve=cv), A.Engine(curve=cv)

    def tuned(x):
        x.set_tuning(T_DIRECT_MAX, 0)                                 # not the small-statement path: the fold schedules
        x.set_tuning(T_IPA_FREEZE_LEN, 16)
        x.set_tuning(T_MSM_FIXED_MIN, 4096)

    def prove(x):
        pr = x.prove_scenario(stmt[0], stmt[1], SEED, m_cap=stmt[2])
        assert x.verify_scenario(stmt[0], stmt[1], pr.proof, pr.commitments, pr.publics) == 0
        return pr.proof

    def table_fold_is_right(W, must_answer):
        try:
            Go, Ho, took = fold(W, TAB, n, tG, tH)
        except A.ArkbpError:
            assert not must_answer and W.eng.debug_tables_ptr(0) == (None, 0) and W.eng.debug_tables_ptr(1) == (None, 0)
            return
        assert took == K_TAB
        same(Go, fold_ref(W, 0, tG, n), "G")
        same(Ho, fold_ref(W, 1, tH, n), "H")
    try:
        tuned(e), tuned(plain)
        e.gens_derive(cap)
        assert e.gens_fold_tables(NTAB, window_bits=8)[0] == 8 and e.gens_msm_tables(cap) == 2 * FB_ROWS * cap * 64
        W0 = _world(oracle, cv, e, G0, H0)
        table_fold_is_right(W0, True)
        runs = e.msm_stats()[0]
        assert (e.msm_gens(cap, sc) == oracle.msm(cv, np.concatenate([G0, H0]), sc)).all() and e.msm_stats()[0] == runs + 1
        defer0 = e.fold_stats()
        assert prove(e) == oracle.r1cs_prove(cv, stmt[0], stmt[1], SEED, cap, m_cap=stmt[2]).proof
        assert e.fold_stats() == (defer0[0] + 1, defer0[1] + 1)       # ... two rounds from the tables
        # other generators: the reference is a ctx that never had tables
        plain.gens_upload(G1, H1)
        ref_proof = prove(plain)
        ref_msm = oracle.msm(cv, np.concatenate([G1, H1]), sc)
        e.gens_upload(G1, H1)
        W1 = _world(oracle, cv, e, G1, H1)
        table_fold_is_right(W1, False)
        assert (e.msm_gens(cap, sc) == ref_msm).all()
        assert prove(e) == ref_proof
        assert e.gens_tables_check() == (0, 0)
        # ... and with tables over them
        assert e.gens_fold_tables(NTAB, window_bits=8)[0] == 8 and e.gens_msm_tables(cap) == 2 * FB_ROWS * cap * 64
        table_fold_is_right(W1, True)
        runs = e.msm_stats()[0]
        assert (e.msm_gens(cap, sc) == ref_msm).all() and e.msm_stats()[0] == runs + 1
        defer0 = e.fold_stats()
        assert prove(e) == ref_proof and e.fold_stats() == (defer0[0] + 1, defer0[1] + 1)
        assert e.gens_tables_check() == (0, 0)
        # the derived chain after caller-installed points: other generators again
        e.gens_derive(cap)
        table_fold_is_right(W0, False)
        assert (e.msm_gens(cap, sc) == oracle.msm(cv, np.concatenate([G0, H0]), sc)).all()
        assert e.gens_tables_check() == (0, 0)
        # a longer chain: the same generators, and the tables stay
        e.gens_derive(NG)
        assert e.gens_fold_tables(NTAB, window_bits=8)[0] == 8 and e.gens_msm_tables(NG) == 2 * FB_ROWS * NG * 64
        ptrs = [e.debug_tables_ptr(k) for k in range(4)]
        e.gens_derive(cap)
        assert [e.debug_tables_ptr(k) for k in range(4)] == ptrs and all(p for p, _ in ptrs)
        assert e.gens_tables_check() == (0, 0)
        table_fold_is_right(W0, True)
    finally:
        plain.close()
        e.close()


# ---- 9: small, with the stepping interface ------------------------------------------------------------------------------------------
def test_small_folds_with_chosen_challenges(T):
    """bp_ipa_begin / round_LR / round_fold / export at n = 8 with the challenges 1, r - 1 and 2 (fold multipliers 1, 1 and 1/4, 4):
    gamma_G * G[i] and gamma_H * H[i] of every round against u^-1 * G_L + u * G_R and u * H_L + u^-1 * H_R by the oracle"""
    O, cv, r, e = T.O, T.cv, T.r, T.eng
    n = 8
    rnd = random.Random(900 + cv)
    G, H = [T.gens[0][i] for i in range(n)], [T.gens[1][i] for i in range(n)]
    Q = T.gens[0][n]
    ints = [[rnd.randrange(1, r) for _ in range(n)] for _ in range(4)]
    Gf, Hf, a, b = [np.array([mont(T, x) for x in xs]) for xs in ints]
    G = [smul(T, P, f) for P, f in zip(G, ints[0])]      # the true vectors: the factors of the first round multiplied in
    H = [smul(T, P, f) for P, f in zip(H, ints[1])]
    e.ipa_begin(Q, Gf, Hf, T.gens[0][:n], T.gens[1][:n], a, b)
    for u in (1, r - 1, 2):
        n //= 2
        ui = pow(u, -1, r)
        e.ipa_round_LR()
        e.ipa_round_fold(mont(T, u))
        G = [O.point_add(cv, smul(T, G[i], ui), smul(T, G[n + i], u)) for i in range(n)]
        H = [O.point_add(cv, smul(T, H[i], u), smul(T, H[n + i], ui)) for i in range(n)]
        _, _, Gx, Hx, gG, gH = e.ipa_export(8)
        assert len(Gx) == n and len(Hx) == n
        same(np.array([O.scalar_mul(cv, P, gG) for P in Gx]), np.array(G), "G after u = %d" % (u if u < 3 else -1))
        same(np.array([O.scalar_mul(cv, P, gH) for P in Hx]), np.array(H), "H after u = %d" % (u if u < 3 else -1))
    e.ipa_finish()
