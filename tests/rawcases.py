"""Case list and reference for the raw-representative unit ops (csrc/dbg_raw.cuh): one list, run on the CPU build of the device
headers with every contract asserted (tests/test_fp29_host.py) and on the GPU (tests/test_gpu_group_law.py).

The device holds a field element as nine 29-bit limbs that stand for ANY representative of the residue: limbs may exceed 2^29
(L = largest limb / 2^29) and the value may exceed p (V = value / p) within the contracts of csrc/fp29.cuh.  Seeded random inputs
through the C ABI only ever produce canonical representatives, so the cases here are built limb by limb: products at the contract
limit, every multiple of p and its neighbours, and Jacobian points whose coordinates are taken in [0, p) or in [p, 2p).

The reference is Python integers and tests/pymodel.py, nothing from the library: a field result is checked as value and as limbs,
a Jacobian result as the affine point the test converts it to itself, the identity as "Z limbs all zero"."""
import random

import pymodel as M

M29 = (1 << 29) - 1
# op numbers of csrc/dbg_raw.cuh
F_MUL, F_SQR, F_MUL2, F_SUB2, F_SUB4, F_SUB8, F_SUB16, F_WRED, F_CANON, F_NORM, F_ZERO, F_EQ, F_PACK = range(13)
P_ADD, P_MADD, P_DBL, P_MADD_FAST, P_QADD, P_QMADD, P_QDBL = range(7)
SUB_K = {F_SUB2: 2, F_SUB4: 4, F_SUB8: 8, F_SUB16: 16}


def field(fid):
    """fid = 2 * curve + (0 base field | 1 scalar field).  The scalar fields are pseudo-Mersenne and hold plain residues (R' = 1);
    the base fields hold x * 2^261 mod p."""
    c = M.CURVES[fid >> 1]
    p = c["r"] if fid & 1 else c["q"]
    pm = bool(fid & 1)
    return dict(p=p, pm=pm, Rp=1 if pm else 1 << 261, bits=p.bit_length())


def limbs(x):
    """the normalised limbs of 0 <= x < 2^261"""
    assert 0 <= x < (1 << 261)
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def val(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def lazy(L, top):
    """limbs 0..7 at L * 2^29, limb 8 = top"""
    return [L << 29] * 8 + [top]


def lazy_at(L, V, p):
    """limbs 0..7 at L * 2^29 and limb 8 as large as keeps the value <= V * p and the limb <= L * 2^29"""
    low = val(lazy(L, 0))
    return lazy(L, min(L << 29, (V * p - low) >> 232))


def subk(K, p):
    """the borrow-free offset of fe_sub<K>: the normalised limbs of K * p, each of limbs 0..7 raised by 4 * 2^29 = 2^31 that the limb
    above gives up (4 units).  Derived here, not read from the generated header."""
    n = limbs(K * p)
    return [n[i] + (1 << 31) * (i < 8) - 4 * (i > 0) for i in range(9)]


# ---- field cases ---------------------------------------------------------------------------------------------------------------
def field_cases(fid):
    """[(op, name, [a, b, c, d] as limb lists)]"""
    f = field(fid)
    p = f["p"]
    rnd = random.Random(1000 + fid)
    Z = [0] * 9
    out = []

    def add(op, name, a, b=Z, c=Z, d=Z):
        out.append((op, name, [list(a), list(b), list(c), list(d)]))

    # products at the contract limit: L(a) L(b) = 6 with limbs 0..7 at the maximum, V(a) V(b) <= 900 (30 * 30)
    for La, Lb in ((2, 3), (3, 2), (1, 6), (6, 1)):
        add(F_MUL, "mul L %dx%d V 30x30" % (La, Lb), lazy_at(La, 30, p), lazy_at(Lb, 30, p))
        add(F_MUL, "mul L %dx%d V small" % (La, Lb), lazy(La, 0), lazy(Lb, 0))
    add(F_SQR, "sqr L 2 V 30", lazy_at(2, 30, p))
    add(F_SQR, "sqr L 2 V small", lazy(2, 0))
    # fe_mul2: L(a)L(b) + L(c)L(d) = 6, V(a)V(b) + V(c)V(d) <= 900 (2 * 21 * 21 = 882)
    for La, Lb, Lc, Ld in ((2, 1, 2, 2), (3, 1, 3, 1), (1, 3, 1, 3), (2, 2, 1, 2)):
        add(F_MUL2, "mul2 L %d*%d+%d*%d V 21" % (La, Lb, Lc, Ld), *[lazy_at(L, 21, p) for L in (La, Lb, Lc, Ld)])
    for i in range(8):
        x = [limbs(rnd.randrange(2 * p)) for _ in range(4)]
        add(F_MUL, "mul random %d" % i, x[0], x[1])
        add(F_SQR, "sqr random %d" % i, x[0])
        add(F_MUL2, "mul2 random %d" % i, *x)
    # every multiple of p below 2^261 and its neighbours: zero tests, canonical form, weak reduction
    for k in range(32):
        for dname, dv in (("", 0), ("+1", 1), ("-1", -1), ("+2^29", 1 << 29), ("-2^29", -(1 << 29)), ("+2^232", 1 << 232), ("-2^232", -(1 << 232)),
                          ("+p/2", p >> 1)):
            v = k * p + dv
            if not 0 <= v < (1 << 261):
                continue
            for op in (F_ZERO, F_CANON, F_WRED):
                add(op, "%d*p%s" % (k, dname), limbs(v))
    # the largest outputs of the weak reduction: p = 2^B +- delta, and fe_wred takes off (a >> B) (- 1) times p, so the values just
    # below a multiple of 2^B keep the most — the inputs on which fe_canon has the most left to subtract.  The precondition of
    # fe_wred / fe_canon / the zero tests is a < 2^261 (csrc/fp29.cuh): k runs to 31 for the 256-bit moduli and to 63 for the 255-bit ones
    B = (p + (p >> 1)).bit_length() - 1
    for k in range(1, 64):
        for dname, dv in (("-1", -1), ("", 0)):
            v = (k << B) + dv
            if v < (1 << 261):
                for op in (F_ZERO, F_CANON, F_WRED):
                    add(op, "%d*2^%d%s" % (k, B, dname), limbs(v))
    add(F_WRED, "2^261-1", limbs((1 << 261) - 1))
    add(F_CANON, "2^261-1", limbs((1 << 261) - 1))
    add(F_NORM, "norm L 2 every limb", lazy(2, 2 << 29))
    add(F_NORM, "norm random lazy", [rnd.randrange(1 << 31) for _ in range(8)] + [rnd.randrange(1 << 24)])
    # fe_sub<K>: a at L = 2 in every limb; b random, and b at the real limit (csrc/fp29.cuh): limb-wise b[i] = SUBK<K>[i], and the
    # largest normalised b (limbs 0..7 full, limb 8 = floor(K p / 2^232) - 4)
    for op, K in SUB_K.items():
        a2 = lazy(2, 2 << 29)
        s = subk(K, p)
        add(op, "sub<%d> a L2, b random" % K, a2, limbs(rnd.randrange(K * p - (1 << 235))))
        add(op, "sub<%d> a L2, b lazy random" % K, a2, [rnd.randrange(s[i] + 1) for i in range(9)])
        add(op, "sub<%d> a L2, b at the limb-wise limit" % K, a2, s)
        add(op, "sub<%d> a L2, b largest normalised" % K, a2, [M29] * 8 + [s[8]])
        add(op, "sub<%d> a 0, b largest normalised" % K, Z, [M29] * 8 + [s[8]])
        add(op, "sub<%d> a random, b random" % K, limbs(rnd.randrange(2 * p)), limbs(rnd.randrange(p)))
    # fe_eq_mod(a, b) = is_zero(a - b + 16 p): the same residue under different multiples of p, and near misses
    for i in range(3):
        x = rnd.randrange(p)
        for ja in (0, 1, 3, 14):
            for jb in (0, 1, 7, 14):
                add(F_EQ, "eq x+%dp, x+%dp" % (ja, jb), limbs(x + ja * p), limbs(x + jb * p))
                add(F_EQ, "eq x+%dp+1, x+%dp" % (ja, jb), limbs(x + ja * p + 1), limbs(x + jb * p))
        add(F_EQ, "eq x, y", limbs(x), limbs(rnd.randrange(p)))
    for name, v in (("2^256-1", (1 << 256) - 1), ("p-1", p - 1), ("0", 0), ("random", rnd.randrange(1 << 256))):
        add(F_PACK, "pack " + name, limbs(v))
    return out


def is_L1(l, top_bits=32):
    return all(0 <= int(v) < (1 << 29) for v in l[:8]) and 0 <= int(l[8]) < (1 << top_bits)


def check_field(fid, op, name, ins, out):
    """asserts what the op must return for these input limbs; out = the 18 words of RAW_F_OUT"""
    f = field(fid)
    p, Rp = f["p"], f["Rp"]
    a, b, c, d = (val(x) for x in ins)
    out = [int(v) for v in out]
    r = val(out[:9])
    tag = "field %d: %s" % (fid, name)
    if op in (F_MUL, F_SQR, F_MUL2):
        prod = a * b if op == F_MUL else a * a if op == F_SQR else a * b + c * d
        assert is_L1(out[:9]), tag
        assert (r * Rp - prod) % p == 0, tag
        if f["pm"]:
            assert r < (1 << f["bits"]) + (1 << 78), tag           # fp29.cuh: "the result is < 2^BITS + 2^78"
        else:
            assert r * (1 << 261) < prod + p * (1 << 261), tag     # (a b + m p) / 2^261 with m < 2^261; implies V < V(a)V(b)/32 + 1
    elif op in SUB_K:
        assert is_L1(out[:9]) and r == a + SUB_K[op] * p - b, tag
    elif op == F_WRED:
        assert is_L1(out[:9], 29) and (r - a) % p == 0 and r < 2 * p, tag       # strictly: ONE subtraction then gives the canonical value
        if f["pm"]:
            assert r < (1 << f["bits"]) + (1 << 40), tag
    elif op == F_CANON:
        assert out[:9] == limbs(a % p), tag
    elif op == F_NORM:
        assert is_L1(out[:9]) and r == a, tag
    elif op == F_ZERO:
        zero = a % p == 0
        assert out[0] == int(zero), tag + ": fe_is_zero_mod"
        assert out[1] in (0, 1) and (out[1] == 1 or not zero), tag + ": fe_maybe_zero_mod misses a zero"
    elif op == F_EQ:
        assert out[0] == int((a - b) % p == 0), tag
    elif op == F_PACK:
        assert out[:9] == ins[0] and sum(out[9 + i] << (32 * i) for i in range(8)) == a, tag
    else:
        raise AssertionError("unknown op")
    assert all(v == 0 for v in out[{F_ZERO: 2, F_EQ: 1, F_PACK: 17}.get(op, 9):]), tag


# ---- point cases ---------------------------------------------------------------------------------------------------------------
REPS = [(i & 1, (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]     # X, Y, Z each in [0, p) (0) or in [p, 2p) (1)


def point_cases(cv):
    """[(op, name, P (27 limbs), Q (27 limbs), kind, expected affine point or None)]; kind: "same", "opp", "inf" (an operand is the
    identity) or "other" — what jac_madd_fast's rare flag must cover"""
    c = M.CURVES[cv]
    q = c["q"]
    Rp = 1 << 261
    rnd = random.Random(2000 + cv)
    G = (c["gx"], c["gy"])
    pts = [M.mul(cv, G, rnd.randrange(1, c["r"])) for _ in range(3)]
    neg = lambda P: (P[0], (-P[1]) % q)   # noqa: E731
    ONE = limbs(Rp % q)

    def jac(P, rep):
        """P under a random lambda, the coordinates' Montgomery residues taken in [0, q) or [q, 2q)"""
        if P is None:
            return ONE + ONE + [0] * 9
        lam = rnd.randrange(1, q)
        co = (P[0] * lam * lam, P[1] * lam ** 3, lam)
        return sum((limbs(v * Rp % q + hi * q) for v, hi in zip(co, rep)), [])

    def aff(P, k):
        """canonical x, y + k q (k = 1, 2: what a lazy negation leaves)"""
        if P is None:
            return [0] * 27
        return limbs(P[0] * Rp % q) + limbs(P[1] * Rp % q + k * q) + [0] * 9

    out = []
    n = 0
    for ra in REPS:
        for rb in REPS:
            P, O = pts[n % 3], pts[(n + 1) % 3]
            n += 1
            for kind, Q in (("same", P), ("opp", neg(P)), ("other", O)):
                for op in (P_ADD, P_QADD):
                    out.append((op, "add %s %s%s" % (kind, ra, rb), jac(P, ra), jac(Q, rb), kind, M.add(cv, P, Q)))
        P = pts[n % 3]
        for op in (P_ADD, P_QADD):
            out.append((op, "add P + inf %s" % (ra,), jac(P, ra), jac(None, ra), "inf", P))
            out.append((op, "add inf + P %s" % (ra,), jac(None, ra), jac(P, ra), "inf", P))
        for op in (P_DBL, P_QDBL):
            for P in pts * 3:        # three lambdas per point: 72 cases, more than the 64 quads of a block
                out.append((op, "dbl %s" % (ra,), jac(P, ra), jac(None, ra), "same", M.add(cv, P, P)))
        for k in (0, 1, 2):
            P, O = pts[n % 3], pts[(n + 1) % 3]
            n += 1
            for op in (P_MADD, P_MADD_FAST, P_QMADD):
                for kind, Q in (("same", P), ("opp", neg(P)), ("other", O)):
                    out.append((op, "madd %s %s y+%dq" % (kind, ra, k), jac(P, ra), aff(Q, k), kind, M.add(cv, P, Q)))
                out.append((op, "madd inf + Q y+%dq" % k, jac(None, ra), aff(P, k), "inf", P))
        for op in (P_MADD, P_MADD_FAST, P_QMADD):
            out.append((op, "madd P + inf %s" % (ra,), jac(pts[0], ra), aff(None, 0), "inf", pts[0]))
    for op in (P_ADD, P_QADD, P_DBL, P_QDBL, P_MADD, P_MADD_FAST, P_QMADD):
        out.append((op, "inf (+ inf)", jac(None, None), jac(None, None) if op in (P_ADD, P_QADD, P_DBL, P_QDBL) else aff(None, 0), "inf", None))
    return out


def to_affine(cv, w):
    """27 raw limbs X | Y | Z -> affine point as integers, None for the identity (Z limbs all zero)"""
    q = M.CURVES[cv]["q"]
    Ri = pow(1 << 261, -1, q)
    X, Y, Z = (val(w[9 * i:9 * i + 9]) * Ri % q for i in range(3))
    if all(int(v) == 0 for v in w[18:27]):
        return None
    assert Z != 0, "Z = 0 (mod q) with non-zero limbs: neither the identity nor a point"
    zi = pow(Z, -1, q)
    return X * zi * zi % q, Y * zi ** 3 % q


def check_point(cv, op, name, kind, expect, lanes):
    """lanes: (1 or 4, 28) result words.  Every lane equals the reference; the lanes of a quad agree limb for limb; stored
    coordinates have limbs 0..7 < 2^29 and V <= 2.25 (the largest the formulas document: Z3 = 2 * (Y * Z) of the quad doubling,
    a product of two V <= 2 operands, < 4 / 32 + 1, doubled)."""
    q = M.CURVES[cv]["q"]
    tag = "curve %d op %d: %s" % (cv, op, name)
    lanes = [[int(v) for v in l] for l in lanes]
    assert len(lanes) == (4 if op >= P_QADD else 1), tag
    for l in lanes[1:]:
        assert l == lanes[0], tag + ": the lanes of the quad differ"
    w = lanes[0]
    if op == P_MADD_FAST:
        if kind != "other":
            assert w[27] == 1, tag + ": rare not set"
        if w[27] == 1:
            return           # the caller redoes the addition with jac_madd; the fast result is meaningless
    else:
        assert w[27] == 0, tag
    got = to_affine(cv, w)
    assert got == expect, tag
    if got is not None:
        for i in range(3):
            co = w[9 * i:9 * i + 9]
            assert is_L1(co, 29) and 4 * val(co) <= 9 * q, tag + ": coordinate %d out of its bounds" % i
