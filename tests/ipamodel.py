"""`InnerProductProof::create` in the exponent, for tests that choose the generators: every generator is a known multiple g_i * B of
one base point B and the challenges are given, so the whole recursion is linear arithmetic mod r and each output point costs one
scalar multiplication.  Python integers and tests/pymodel.py only.  A test can then solve for g_i that make a fold round meet a
chosen relation (equal, opposite or identity operands) — data that random inputs never produce."""
import numpy as np

import pymodel as M

R = 1 << 256


def mont_words(x, p):
    """x as the C ABI holds a field element: 4 x u64 of x * 2^256 mod p"""
    v = x * R % p
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def from_mont_words(w, p):
    return sum(int(v) << (64 * i) for i, v in enumerate(np.asarray(w).reshape(-1)[:4])) * pow(R, -1, p) % p


def point_words(cv, P):
    """affine point (or None = the identity: all zero) as 8 x u64"""
    if P is None:
        return np.zeros(8, dtype=np.uint64)
    q = M.CURVES[cv]["q"]
    return np.concatenate([mont_words(P[0], q), mont_words(P[1], q)])


def point_from_words(cv, w):
    w = np.asarray(w, dtype=np.uint64).reshape(8)
    if not w.any():
        return None
    q = M.CURVES[cv]["q"]
    return from_mont_words(w[:4], q), from_mont_words(w[4:], q)


_TABLES = {}


def mulB(cv, k):
    """k * B for the curve's generator B, from a table of d * 16^j * B (64 additions)"""
    c = M.CURVES[cv]
    if cv not in _TABLES:
        rows, P = [], (c["gx"], c["gy"])
        for _ in range(64):
            row = [None, P]
            for _ in range(14):
                row.append(M.add(cv, row[-1], P))
            rows.append(row)
            P = M.add(cv, row[15], P)
        _TABLES[cv] = rows
    k %= c["r"]
    acc = None
    for j in range(64):
        acc = M.add(cv, acc, _TABLES[cv][j][(k >> (4 * j)) & 15])
    return acc


def ipa_create(cv, qe, Gf, Hf, g, h, a, b, us):
    """src/inner_product_proof.rs InnerProductProof::create with G[i] = g[i] * B, H[i] = h[i] * B, Q = qe * B and the challenges us:
    returns (L exponents, R exponents, a, b), all integers mod r; L_j = Ls[j] * B"""
    r = M.CURVES[cv]["r"]
    n = len(g)
    assert n & (n - 1) == 0 and all(len(x) == n for x in (Gf, Hf, h, a, b)) and len(us) == max(n.bit_length() - 1, 0)
    g, h, a, b = list(g), list(h), list(a), list(b)
    Ls, Rs = [], []
    first = True
    for u in us:
        n //= 2
        ui = pow(u, -1, r)
        fG = Gf if first else [1] * (2 * n)
        fH = Hf if first else [1] * (2 * n)
        cL = sum(a[i] * b[n + i] for i in range(n))
        cR = sum(a[n + i] * b[i] for i in range(n))
        Ls.append((sum(a[i] * fG[n + i] * g[n + i] + b[n + i] * fH[i] * h[i] for i in range(n)) + cL * qe) % r)
        Rs.append((sum(a[n + i] * fG[i] * g[i] + b[i] * fH[n + i] * h[n + i] for i in range(n)) + cR * qe) % r)
        g = [(ui * fG[i] * g[i] + u * fG[n + i] * g[n + i]) % r for i in range(n)]
        h = [(u * fH[i] * h[i] + ui * fH[n + i] * h[n + i]) % r for i in range(n)]
        a, b = [(a[i] * u + ui * a[n + i]) % r for i in range(n)], [(b[i] * ui + u * b[n + i]) % r for i in range(n)]
        first = False
    return Ls, Rs, a[0], b[0]
