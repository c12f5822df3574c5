"""Test gadgets written ONCE against the reference's ConstraintSystem trait shape (src/r1cs/constraint_system.rs:19-135) and run
on both recorders: the product's (ark_bulletproofs_amd.engine.ProverCS / VerifierCS over the C ABI) and the oracle's
(oracle.pyoracle.ProverCS / VerifierCS).  None of them is one of the product's built-in scenarios.

A "program" is a random sparse constraint system, satisfiable by construction: its STRUCTURE comes from one seed (so several
instances share it), its witness from another.  With `two_phase` it adds randomized constraints whose coefficients depend on a
transcript challenge (the shape of the reference's shuffle gadget, benches/r1cs_secq256k1.rs:47-76)."""
import random

VAR_COMMITTED, VAR_MULT_LEFT, VAR_MULT_RIGHT, VAR_MULT_OUT, VAR_ONE = 0, 1, 2, 3, 4
ONE = (VAR_ONE, 0)


class Field:
    """scalar-field helper: python ints <-> 4 x u64 Montgomery words (conversion by the oracle: test infrastructure)"""

    def __init__(self, O, curve):
        self.O, self.fid = O, O.fid(curve, True)
        self.p = O.modulus(self.fid)
        self._cache = {}

    def w(self, x):
        x %= self.p
        r = self._cache.get(x)
        if r is None:
            r = self._cache[x] = self.O.fe_from_int(self.fid, x)
        return r

    def i(self, words):
        return self.O.fe_to_int(self.fid, words)


class Witness:
    """values of the variables a prover-side run has seen (None on the verifier side)"""

    def __init__(self, F):
        self.F, self.val = F, {ONE: 1}

    def eval(self, lc):
        return sum(c * self.val[v] for v, c in lc) % self.F.p


def random_program(cs, F, struct_seed, wit, committed_vars, n_mul=12, n_alloc=3, n_extra=6, two_phase=False, n_mul2=5, publics=None, dense_coefs=True):
    """Records a random satisfiable circuit on `cs`.  wit: Witness (prover) or None (verifier).  publics: list the prover run fills
    with the public constants it derives (ints) and the verifier run reads back in the same order.  Returns nothing: all state is
    in cs / publics."""
    rs = random.Random(struct_seed)
    proving = wit is not None
    pub_iter = iter(publics) if (publics is not None and not proving) else None
    pool = list(committed_vars) + [ONE]

    def coef():
        t = rs.random()
        if t < 0.35:
            return 1
        if t < 0.55:
            return F.p - 1
        if t < 0.75 or not dense_coefs:
            return rs.randrange(2, 50)
        return rs.randrange(F.p)

    def rand_lc(maxlen=3):
        return [(rs.choice(pool), coef()) for _ in range(rs.randint(1, maxlen))]

    def W(lc):
        return [(v, F.w(c)) for v, c in lc]

    def mul(left, right):
        l, r, o = cs.multiply(W(left), W(right))
        if proving:
            wit.val[l], wit.val[r] = wit.eval(left), wit.eval(right)
            wit.val[o] = wit.val[l] * wit.val[r] % F.p
        pool.extend([l, r, o])
        return l, r, o

    def pin(lc):
        """a satisfiable constraint on lc without a public constant: bind it to a fresh allocated variable"""
        val = wit.eval(lc) if proving else None
        x = cs.allocate(F.w(val) if proving else None)
        if proving:
            wit.val[x] = val
        pool.append(x)
        cs.constrain(W(lc + [(x, F.p - 1)]))

    for _ in range(n_mul):
        mul(rand_lc(), rand_lc())
    for _ in range(n_alloc):   # allocate_multiplier with explicit inputs
        a, b = (rs.randrange(F.p), rs.randrange(1 << 20))
        l, r, o = cs.allocate_multiplier((F.w(a), F.w(b)) if proving else None)
        if proving:
            wit.val[l], wit.val[r], wit.val[o] = a, b, a * b % F.p
        pool.extend([l, r, o])
    for j in range(n_extra):
        lc = rand_lc(4)
        if j % 2 == 0:
            pin(lc)
        else:     # lc - c = 0 with a PUBLIC constant c (differs per instance: the per-instance coefficient-table path)
            if proving:
                c = wit.eval(lc)
                publics.append(c)
            else:
                c = next(pub_iter)
            cs.constrain(W(lc + [(ONE, (F.p - c) % F.p)]))
    if two_phase:
        snapshot = list(pool)
        seed2 = rs.randrange(1 << 30)

        def randomized(cs2):
            r2 = random.Random(seed2)
            z = F.i(cs2.challenge_scalar(b"gadget challenge"))
            pool2 = list(snapshot)

            def coef2():
                t = r2.random()
                return 1 if t < 0.3 else F.p - 1 if t < 0.5 else z if t < 0.7 else (F.p - z) % F.p if t < 0.85 else (z * z + r2.randrange(5)) % F.p

            def lc2(maxlen=3):
                return [(r2.choice(pool2), coef2()) for _ in range(r2.randint(1, maxlen))]

            for _ in range(n_mul2):
                left, right = lc2(), lc2()
                l, r, o = cs2.multiply(W(left), W(right))
                if proving:
                    wit.val[l], wit.val[r] = wit.eval(left), wit.eval(right)
                    wit.val[o] = wit.val[l] * wit.val[r] % F.p
                pool2.extend([l, r, o])
            for _ in range(3):
                lc = lc2(4)
                val = wit.eval(lc) if proving else None
                x = cs2.allocate(F.w(val) if proving else None)
                if proving:
                    wit.val[x] = val
                pool2.append(x)
                cs2.constrain(W(lc + [(x, F.p - 1)]))

        cs.specify_randomized_constraints(randomized)


def rare_shapes_program(cs, F, wit, committed_vars, two_phase=False, summary=None):
    """A deterministic satisfiable circuit whose flattened constraints reach the shapes random_program does not: multiplier columns
    (the entries of columns i of W_L, W_R, W_O together) with 0, 6, 7 and 20 or more entries spread over the three matrices, +1 / -1 /
    general coefficients, a constraint naming one variable twice, a constraint naming a_L[i] and a_O[i], more than 256 constraints
    with long columns at constraint indices 254, 255 and 256, more constant terms than twice the padded size, a committed variable
    in 30 or more constraints; with `two_phase` the same shapes among the randomized phase's multipliers.  No public constants:
    every witness of it is a like-instance of every other.  committed_vars: three or more.

    The extra constraints restate relations that multiply() recorded (c * (left - a_L[i]) + d * (right - a_R[i]) = 0 and the like),
    so they hold for any witness.  `summary`: a dict the run fills with the shape counts, taken from the terms as recorded."""
    proving = wit is not None
    V0, V1, V2 = committed_vars[:3]
    cons = []        # every constraint as recorded, multiply()'s own included: [(var, coefficient as int)]
    muls = []        # multiplier index -> phase (1 or 2)

    def W(lc):
        return [(v, F.w(c)) for v, c in lc]

    def constrain(c, lc):
        cons.append(lc)
        c.constrain(W(lc))

    def mul(c, phase, left, right):
        l, r, o = c.multiply(W(left), W(right))
        if proving:
            wit.val[l], wit.val[r] = wit.eval(left), wit.eval(right)
            wit.val[o] = wit.val[l] * wit.val[r] % F.p
        cons.append(left + [(l, F.p - 1)])
        cons.append(right + [(r, F.p - 1)])
        muls.append(phase)
        return (l, r, o), left + [(l, F.p - 1)], right + [(r, F.p - 1)]

    def unused(c, phase):     # a multiplier no constraint names: a column with no entries
        a, b = 5 + 7 * len(muls), 11
        l, r, o = c.allocate_multiplier((F.w(a), F.w(b)) if proving else None)
        if proving:
            wit.val[l], wit.val[r], wit.val[o] = a, b, a * b % F.p
        muls.append(phase)

    def comb(*parts):         # sum of c * (a relation that is zero for every witness)
        return [(v, c * x % F.p) for c, zl in parts for v, x in zl]

    def build(c, phase, w):
        """w: the phase's general coefficient (a constant in phase 1, the gadget challenge in phase 2)"""
        m1 = F.p - 1
        hub, zl, zr = mul(c, phase, [(V0, 1), (ONE, 2)], [(V1, 3), (V2, m1)])            # the long column
        h7, zl7, zr7 = mul(c, phase, [(V0, w), (ONE, 4)], [(V2, 1)])                     # 7 entries
        h6, zl6, zr6 = mul(c, phase, [(V1, m1), (ONE, 9)], [(V0, 1), (V1, w)])           # 6 entries
        ch, zo, _ = mul(c, phase, [(hub[2], 1)], [(V1, 1)])                              # a_O[hub] = a_L[ch]
        _, zo7, _ = mul(c, phase, [(h7[2], 1)], [(ONE, 3)])                              # a_O[h7] = a_L[..]
        unused(c, phase)
        fill, zlf, _ = mul(c, phase, [(V0, 1), (V2, w), (ONE, 6)], [(V1, 1)])            # carries the bulk of the constraints
        mul(c, phase, [(V2, 1)], [(V0, 1)])
        # 7 = 3 (own) + 4: a_L with a_O of the same multiplier in one constraint, then a_L and a_R
        constrain(c, comb((1, zl7), (m1, zo7)))
        constrain(c, comb((w, zl7), (5, zr7)))
        # 6 = 2 (own) + 4
        constrain(c, comb((m1, zl6), (w, zr6)))
        constrain(c, comb((1, zl6), (1, zr6)))
        # the hub: a_L named twice in one constraint, a_L with a_O, a_L with a_R
        l0 = hub[0]
        constrain(c, [(V0, 7), (ONE, 14), (l0, F.p - 3), (l0, F.p - 4)])
        constrain(c, comb((m1, zl), (1, zo)))
        for j in range(8):
            constrain(c, comb(((1, m1, w, 3 + j)[j % 4], zl), ((w, 1, m1, 2)[j % 4], zr)))
        return hub, fill, zl, zr, zlf

    hub, fill, zl, zr, zlf = build(cs, 1, 12345)
    mul(cs, 1, [(V1, 1)], [(V2, 1)])     # (9 phase-1 multipliers, 17 in all: padded sizes 16 and 32 with padding lanes)
    # bulk: constraints over the fill column (a constant term and V0 in each) up to constraint index 253, then the hub and the
    # fill column at 254, 255, 256, then some more
    while len(cons) < 254:
        constrain(cs, comb((3 + len(cons), zlf)))
    constrain(cs, comb((1, zl), (F.p - 1, zr)))
    constrain(cs, comb((2, zl), (5, zlf)))
    constrain(cs, comb((F.p - 1, zl), (1, zlf), (7, zr)))
    for j in range(40):
        constrain(cs, comb((9 + j, zlf)))
    n1_cons = len(cons)

    def randomized(cs2):
        z = F.i(cs2.challenge_scalar(b"rare shapes challenge"))
        _, _, zl2, zr2, zlf2 = build(cs2, 2, z)
        for j in range(24):
            constrain(cs2, comb(((z + j) % F.p, zlf2), ((1, F.p - 1)[j % 2], zl2)))
        constrain(cs2, comb((z, zl2), (1, zr2)))
        if summary is not None:
            _summarize(summary, F, cons, muls, committed_vars)

    if two_phase:
        cs.specify_randomized_constraints(randomized)
    elif summary is not None:
        _summarize(summary, F, cons, muls, committed_vars)
    if summary is not None:
        summary["phase1_constraints"] = n1_cons


def _summarize(summary, F, cons, muls, committed_vars):
    """shape counts of a recorded circuit (what the flattened W_L / W_R / W_O / W_V / constants hold)"""
    n = len(muls)
    n1 = sum(1 for p in muls if p == 1)
    cols = [dict(L=0, R=0, O=0, q=set()) for _ in range(n)]
    names = {VAR_MULT_LEFT: "L", VAR_MULT_RIGHT: "R", VAR_MULT_OUT: "O"}
    coefs, twice, lo_same, n_const = set(), False, False, 0
    committed = {tuple(v): 0 for v in committed_vars}
    for q, lc in enumerate(cons):
        seen = set()
        for v, c in lc:
            v = tuple(v)
            twice |= v in seen
            seen.add(v)
            coefs.add("+1" if c == 1 else "-1" if c == F.p - 1 else "general")
            if v[0] in names:
                cols[v[1]][names[v[0]]] += 1
                cols[v[1]]["q"].add(q)
            elif v[0] == VAR_ONE:
                n_const += 1
        for v in set(tuple(v) for v, _ in lc):
            if v in committed:
                committed[v] += 1
        lo_same |= any((VAR_MULT_LEFT, i) in seen and (VAR_MULT_OUT, i) in seen for i in range(n))
    N = 1
    while N < n:
        N *= 2
    summary.update(n=n, n1=n1, N=N, constraints=len(cons), constants=n_const, coefs=coefs, twice=twice, lo_same=lo_same,
                   committed_max=max(committed.values()),
                   columns=[(i, c["L"] + c["R"] + c["O"], sum(1 for k in "LRO" if c[k]), sorted(c["q"])) for i, c in enumerate(cols)])


def make_witness(F, wit_seed, m):
    rw = random.Random(wit_seed)
    vals = [rw.randrange(F.p) if j % 2 else rw.randrange(1 << 32) for j in range(m)]
    blinds = [rw.randrange(F.p) for _ in range(m)]
    return vals, blinds
