"""Helpers of the witness-check tests (test_witness_check_cpu.py, test_gpu_witness_check.py): a recording proxy that keeps, in
Python integers, every row and every assignment a gadget puts into a ProverCS — the model the reports are compared with — and a
few small programs."""
import gadgets as GD

NONE = (1 << 64) - 1
LABEL = b"WitnessCheckTest"


class Model:
    """rows: every constraint as recorded, multiply's two included, in order: [(var, coefficient int)]; val: var -> int"""

    def __init__(self, F):
        self.F, self.rows, self.val, self.n = F, [], {GD.ONE: 1}, 0
        self.pending = None

    def row_value(self, q):
        return sum(c * self.val[tuple(v)] for v, c in self.rows[q]) % self.F.p

    def bad_rows(self):
        return [q for q in range(len(self.rows)) if self.row_value(q)]

    def bad_gates(self):
        p = self.F.p
        return [i for i in range(self.n) if self.val[(1, i)] * self.val[(2, i)] % p != self.val[(3, i)]]

    def expect(self, deferred=0):
        """(gates_checked, constraints_checked, bad_gates, first_bad_gate, bad_constraints, first_bad_constraint, deferred, residual)"""
        g, r = self.bad_gates(), self.bad_rows()
        return (self.n, len(self.rows), len(g), g[0] if g else NONE, len(r), r[0] if r else NONE, deferred, self.row_value(r[0]) if r else 0)


def observed(F, rep):
    t = rep.astuple()
    return t[:7] + (F.i(rep.first_bad_residual),)


class Recorder:
    """a ProverCS seen through the ConstraintSystem calls gadgets make, mirrored into a Model"""

    def __init__(self, cs, model):
        self.cs, self.m = cs, model

    def _ints(self, lc):
        return [(tuple(v), self.m.F.i(c)) for v, c in lc]

    def _eval(self, lc):
        return sum(c * self.m.val[v] for v, c in self._ints(lc)) % self.m.F.p

    def multiply(self, left, right):
        l, r, o = self.cs.multiply(left, right)
        m = self.m
        m.val[l], m.val[r] = self._eval(left), self._eval(right)
        m.val[o] = m.val[l] * m.val[r] % m.F.p
        m.rows.append(self._ints(left) + [(l, m.F.p - 1)])
        m.rows.append(self._ints(right) + [(r, m.F.p - 1)])
        m.n += 1
        return l, r, o

    def allocate(self, assignment=None):
        x = self.cs.allocate(assignment)
        m = self.m
        if m.pending is None:
            m.pending = x[1]
            m.val[x], m.val[(2, x[1])], m.val[(3, x[1])] = m.F.i(assignment), 0, 0
            m.n += 1
        else:
            m.pending = None
            m.val[x] = m.F.i(assignment)
            m.val[(3, x[1])] = m.val[(1, x[1])] * m.val[x] % m.F.p
        return x

    def allocate_multiplier(self, assignments=None):
        l, r, o = self.cs.allocate_multiplier(assignments)
        m = self.m
        m.val[l], m.val[r] = m.F.i(assignments[0]), m.F.i(assignments[1])
        m.val[o] = m.val[l] * m.val[r] % m.F.p
        m.n += 1
        return l, r, o

    def constrain(self, lc):
        self.cs.constrain(lc)
        self.m.rows.append(self._ints(lc))

    def challenge_scalar(self, label):
        return self.cs.challenge_scalar(label)

    def specify_randomized_constraints(self, fn):
        def run(cs2):
            self.m.pending = None     # (the randomized phase starts a fresh allocate pair)
            fn(Recorder(cs2, self.m))

        self.cs.specify_randomized_constraints(run)


def new_prover(E, curve, F, vals, blinds, engine=None):
    """a ProverCS with `vals` committed, its Model and Recorder, the committed variables"""
    t = E.HostTranscript(LABEL)
    t.append_message(b"dom-sep", b"witness check v1")
    p = E.ProverCS(curve, t)
    V, vars_ = p.commit([F.w(v) for v in vals], [F.w(b) for b in blinds], engine=engine)
    m = Model(F)
    for var, v in zip(vars_, vals):
        m.val[var] = v % F.p
    return p, m, Recorder(p, m), vars_, V


def random_prover(E, curve, F, struct_seed, wit_seed, two_phase, engine=None, **kw):
    vals, blinds = GD.make_witness(F, wit_seed, 3)
    p, m, rec, vars_, V = new_prover(E, curve, F, vals, blinds, engine)
    wit = GD.Witness(F)
    for var, v in zip(vars_, vals):
        wit.val[var] = v
    pubs = []
    GD.random_program(rec, F, struct_seed, wit, vars_, two_phase=two_phase, publics=pubs, **kw)
    return p, m, V, pubs


def poke(E, p, m, vec, index, value):
    """spoil one assignment in the prover and in the model; vec 0 a_L, 1 a_R, 2 a_O, 3 v"""
    E.debug_poke_witness(p, vec, index, m.F.w(value))
    m.val[((1, 2, 3, 0)[vec], index)] = value % m.F.p


def shuffle_gadget(cs, F, x, y):
    """the reference's k-shuffle (benches/r1cs_secq256k1.rs:34-76), k >= 2: two-phase, every constraint in the randomized phase"""
    k = len(x)
    p = F.p

    def rnd(c):
        z = F.i(c.challenge_scalar(b"shuffle challenge"))

        def mz(v):
            return [(v, F.w(1)), (GD.ONE, F.w(p - z))]

        def chain(vs):
            prev = c.multiply(mz(vs[k - 1]), mz(vs[k - 2]))[2]
            for i in range(k - 3, -1, -1):
                prev = c.multiply([(prev, F.w(1))], mz(vs[i]))[2]
            return prev

        fx = chain(x)
        fy = chain(y)
        c.constrain([(fx, F.w(1)), (fy, F.w(p - 1))])

    cs.specify_randomized_constraints(rnd)


def shuffle_prover(E, curve, F, k, permuted, engine=None):
    """a k-shuffle prover whose outputs are a rotation of its inputs (permuted) or have one value changed (not a permutation)"""
    ins = [1000 + 17 * i for i in range(k)]
    outs = ins[1:] + ins[:1]
    if not permuted:
        outs[0] += 1
    blinds = [5 + i for i in range(2 * k)]
    p, m, rec, vars_, V = new_prover(E, curve, F, ins + outs, blinds, engine)
    shuffle_gadget(rec, F, vars_[:k], vars_[k:])
    return p, m, V


def shuffle_verifier(E, curve, F, k, V):
    t = E.HostTranscript(LABEL)
    t.append_message(b"dom-sep", b"witness check v1")
    v = E.VerifierCS(curve, t)
    vars_ = v.commit(V)
    shuffle_gadget(v, F, vars_[:k], vars_[k:])
    return v
