// Stand-alone check of prove_steps.hpp (pure host code; its own main, no HIP, not loaded into anything): built and run by
// tests/test_prove_steps_host.py with the address and undefined-behaviour sanitizers.  For both curves it records three small
// statements with host::ConstraintSystem — single-phase with 3 multipliers and 2 committed variables, a k = 2 shuffle (no phase-1
// multipliers), two-phase with 3 + 2 multipliers — and compares each shared step with an independent path.
#include <cstdio>
#include <cstring>
#include "host_proto.hpp"
#include "prove_steps.hpp"

using namespace arkbp;
using namespace arkbp::host;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

template <class C> struct Stmt {
    Transcript tr{"prove_steps selftest"};
    ConstraintSystem<C> cs;
    Stmt() { cs.tr = &tr; cs.proving = true; }
    Var commit(u64 v, u64 blind) {
        typedef Fld<typename C::Fr> S;
        cs.v.push_back(S::from_u64(v)); cs.v_blinding.push_back(S::from_u64(blind));
        return Var{VK_COMMITTED, (u32)(cs.v.size() - 1)};
    }
};
template <class C> static LinComb lc2(const Var& a, const F4& ca, const Var& b, const F4& cb) { return LinComb{Term{a, ca}, Term{b, cb}}; }

// three multipliers in phase 1 over two committed variables, +1 / -1 / general coefficients, a committed variable in several
// constraints (wV carries z^(q+1) over gaps of different lengths); with `phase2`, two more multipliers in a randomized phase
template <class C> static void record_gadget(Stmt<C>& s, bool phase2) {
    typedef Fld<typename C::Fr> S;
    typedef ConstraintSystem<C> CS;
    const Var v0 = s.commit(7, 1001), v1 = s.commit(0xFFFFFFFFFFull, 1002), one = Var{VK_ONE, 0};
    const F4 c5 = S::from_u64(5), m1 = S::neg(S::one()), big = S::neg(S::from_u64(123456789));
    Var o[3], p[3], q[3];
    s.cs.multiply(lc2<C>(v0, S::one(), one, c5), lc2<C>(v1, m1, v0, big), o);
    s.cs.multiply(LinComb{Term{o[2], S::one()}}, lc2<C>(v1, c5, one, m1), p);
    s.cs.multiply(lc2<C>(p[0], big, v0, S::one()), LinComb{Term{v1, S::one()}}, q);
    // (satisfiability plays no part in what is checked here: the steps under test never look at it)
    s.cs.constrain(LinComb{Term{q[2], S::one()}, Term{v1, big}, Term{one, c5}});
    s.cs.constrain(LinComb{Term{o[0], m1}, Term{p[1], c5}});
    s.cs.constrain(LinComb{Term{v0, c5}, Term{v1, m1}, Term{q[1], S::one()}});
    if (phase2)
        s.cs.specify_randomized_constraints([v0, v1, q](CS& cs) -> int {
            const F4 z = cs.challenge_scalar("gadget challenge");
            Var a[3], b[3];
            cs.multiply(LinComb{Term{v0, z}, Term{Var{VK_ONE, 0}, S::neg(z)}}, LinComb{Term{q[2], S::one()}}, a);
            cs.multiply(LinComb{Term{a[2], S::one()}}, LinComb{Term{v1, S::sqr(z)}}, b);
            cs.constrain(LinComb{Term{b[2], z}, Term{v1, S::one()}, Term{v0, S::neg(S::one())}});
            return BP_OK;
        });
}
template <class C> static void record_shuffle2(Stmt<C>& s) {
    std::vector<Var> x = {s.commit(3, 11), s.commit(9, 12)}, y = {s.commit(9, 13), s.commit(3, 14)};
    CHECK(shuffle_gadget<C>(s.cs, x, y) == BP_OK);
}

// prove_wv over build_host_csc against cs.flatten's wV
template <class C> static void check_wv(Stmt<C>& s, size_t want_n1, size_t want_n) {
    typedef Fld<typename C::Fr> S;
    CHECK(s.cs.run_randomized() == BP_OK);
    CHECK(s.cs.n1 == want_n1 && s.cs.a_L.size() == want_n);
    HostCsc csc;
    CHECK(build_host_csc<C>(s.cs, csc));
    CHECK(csc.n == want_n && csc.q == s.cs.num_constraints() && !csc.vterms.empty());
    const F4 zs[3] = {S::one(), S::from_u64(2), TP<C>::challenge_scalar(s.tr, "z")};
    for (const F4& z : zs) {
        F4 ztab[32];
        prove_pow_tables<C>(z, z, ztab, nullptr);
        std::vector<F4> wV, wL, wR, wO, wV_ref; F4 wc;
        prove_wv<C>(csc, ztab, s.cs.v.size(), wV);
        s.cs.flatten(z, wL, wR, wO, wV_ref, wc, s.cs.v.size());
        CHECK(wV.size() == wV_ref.size());
        for (size_t i = 0; i < wV.size() && i < wV_ref.size(); i++) CHECK(wV[i] == wV_ref[i]);
    }
}

template <class C> static void check_pow_tables() {
    typedef Fld<typename C::Fr> S;
    Transcript tr("pow tables");
    const F4 z = TP<C>::challenge_scalar(tr, "z"), y = TP<C>::challenge_scalar(tr, "y");
    F4 ztab[32], ypw[64];
    prove_pow_tables<C>(z, y, ztab, ypw);
    F4 cz = z, cy = y;
    for (int k = 0; k < 32; k++) {
        CHECK(ztab[k] == cz && ypw[k] == cy);
        CHECK(S::mul(ypw[k], ypw[32 + k]) == S::one());
        cz = S::mul(cz, cz); cy = S::mul(cy, cy);
    }
    CHECK(S::mul(y, ypw[32]) == S::one());
    F4 only_y[64];
    prove_pow_tables<C>(z, y, nullptr, only_y);
    CHECK(memcmp(only_y, ypw, sizeof ypw) == 0);
}

template <class C> static void check_to_aff() {
    typedef Grp<C> G;
    typedef Fld<typename C::Fr> S;
    const A4 B = PedersenGens<C>::default_ref().B;
    for (size_t len : {(size_t)1, (size_t)3, (size_t)5, (size_t)130}) {
        for (size_t hole : {(size_t)0, len / 2, len - 1, len /* none */}) {
            std::vector<J4> in(len);
            J4 run = G::dbl(G::from_aff(B));
            for (size_t i = 0; i < len; i++) { run = G::add(G::dbl(run), G::from_aff(B)); in[i] = i == hole ? G::inf() : run; }   // (Z != 1 throughout)
            std::vector<A4> out(len), out2(len);
            std::vector<F4> prefix(len);
            to_aff_many<C>(in.data(), len, out.data());
            to_aff_many<C>(in.data(), len, out2.data(), prefix.data());
            for (size_t i = 0; i < len; i++) {
                const A4 ref = G::to_aff(in[i]);
                CHECK(out[i] == ref && out2[i] == ref);
                CHECK((i == hole) == out[i].is_inf());
            }
        }
    }
    // a result record of the table-sum kernels: X | Y | Z words
    const J4 p = G::mul(B, S::from_u64(77));
    u64 rec[12];
    memcpy(rec, p.X.v, 32); memcpy(rec + 4, p.Y.v, 32); memcpy(rec + 8, p.Z.v, 32);
    const J4 back = jac_from_words(rec);
    CHECK(back.X == p.X && back.Y == p.Y && back.Z == p.Z);
}

// the same transcript state twice: equal outputs, equal next challenges; and the draws are the rng's next values in order
template <class C> static void check_t_tail_and_draws() {
    typedef typename C::Fr FrP;
    typedef Fld<FrP> S;
    typedef Grp<C> G;
    Transcript t0("t tail");
    t0.append_u64("m", 2);
    const A4 B = PedersenGens<C>::default_ref().B;
    A4 Tc[5];
    F4 tco[6], tb[5], b1[3], bl2[3];
    for (int i = 0; i < 5; i++) { Tc[i] = G::to_aff(G::mul(B, S::from_u64(3 + i))); tb[i] = TP<C>::challenge_scalar(t0, "tb"); }
    for (int i = 0; i < 6; i++) tco[i] = TP<C>::challenge_scalar(t0, "tco");
    for (int i = 0; i < 3; i++) { b1[i] = TP<C>::challenge_scalar(t0, "b1"); bl2[i] = TP<C>::challenge_scalar(t0, "b2"); }
    const std::vector<F4> wV = {S::from_u64(5), TP<C>::challenge_scalar(t0, "wV")}, vb = {S::from_u64(8), S::from_u64(9)};
    Transcript ta = t0, tb2 = t0;
    F4 a[6], b[6];
    prove_t_tail<C>(ta, Tc, tco, tb, wV, vb, b1, bl2, a[0], a[1], a[2], a[3], a[4], a[5]);
    prove_t_tail<C>(tb2, Tc, tco, tb, wV, vb, b1, bl2, b[0], b[1], b[2], b[3], b[4], b[5]);
    for (int i = 0; i < 6; i++) CHECK(a[i] == b[i]);
    CHECK(TP<C>::challenge_scalar(ta, "next") == TP<C>::challenge_scalar(tb2, "next"));
    // t(x) by the definition: sum t_i x^i
    F4 tx = S::zero(), xp = a[1];
    for (int i = 0; i < 6; i++) { tx = S::add(tx, S::mul(tco[i], xp)); xp = S::mul(xp, a[1]); }
    CHECK(tx == a[2]);
    // a round: L, R in, u out — the same on both copies, and the transcripts stay equal
    CHECK(prove_round_challenge<C>(ta, Tc[0], Tc[1]) == prove_round_challenge<C>(tb2, Tc[0], Tc[1]));

    for (int expanded = 0; expanded < 2; expanded++) {
        TranscriptRng r1(t0), r2(t0);
        const u8 key[32] = {1, 2, 3};
        r1.finalize_bytes(key); r2.finalize_bytes(key);
        F4 d[3], kappa2, t5[5];
        std::vector<F4> sL(3, S::one()), sR(3, S::one());
        prove_draw_phase2<C>(r1, true, expanded != 0, 3, 5, d, kappa2, sL, sR);
        prove_draw_t<C>(r1, t5);
        for (int i = 0; i < 3; i++) CHECK(d[i] == rand_fe<FrP>(r2));
        if (expanded) { CHECK(kappa2 == rand_fe<FrP>(r2) && sL.size() == 3 && sR.size() == 3); }
        else {
            CHECK(sL.size() == 5 && sR.size() == 5 && kappa2.is_zero());
            for (size_t i = 0; i < 3; i++) CHECK(sL[i] == S::one() && sR[i] == S::one());
            for (size_t i = 3; i < 5; i++) CHECK(sL[i] == rand_fe<FrP>(r2));
            for (size_t i = 3; i < 5; i++) CHECK(sR[i] == rand_fe<FrP>(r2));
        }
        for (int i = 0; i < 5; i++) CHECK(t5[i] == rand_fe<FrP>(r2));
        // no second phase: no draws but those of T
        TranscriptRng r3(t0), r4(t0);
        prove_draw_phase2<C>(r3, false, expanded != 0, 3, 3, d, kappa2, sL, sR);
        CHECK(d[0].is_zero() && d[1].is_zero() && d[2].is_zero() && kappa2.is_zero());
        CHECK(rand_fe<FrP>(r3) == rand_fe<FrP>(r4));
    }
    Transcript p1 = t0, p2 = t0;
    prove_append_phase<C>(p1, 1, Tc[0], Tc[1], Tc[2]);
    TP<C>::append_point(p2, "A_I1", Tc[0]); TP<C>::append_point(p2, "A_O1", Tc[1]); TP<C>::append_point(p2, "S1", Tc[2]);
    prove_append_phase<C>(p1, 2, Tc[2], Tc[3], Tc[4]);
    TP<C>::append_point(p2, "A_I2", Tc[2]); TP<C>::append_point(p2, "A_O2", Tc[3]); TP<C>::append_point(p2, "S2", Tc[4]);
    CHECK(TP<C>::challenge_scalar(p1, "c") == TP<C>::challenge_scalar(p2, "c"));
}

// Witness check: the host twin (plain loops over the recorder) against the row index walked the way the kernels walk it: one sum
// per piece, a one-piece row decided there, the partial sums of a longer row added afterwards.  Piece lengths 2, 4 and 256 over a
// statement with rows of 0, 1, 3 and 11 terms; the gadget's own rows are not satisfied, one gate is spoiled on top.
template <class C> static void index_walk(const ConstraintSystem<C>& cs, const HostRowIndex& h, u32 res[4]) {
    typedef Fld<typename C::Fr> S;
    res[0] = res[2] = 0; res[1] = res[3] = 0xFFFFFFFFu;
    for (size_t i = 0; i < h.n; i++) if (!(S::mul(cs.a_L[i], cs.a_R[i]) == cs.a_O[i])) { res[0]++; res[1] = std::min<u32>(res[1], (u32)i); }
    std::vector<F4> partial(h.nslots, S::zero());
    CHECK(h.poff.size() == h.npieces() + 1 && h.tvar.size() == cs.cs_terms.size() && h.tcid.size() == h.tvar.size());
    for (size_t p = 0; p < h.npieces(); p++) {
        F4 acc = S::zero();
        for (u32 e = h.poff[p]; e < h.poff[p + 1]; e++) {
            const u32 kind = h.tvar[e] >> 29, idx = h.tvar[e] & ((1u << 29) - 1), cid = h.tcid[e];
            const F4 val = kind == VK_COMMITTED ? cs.v[idx] : kind == VK_LEFT ? cs.a_L[idx] : kind == VK_RIGHT ? cs.a_R[idx] : kind == VK_OUT ? cs.a_O[idx] : S::one();
            acc = S::add(acc, (cid & CID_ONE) ? val : (cid & CID_MONE) ? S::neg(val) : S::mul(val, h.coefs[cid]));
        }
        if (h.pinfo[p] & HostRowIndex::ROW_LONG) partial[h.pinfo[p] & ~HostRowIndex::ROW_LONG] = acc;
        else if (!acc.is_zero()) { res[2]++; res[3] = std::min(res[3], h.pinfo[p]); }
    }
    for (size_t r = 0; r < h.nlong(); r++) {
        F4 acc = S::zero();
        CHECK(h.lrow[3 * r + 2] <= h.max_pieces && h.lrow[3 * r + 1] + h.lrow[3 * r + 2] <= h.nslots);
        for (u32 j = 0; j < h.lrow[3 * r + 2]; j++) acc = S::add(acc, partial[h.lrow[3 * r + 1] + j]);
        if (!acc.is_zero()) { res[2]++; res[3] = std::min(res[3], h.lrow[3 * r]); }
    }
}
template <class C> static void check_witness() {
    typedef Fld<typename C::Fr> S;
    Stmt<C> s;
    record_gadget<C>(s, false);
    const Var v0{VK_COMMITTED, 0}, one{VK_ONE, 0};
    const F4 m1 = S::neg(S::one());
    s.cs.constrain(LinComb{});
    s.cs.constrain(LinComb{Term{one, S::zero()}});
    LinComb row;
    for (int i = 0; i < 10; i++) row.push_back(Term{v0, i % 2 ? m1 : S::one()});   // cancels
    row.push_back(Term{one, S::zero()});
    s.cs.constrain(row);          // 11 terms, satisfied
    row.back().c = S::from_u64(3);
    s.cs.constrain(row);          // 11 terms, residual 3
    s.cs.a_O[1] = S::add(s.cs.a_O[1], S::one());
    bp_witness_report twin;
    witness_check_host<C>(s.cs, twin);
    CHECK(twin.gates_checked == 3 && twin.constraints_checked == s.cs.cs_off.size() - 1 && twin.bad_gates == 1 && twin.first_bad_gate == 1 && twin.deferred_callbacks == 0);
    CHECK(twin.bad_constraints >= 1);
    for (size_t piece : {(size_t)2, (size_t)4, (size_t)256}) {
        HostRowIndex h;
        CHECK(build_row_index<C>(s.cs, piece, h, [](size_t count, const std::function<void(size_t)>& fn) { for (size_t c = count; c-- > 0;) fn(c); }));
        CHECK((piece == 256) == (h.nlong() == 0));
        u32 res[4];
        index_walk<C>(s.cs, h, res);
        bp_witness_report dev;
        witness_report_from_flags<C>(s.cs, res, dev);
        CHECK(memcmp(&dev, &twin, sizeof dev) == 0);
    }
    HostRowIndex h;
    CHECK(!build_row_index<C>(s.cs, 1, h));
    s.cs.cs_terms[0].v.i = 99;    // a variable nobody handed out: refused, not indexed
    CHECK(!build_row_index<C>(s.cs, 4, h));
}

template <class C> static void run_curve() {
    check_witness<C>();
    { Stmt<C> s; record_gadget<C>(s, false); check_wv<C>(s, 3, 3); }
    { Stmt<C> s; record_shuffle2<C>(s); check_wv<C>(s, 0, 2); }
    { Stmt<C> s; record_gadget<C>(s, true); check_wv<C>(s, 3, 5); }
    check_pow_tables<C>();
    check_to_aff<C>();
    check_t_tail_and_draws<C>();
}

int main() {
    run_curve<Secq>();
    run_curve<Zorro>();
    printf(g_fail ? "prove_steps selftest: %d check(s) FAILED\n" : "prove_steps selftest ok\n", g_fail);
    return g_fail ? 1 : 0;
}
