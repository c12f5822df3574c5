// Stand-alone check of the `base` form of prove_steps.hpp's constraint indices (pure host code; its own main, no HIP, not loaded into
// anything): built and run by tests/test_prover_like_cpu.py with the address and undefined-behaviour sanitizers.  A prover that shares
// a frozen phase-1 recording (ConstraintSystem::base, bp_prover_new_like) and records further constraints of its own must index to
// exactly what the same constraints recorded flat give: HostCsc and HostRowIndex field by field, at n = 1, 3, 257 multipliers, on
// both curves; the recording's once-built indices equal the flat ones of phase 1 alone; the host witness check reads both alike.
#include <cstdio>
#include <cstring>
#include "host_proto.hpp"
#include "prove_steps.hpp"

using namespace arkbp;
using namespace arkbp::host;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

// phase 1: n multipliers chained through their outputs over two committed variables, coefficients +1, -1 and general ones (two of
// them repeated: the coefficient table de-duplicates), a long row (more terms than the piece of 4 used below) when n allows
template <class C> static void record_phase1(ConstraintSystem<C>& cs, size_t n) {
    typedef Fld<typename C::Fr> S;
    const Var v0{VK_COMMITTED, 0}, v1{VK_COMMITTED, 1}, one{VK_ONE, 0};
    const F4 m1 = S::neg(S::one());
    Var prev = v0;
    LinComb all;
    for (size_t i = 0; i < n; i++) {
        const F4 c = S::from_u64(3 + i % 5);
        Var o[3];
        cs.multiply(LinComb{Term{prev, S::one()}, Term{one, c}}, LinComb{Term{v1, i % 2 ? m1 : c}, Term{v0, S::one()}}, o);
        prev = o[2];
        if (i < 9) all.push_back(Term{o[i % 3], i % 2 ? m1 : S::from_u64(1000 + i)});
    }
    cs.constrain(all);
    cs.constrain(LinComb{Term{prev, S::one()}, Term{v1, S::from_u64(4)}, Term{one, m1}});
}
// what the instance records itself (a randomized phase's worth): two multipliers and two constraints that reach back into phase 1
template <class C> static void record_own(ConstraintSystem<C>& cs, const F4& z) {
    typedef Fld<typename C::Fr> S;
    const Var v0{VK_COMMITTED, 0}, v1{VK_COMMITTED, 1}, one{VK_ONE, 0};
    Var a[3], b[3];
    cs.multiply(LinComb{Term{v0, z}, Term{one, S::neg(z)}}, LinComb{Term{Var{VK_OUT, 0}, S::one()}}, a);
    cs.multiply(LinComb{Term{a[2], S::one()}}, LinComb{Term{v1, S::sqr(z)}, Term{Var{VK_LEFT, 0}, S::from_u64(4)}}, b);
    cs.constrain(LinComb{Term{b[2], z}, Term{v1, S::one()}, Term{v0, S::neg(S::one())}, Term{a[0], z}, Term{a[1], S::one()}, Term{b[0], S::from_u64(3)}});
    cs.constrain(LinComb{});
}
template <class C> static void commit2(ConstraintSystem<C>& cs) {
    typedef Fld<typename C::Fr> S;
    cs.v = {S::from_u64(7), S::from_u64(0xFFFFFFFFFFull)}; cs.v_blinding = {S::from_u64(1001), S::from_u64(1002)};
}

static bool same_csc(const HostCsc& a, const HostCsc& b) {
    bool ok = a.n == b.n && a.q == b.q && a.moff == b.moff && a.ment == b.ment && a.mc == b.mc && a.coefs.size() == b.coefs.size() && a.vterms.size() == b.vterms.size();
    for (size_t i = 0; ok && i < a.coefs.size(); i++) ok = a.coefs[i] == b.coefs[i];
    for (size_t i = 0; ok && i < a.vterms.size(); i++) ok = a.vterms[i].j == b.vterms[i].j && a.vterms[i].q == b.vterms[i].q && a.vterms[i].c == b.vterms[i].c;
    return ok;
}
static bool same_row(const HostRowIndex& a, const HostRowIndex& b) {
    bool ok = a.n == b.n && a.q == b.q && a.m == b.m && a.poff == b.poff && a.pinfo == b.pinfo && a.tvar == b.tvar && a.tcid == b.tcid && a.lrow == b.lrow &&
              a.nslots == b.nslots && a.max_pieces == b.max_pieces && a.coefs.size() == b.coefs.size();
    for (size_t i = 0; ok && i < a.coefs.size(); i++) ok = a.coefs[i] == b.coefs[i];
    return ok;
}
static bool same_report(const bp_witness_report& a, const bp_witness_report& b) { return memcmp(&a, &b, sizeof a) == 0; }

template <class C> static void check_size(size_t n) {
    typedef Fld<typename C::Fr> S;
    Transcript tr("prove_like selftest");
    const F4 z = TP<C>::challenge_scalar(tr, "z");
    const size_t PIECE = 4;
    // flat: one prover records everything itself
    ConstraintSystem<C> flat; flat.tr = &tr; flat.proving = true;
    commit2(flat);
    record_phase1(flat, n);
    // source: records phase 1, is frozen; like: shares it and takes the witness as two vectors
    ConstraintSystem<C> src; src.tr = &tr; src.proving = true;
    commit2(src);
    record_phase1(src, n);
    CHECK(src.freeze(false) == BP_E_ARG && !src.base);          // (the verifier's form refuses a prover, nothing frozen)
    CHECK(src.freeze(true) == BP_OK && src.base && src.own_empty());
    CHECK(src.freeze(true) == BP_OK);                            // a second freeze shares the same recording
    CHECK(src.num_constraints() == flat.num_constraints() && src.num_terms() == flat.num_terms());
    ConstraintSystem<C> like; like.tr = &tr;
    like.init_like_prover(src);
    commit2(like);
    CHECK(like.base == src.base && like.num_vars == n && like.proving && like.like && !like.assigned);
    like.assign_multipliers(flat.a_L.data(), flat.a_R.data(), n);
    CHECK(like.assigned && like.aO_lazy && like.a_O.empty());

    // phase 1 alone: the recording's once-built indices, the like-prover's and the frozen source's own all equal the flat ones
    HostCsc c_flat, c_src, c_like;
    CHECK(build_host_csc<C>(flat, c_flat) && build_host_csc<C>(src, c_src) && build_host_csc<C>(like, c_like));
    CHECK(same_csc(c_flat, c_src) && same_csc(c_flat, c_like));
    const auto c_shared = shared_host_csc<C>(*src.base);
    CHECK(c_shared && same_csc(c_flat, *c_shared) && shared_host_csc<C>(*like.base).get() == c_shared.get());
    HostRowIndex r_flat, r_src, r_like;
    CHECK(build_row_index<C>(flat, PIECE, r_flat) && build_row_index<C>(src, PIECE, r_src) && build_row_index<C>(like, PIECE, r_like));   // (the like-prover's a_O is still lazy)
    CHECK(same_row(r_flat, r_src) && same_row(r_flat, r_like));
    if (n >= 9) CHECK(r_flat.nlong() >= 1);
    const auto r_shared = shared_row_index<C>(*src.base, 2, PIECE);
    CHECK(r_shared && same_row(r_flat, *r_shared) && shared_row_index<C>(*like.base, 2, PIECE).get() == r_shared.get());
    CHECK(!shared_row_index<C>(*like.base, 3, PIECE));           // another number of commitments: not the shared one

    // the host twin: lazily materialised a_O is the product, the reports agree; a poked a_O is seen
    like.materialise_aO();
    CHECK(!like.aO_lazy && like.a_O.size() == n);
    for (size_t i = 0; i < n; i++) CHECK(like.a_O[i] == flat.a_O[i]);
    bp_witness_report w_flat, w_src, w_like;
    witness_check_host<C>(flat, w_flat); witness_check_host<C>(src, w_src); witness_check_host<C>(like, w_like);
    CHECK(same_report(w_flat, w_src) && same_report(w_flat, w_like));
    CHECK(w_flat.gates_checked == n && w_flat.constraints_checked == flat.num_constraints() && w_flat.bad_gates == 0);
    like.a_O[n - 1] = S::add(like.a_O[n - 1], S::one()); flat.a_O[n - 1] = S::add(flat.a_O[n - 1], S::one());
    witness_check_host<C>(flat, w_flat); witness_check_host<C>(like, w_like);
    CHECK(same_report(w_flat, w_like) && w_like.bad_gates == 1 && w_like.first_bad_gate == n - 1);
    like.a_O[n - 1] = S::sub(like.a_O[n - 1], S::one()); flat.a_O[n - 1] = S::sub(flat.a_O[n - 1], S::one());

    // base + own terms against the same constraints recorded flat
    record_own(flat, z); record_own(like, z); record_own(src, z);
    CHECK(like.num_constraints() == flat.num_constraints() && like.num_vars == n + 2 && !like.own_empty());
    HostCsc d_flat, d_like, d_src;
    CHECK(build_host_csc<C>(flat, d_flat) && build_host_csc<C>(like, d_like) && build_host_csc<C>(src, d_src));
    CHECK(same_csc(d_flat, d_like) && same_csc(d_flat, d_src) && d_flat.n == n + 2);
    HostRowIndex s_flat, s_like;
    CHECK(build_row_index<C>(flat, PIECE, s_flat) && build_row_index<C>(like, PIECE, s_like));
    CHECK(same_row(s_flat, s_like) && s_flat.q == flat.num_constraints());
    for (size_t q = 0; q < flat.num_constraints(); q++) CHECK(witness_row_value<C>(flat, q) == witness_row_value<C>(like, q));
    witness_check_host<C>(flat, w_flat); witness_check_host<C>(like, w_like);
    CHECK(same_report(w_flat, w_like));
    // the shared indices did not move
    CHECK(same_csc(c_flat, *shared_host_csc<C>(*like.base)) && same_row(r_flat, *shared_row_index<C>(*like.base, 2, PIECE)));
    // flatten walks base + own the same way
    std::vector<F4> aL, aR, aO, aV, bL, bR, bO, bV; F4 ac, bc;
    flat.flatten(z, aL, aR, aO, aV, ac, 2); like.flatten(z, bL, bR, bO, bV, bc, 2);
    CHECK(aL.size() == bL.size() && ac == bc);
    for (size_t i = 0; i < aL.size() && i < bL.size(); i++) CHECK(aL[i] == bL[i] && aR[i] == bR[i] && aO[i] == bO[i]);
    for (size_t i = 0; i < 2; i++) CHECK(aV[i] == bV[i]);
}

template <class C> static void check_curve() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)257}) check_size<C>(n);
}

int main() {
    check_curve<Secq>();
    check_curve<Zorro>();
    if (g_fail) { printf("prove_like selftest: %d failure(s)\n", g_fail); return 1; }
    printf("prove_like selftest ok\n");
    return 0;
}
