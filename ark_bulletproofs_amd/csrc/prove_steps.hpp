// The host steps of Prover::prove (src/r1cs/prover.rs:454-831) that both prover routes take, each written once: r1cs_prove
// (r1cs_host.inc, one proof on the ctx's workspaces) and the groups of bp_prover_prove_batch (prove_batch.inc, inside their pool
// lambdas).  Pure host code on host_proto.hpp / host_math.hpp: no HIP, no ctx, compiles with a plain C++17 compiler
// (prove_steps_selftest.cpp).  The ORDER of the TranscriptRng draws and of the transcript operations is the reference's: the proofs
// are byte-identical to it.
#pragma once
#include "host_proto.hpp"

namespace arkbp {
namespace host {

// Merged CSC of a recorded constraint system (see k_r1cs_flatten): built on the host, once per statement — with the statement for
// single-phase circuits (outside prove()), after the randomized phase otherwise.
struct HostCsc {
    size_t n = 0, q = 0;
    std::vector<u32> moff, ment, mc;   // n+1 offsets; (vector << 30) | constraint; coefficient id with the +-1 flags in bits 31 / 30
    std::vector<F4> coefs;
    std::vector<VTerm> vterms;   // committed-variable terms in constraint order: feed wV (t_2's blinding, prover.rs:716-721)
};
// The index of `base` (a shared phase-1 recording, may be null) followed by the Q own constraints of (terms, off): what the same
// constraints recorded flat give, entry by entry.  n: multipliers.
template <class C> static bool build_host_csc_parts(const FrozenRecording* base, const Term* terms, const size_t* off, size_t Qown, size_t n, HostCsc& h) {
    typedef Fld<typename C::Fr> S;
    const size_t Qb = base ? base->nq() : 0, Q = Qb + Qown;
    if (Q >= ((size_t)1 << 30) || n >= ((size_t)1 << 31)) return false;
    h.n = n; h.q = Q;
    reserve_huge(h.moff, n + 1);
    h.moff.assign(n + 1, 0);
    auto vec_of = [](int k) { return k == VK_LEFT ? 0 : k == VK_RIGHT ? 1 : k == VK_OUT ? 2 : -1; };
    bool ok = true;
    auto count = [&](const Term* t, size_t cnt) { for (size_t k = 0; k < cnt; k++) if (vec_of(t[k].v.k) >= 0) { if (t[k].v.i < n) h.moff[t[k].v.i + 1]++; else ok = false; } };
    if (base) count(base->terms.data(), base->terms.size());
    count(terms, off[Qown]);
    if (!ok) return false;
    for (size_t i = 0; i < n; i++) h.moff[i + 1] += h.moff[i];
    reserve_huge(h.ment, h.moff[n]); reserve_huge(h.mc, h.moff[n]);
    h.ment.resize(h.moff[n]); h.mc.resize(h.moff[n]);
    std::vector<u32> cur;
    reserve_huge(cur, n + 1);
    cur.assign(h.moff.begin(), h.moff.end() - 1);
    const F4 one = S::one(), mone = S::neg(S::one());
    CanonState st;
    // constraints in order: every column's run comes out sorted by q
    auto put = [&](size_t q, const Term& t, u32 cid) {
        const int v = vec_of(t.v.k);
        if (t.v.k == VK_COMMITTED) h.vterms.push_back(VTerm{t.v.i, (u32)q, t.c});
        if (v < 0) return;   // (the constant terms enter wc, which the prover does not use)
        if (!(cid & (CID_ONE | CID_MONE)) && cid >= (1u << 30)) ok = false;
        const u32 pos = cur[t.v.i]++;
        h.ment[pos] = ((u32)v << 30) | (u32)q;
        h.mc[pos] = cid;
    };
    if (base) st.walk(base->terms.data(), base->off.data(), Qb, 0, one, mone, put);
    st.walk(terms, off, Qown, Qb, one, mone, put);
    h.coefs.swap(st.coefs);
    if (h.coefs.empty()) h.coefs.push_back(one);
    return ok;
}
template <class C> static bool build_host_csc(const ConstraintSystem<C>& cs, HostCsc& h) {
    if (!cs.deferred.empty()) return false;
    return build_host_csc_parts<C>(cs.base.get(), cs.cs_terms.data(), cs.cs_off.data(), cs.cs_off.size() - 1, cs.num_vars, h);
}
// the index of a shared recording alone: built by the first prover that asks, under the recording's once-flag (null: cannot be indexed)
template <class C> static std::shared_ptr<const HostCsc> shared_host_csc(const FrozenRecording& f) {
    std::call_once(f.csc_once, [&] {
        auto h = std::make_shared<HostCsc>();
        const size_t none[1] = {0};
        if (build_host_csc_parts<C>(&f, nullptr, none, 0, f.num_vars, *h)) f.csc = h;
    });
    return f.csc;
}

// ---- witness check (include/arkbp.h: bp_prover_check; the kernels: witness_check.cuh) -----------------------------------------------
// The constraints by ROW, the recorder's own order (cs_terms / cs_off), for the device: every row cut into pieces of at most `piece`
// terms.  poff: npieces + 1 term offsets; pinfo[p]: the row a one-piece row's piece belongs to, or ROW_LONG | partial slot for a piece
// of a longer row; tvar: (kind << 29) | index; tcid: coefficient id in HostCsc's convention (a de-duplicated table, +-1 as flags, no
// product for them); lrow: (row, first partial slot, pieces) per long row.
struct HostRowIndex {
    static constexpr u32 ROW_LONG = 0x80000000u;
    size_t n = 0, q = 0, m = 0;
    std::vector<u32> poff, pinfo, tvar, tcid, lrow;
    std::vector<F4> coefs;
    size_t nslots = 0;       // partial sums of all long rows
    u32 max_pieces = 0;      // most pieces of one row
    size_t nlong() const { return lrow.size() / 3; }
    size_t npieces() const { return pinfo.size(); }
};
// par(count, fn): fn(0) .. fn(count - 1) in any order, possibly on several threads (null: here, one after the other).  The result does
// not depend on it: coefficients other than +-1 are numbered in a second, sequential pass, in order of first occurrence.
typedef std::function<void(size_t, const std::function<void(size_t)>&)> RowIndexPar;
// (the core: Q constraints flat in (terms, off), n multipliers, m committed variables)
template <class C> static bool build_row_index_flat(const Term* terms, const size_t* off, size_t Q, size_t n, size_t m, size_t piece, HostRowIndex& h, const RowIndexPar& par) {
    typedef Fld<typename C::Fr> S;
    const size_t nt = off[Q];
    if (piece < 2 || n >= ((size_t)1 << 29) || m >= ((size_t)1 << 29) || Q >= ((size_t)1 << 30) || nt >= ((size_t)1 << 31)) return false;
    h = HostRowIndex();
    h.n = n; h.q = Q; h.m = m;
    auto run = [&](size_t count, const std::function<void(size_t)>& fn) { if (par && count > 1) par(count, fn); else for (size_t c = 0; c < count; c++) fn(c); };
    reserve_huge(h.tvar, nt); reserve_huge(h.tcid, nt);
    h.tvar.resize(nt); h.tcid.resize(nt);
    const F4 one = S::one(), mone = S::neg(S::one());
    static constexpr size_t CHUNK = (size_t)1 << 16;
    static constexpr u32 GENERAL = 0x3fffffffu;   // pass 1's mark of a coefficient that still needs its number (never a valid id: ids stay below 2^30 - 1)
    const size_t tchunks = (nt + CHUNK - 1) / CHUNK, qchunks = (Q + CHUNK - 1) / CHUNK;
    std::vector<u8> bad(tchunks, 0), general(tchunks, 0), longrow(qchunks, 0);
    run(tchunks, [&](size_t c) {
        for (size_t k = c * CHUNK, hi = std::min(nt, k + CHUNK); k < hi; k++) {
            const Term& t = terms[k];
            const size_t lim = t.v.k == VK_COMMITTED ? m : t.v.k <= VK_OUT ? n : 0;
            if (t.v.k != VK_ONE && t.v.i >= lim) bad[c] = 1;   // a variable the recorder never handed out
            h.tvar[k] = ((u32)t.v.k << 29) | (t.v.k == VK_ONE ? 0u : t.v.i);
            if (t.c == one) h.tcid[k] = CID_ONE; else if (t.c == mone) h.tcid[k] = CID_MONE; else { h.tcid[k] = GENERAL; general[c] = 1; }
        }
    });
    CanonState st;   // (its coefficient numbering only)
    for (size_t c = 0; c < tchunks; c++) {
        if (bad[c]) return false;
        if (!general[c]) continue;
        for (size_t k = c * CHUNK, hi = std::min(nt, k + CHUNK); k < hi; k++) {
            if (h.tcid[k] != GENERAL) continue;
            const u32 id = st.id_of(terms[k].c);
            if (id >= GENERAL) return false;
            h.tcid[k] = id;
        }
    }
    run(qchunks, [&](size_t c) { for (size_t q = c * CHUNK, hi = std::min(Q, q + CHUNK); q < hi; q++) if (off[q + 1] - off[q] > piece) longrow[c] = 1; });
    bool any_long = false;
    for (size_t c = 0; c < qchunks; c++) any_long |= longrow[c] != 0;
    if (!any_long) {   // every row is one piece (an empty row is one empty piece: sum 0, satisfied)
        reserve_huge(h.poff, Q + 1); reserve_huge(h.pinfo, Q);
        h.poff.resize(Q + 1); h.pinfo.resize(Q);
        h.poff[0] = 0;
        run(qchunks, [&](size_t c) { for (size_t q = c * CHUNK, hi = std::min(Q, q + CHUNK); q < hi; q++) { h.pinfo[q] = (u32)q; h.poff[q + 1] = (u32)off[q + 1]; } });
    } else {
        reserve_huge(h.poff, Q + nt / piece + 2); reserve_huge(h.pinfo, Q + nt / piece + 1);
        h.poff.push_back(0);
        for (size_t q = 0; q < Q; q++) {
            const size_t lo = off[q], hi = off[q + 1], len = hi - lo;
            const size_t np = len <= piece ? 1 : (len + piece - 1) / piece;
            if (np == 1) { h.pinfo.push_back((u32)q); h.poff.push_back((u32)hi); continue; }
            if (h.nslots + np >= HostRowIndex::ROW_LONG) return false;
            h.lrow.push_back((u32)q); h.lrow.push_back((u32)h.nslots); h.lrow.push_back((u32)np);
            for (size_t p = 0; p < np; p++) { h.pinfo.push_back(HostRowIndex::ROW_LONG | (u32)(h.nslots + p)); h.poff.push_back((u32)std::min(hi, lo + (p + 1) * piece)); }
            h.nslots += np;
            h.max_pieces = std::max<u32>(h.max_pieces, (u32)np);
        }
    }
    h.coefs.swap(st.coefs);
    if (h.coefs.empty()) h.coefs.push_back(one);
    return true;
}
// An instance's index: its own constraints; behind a shared recording (ConstraintSystem::base) the recording's rows first — copied in
// front of the own ones, so that the result is what the same constraints recorded flat give.  (A like-prover that recorded nothing
// itself uses the recording's own index instead: shared_row_index, no copy.)
template <class C> static bool build_row_index(const ConstraintSystem<C>& cs, size_t piece, HostRowIndex& h, const RowIndexPar& par = nullptr) {
    const size_t n = cs.mults();
    if (!cs.dev.held() && (cs.a_R.size() != n || (!cs.aO_lazy && cs.a_O.size() != n))) return false;
    if (!cs.base) return build_row_index_flat<C>(cs.cs_terms.data(), cs.cs_off.data(), cs.cs_off.size() - 1, n, cs.v.size(), piece, h, par);
    const FrozenRecording& f = *cs.base;
    std::vector<Term> terms;
    std::vector<size_t> off;
    reserve_huge(terms, f.terms.size() + cs.cs_terms.size()); reserve_huge(off, f.off.size() + cs.cs_off.size());
    terms.insert(terms.end(), f.terms.begin(), f.terms.end()); terms.insert(terms.end(), cs.cs_terms.begin(), cs.cs_terms.end());
    off.insert(off.end(), f.off.begin(), f.off.end());
    for (size_t q = 1; q < cs.cs_off.size(); q++) off.push_back(f.terms.size() + cs.cs_off[q]);
    return build_row_index_flat<C>(terms.data(), off.data(), off.size() - 1, n, cs.v.size(), piece, h, par);
}
// the index of a shared recording alone for provers that hold m commitments (like-provers of one recording hold the same number: one
// that differs gets null and builds its own): once per recording
template <class C> static std::shared_ptr<const HostRowIndex> shared_row_index(const FrozenRecording& f, size_t m, size_t piece, const RowIndexPar& par = nullptr) {
    std::call_once(f.row_once, [&] {
        auto h = std::make_shared<HostRowIndex>();
        if (build_row_index_flat<C>(f.terms.data(), f.off.data(), f.nq(), f.num_vars, m, piece, *h, par)) { f.row = h; f.row_m = m; }
    });
    return f.row && f.row_m == m && f.row->n == f.num_vars ? f.row : nullptr;
}
// the value of row q's combination (ark words)
template <class C> static F4 witness_row_value(const ConstraintSystem<C>& cs, size_t q) {
    const Term* p; size_t cnt;
    cs.row(q, p, cnt);
    return cs.eval(p, cnt);
}
// The host twin: plain loops over the recorder with the host field.  What the kernels are tested against, and what a NULL or host-only
// ctx runs.
template <class C> static void witness_check_host(const ConstraintSystem<C>& cs, bp_witness_report& r) {
    typedef Fld<typename C::Fr> S;
    memset(&r, 0, sizeof r);
    const size_t n = cs.a_L.size(), Q = cs.num_constraints();
    r.gates_checked = n; r.constraints_checked = Q; r.deferred_callbacks = cs.deferred.size();
    r.first_bad_gate = r.first_bad_constraint = ~(uint64_t)0;
    for (size_t i = 0; i < n; i++)
        if (!(S::mul(cs.a_L[i], cs.a_R[i]) == cs.a_O[i])) { if (!r.bad_gates++) r.first_bad_gate = i; }
    for (size_t q = 0; q < Q; q++) {
        const F4 s = witness_row_value<C>(cs, q);
        if (s.is_zero()) continue;
        if (!r.bad_constraints++) { r.first_bad_constraint = q; memcpy(r.first_bad_residual, s.v, 32); }
    }
}
// a device result (bad gates, first, bad constraints, first) as a report; the residual comes from the recorder
template <class C> static void witness_report_from_flags(const ConstraintSystem<C>& cs, const u32 res[4], bp_witness_report& r) {
    memset(&r, 0, sizeof r);
    r.gates_checked = cs.a_L.size(); r.constraints_checked = cs.num_constraints(); r.deferred_callbacks = cs.deferred.size();
    r.bad_gates = res[0]; r.first_bad_gate = res[0] ? res[1] : ~(uint64_t)0;
    r.bad_constraints = res[2]; r.first_bad_constraint = res[2] ? res[3] : ~(uint64_t)0;
    if (res[2] && res[3] < cs.num_constraints()) { const F4 s = witness_row_value<C>(cs, res[3]); memcpy(r.first_bad_residual, s.v, 32); }
}

// ztab[j] = z^(2^j); ypw[k] = y^(2^k), ypw[32 + k] = y^-(2^k): ONE inversion.  A null table is left out.
template <class C> static void prove_pow_tables(const F4& z, const F4& y, F4* ztab /* [32] */, F4* ypw /* [64] */) {
    typedef Fld<typename C::Fr> S;
    if (ztab) { F4 c = z; for (int j = 0; j < 32; j++) { ztab[j] = c; c = S::sqr(c); } }
    if (ypw) { F4 c = y, ci = S::inv(y); for (int k = 0; k < 32; k++) { ypw[k] = c; ypw[32 + k] = ci; c = S::sqr(c); ci = S::sqr(ci); } }
}

// wV (prover.rs:385-387) from the index: the few terms on the nv committed variables, z^(q+1) carried from term to term
template <class C> static void prove_wv(const HostCsc& csc, const F4* ztab /* [32] */, size_t nv, std::vector<F4>& wV) {
    typedef Fld<typename C::Fr> S;
    wV.assign(nv, S::zero());
    auto pow_z = [&](u32 e) { F4 r = S::one(); for (u32 j = 0; e; e >>= 1, j++) if (e & 1) r = S::mul(r, ztab[j]); return r; };
    F4 zq = S::one(), zstep = S::one();
    u32 cur = 0, last_d = 0;
    for (const VTerm& t : csc.vterms) {
        const u32 q1 = t.q + 1;
        if (cur == 0) zq = pow_z(q1);
        else if (q1 != cur) { const u32 d = q1 - cur; if (d != last_d) { zstep = pow_z(d); last_d = d; } zq = S::mul(zq, zstep); }
        cur = q1;
        wV[t.j] = S::sub(wV[t.j], S::mul(zq, t.c));
    }
}

// The draws after the randomized phase (prover.rs:585-602): i_b2, o_b2, s_b2 when the phase has multipliers, then the phase's
// blinding vectors s_L[n1 .. n), s_R[n1 .. n) — or, expanded, the ONE key they come from on the device, drawn where they would begin.
template <class C> static void prove_draw_phase2(TranscriptRng& rng, bool has2, bool expanded, size_t n1, size_t n, F4 bl2[3], F4& kappa2, std::vector<F4>& s_L, std::vector<F4>& s_R) {
    typedef typename C::Fr FrP;
    bl2[0] = bl2[1] = bl2[2] = kappa2 = Fld<FrP>::zero();
    if (has2) { bl2[0] = rand_fe<FrP>(rng); bl2[1] = rand_fe<FrP>(rng); bl2[2] = rand_fe<FrP>(rng); }
    if (expanded) { if (has2) kappa2 = rand_fe<FrP>(rng); return; }
    s_L.resize(n); s_R.resize(n);
    for (size_t i = n1; i < n; i++) s_L[i] = rand_fe<FrP>(rng);
    for (size_t i = n1; i < n; i++) s_R[i] = rand_fe<FrP>(rng);
}
// The blinding factors of T_1, T_3 .. T_6 (prover.rs:700-707): the next draws whatever t(x) turns out to be
template <class C> static void prove_draw_t(TranscriptRng& rng, F4 tb[5]) {
    for (int i = 0; i < 5; i++) tb[i] = rand_fe<typename C::Fr>(rng);
}

// A_I, A_O, S of phase 1 or 2 into the transcript
template <class C> static void prove_append_phase(Transcript& tr, int phase, const A4& A_I, const A4& A_O, const A4& S) {
    typedef TP<C> T;
    T::append_point(tr, phase == 1 ? "A_I1" : "A_I2", A_I); T::append_point(tr, phase == 1 ? "A_O1" : "A_O2", A_O); T::append_point(tr, phase == 1 ? "S1" : "S2", S);
}

// From the T commitments to the challenge w (prover.rs:709-777).  Tc: T_1, T_3 .. T_6; tco: t_1 .. t_6; tb: the blinding factors of
// T_1, T_3 .. T_6; b1 / bl2: i_b, o_b, s_b of the two phases.
template <class C> static void prove_t_tail(Transcript& tr, const A4 Tc[5], const F4 tco[6], const F4 tb[5], const std::vector<F4>& wV, const std::vector<F4>& v_blinding, const F4 b1[3],
                                            const F4 bl2[3], F4& u, F4& x, F4& t_x, F4& t_x_blinding, F4& e_blinding, F4& w) {
    typedef Fld<typename C::Fr> S;
    typedef TP<C> T;
    T::append_point(tr, "T_1", Tc[0]); T::append_point(tr, "T_3", Tc[1]); T::append_point(tr, "T_4", Tc[2]); T::append_point(tr, "T_5", Tc[3]); T::append_point(tr, "T_6", Tc[4]);
    u = T::challenge_scalar(tr, "u"); x = T::challenge_scalar(tr, "x");
    F4 t2b = S::zero();
    for (size_t j = 0; j < wV.size(); j++) t2b = S::add(t2b, S::mul(v_blinding[j], wV[j]));
    auto poly6 = [&](const F4& c1, const F4& c2, const F4& c3, const F4& c4, const F4& c5, const F4& c6) {  // util.rs:107-109
        F4 acc = S::add(S::mul(x, c6), c5);
        acc = S::add(S::mul(acc, x), c4); acc = S::add(S::mul(acc, x), c3); acc = S::add(S::mul(acc, x), c2); acc = S::add(S::mul(acc, x), c1);
        return S::mul(acc, x);
    };
    t_x = poly6(tco[0], tco[1], tco[2], tco[3], tco[4], tco[5]);
    t_x_blinding = poly6(tb[0], t2b, tb[1], tb[2], tb[3], tb[4]);
    const F4 i_b = S::add(b1[0], S::mul(u, bl2[0])), o_b = S::add(b1[1], S::mul(u, bl2[1])), s_b = S::add(b1[2], S::mul(u, bl2[2]));
    e_blinding = S::mul(x, S::add(i_b, S::mul(x, S::add(o_b, S::mul(x, s_b)))));
    T::append_scalar(tr, "t_x", t_x); T::append_scalar(tr, "t_x_blinding", t_x_blinding); T::append_scalar(tr, "e_blinding", e_blinding);
    w = T::challenge_scalar(tr, "w");
}

// One round of the inner-product argument on the transcript (inner_product_proof.rs:160-163): L, R in, u out
template <class C> static F4 prove_round_challenge(Transcript& tr, const A4& L, const A4& R) {
    TP<C>::append_point(tr, "L", L); TP<C>::append_point(tr, "R", R);
    return TP<C>::challenge_scalar(tr, "u");
}

// A 96-byte result record of the table-sum kernels: X, Y, Z as ark words (Z = 0 for the identity)
static inline J4 jac_from_words(const u64* P) {
    J4 p;
    memcpy(p.X.v, P, 32); memcpy(p.Y.v, P + 4, 32); memcpy(p.Z.v, P + 8, 32);
    return p;
}

// Affine forms of `count` Jacobian points with ONE field inversion (Montgomery's trick; the identity stays (0, 0)).  The running
// products need `count` values of room: the caller's `prefix`, else the stack up to TO_AFF_STACK points (every single-proof call:
// no allocation on that path) and a vector beyond.
static constexpr size_t TO_AFF_STACK = 16;
template <class C> static void to_aff_many(const J4* in, size_t count, A4* out, F4* prefix = nullptr) {
    typedef Grp<C> G;
    typedef Fld<typename C::Fq> F;
    F4 few[TO_AFF_STACK];
    std::vector<F4> many;
    F4* pref = prefix ? prefix : few;
    if (!prefix && count > TO_AFF_STACK) { many.resize(count); pref = many.data(); }
    F4 run = F::one();
    for (size_t i = 0; i < count; i++) { pref[i] = run; if (!G::is_inf(in[i])) run = F::mul(run, in[i].Z); }
    F4 inv = F::inv(run);
    for (size_t i = count; i-- > 0;) {
        if (G::is_inf(in[i])) { out[i] = G::aff_inf(); continue; }
        const F4 zi = F::mul(inv, pref[i]), zi2 = F::sqr(zi);
        inv = F::mul(inv, in[i].Z);
        out[i] = A4{F::mul(in[i].X, zi2), F::mul(in[i].Y, F::mul(zi2, zi))};
    }
}

}  // namespace host
}  // namespace arkbp
