// Unit-test operations on RAW representatives: operands and results are the nine 32-bit limbs an Fe holds, with no conversion on
// the way in or out, so a test can feed any legal representative (limbs above 2^29, values in [p, 2p) and beyond) and inspect the
// limbs that come back.  Host+device: csrc/fp29_selftest.cpp runs these bodies on the CPU with every contract asserted, the
// k_dbg_*_raw kernels of arkbp.hip run them on the GPU (bp_debug_field_raw / bp_debug_point_raw), both on the case list of
// tests/rawcases.py.  Not a product path.
#pragma once
#include "ecq.cuh"

namespace arkbp {

// field ops: in = a | b | c | d (4 x 9 limbs), out = 18 words
enum {
    RAW_F_MUL = 0,     // out[0..9) = fe_mul(a, b)
    RAW_F_SQR = 1,     // fe_sqr(a)
    RAW_F_MUL2 = 2,    // fe_mul2(a, b, c, d)
    RAW_F_SUB2 = 3,    // fe_sub<K>(a, b), K = 2, 4, 8, 16
    RAW_F_SUB4 = 4,
    RAW_F_SUB8 = 5,
    RAW_F_SUB16 = 6,
    RAW_F_WRED = 7,    // fe_wred(a)
    RAW_F_CANON = 8,   // fe_canon(a)
    RAW_F_NORM = 9,    // fe_norm(a)
    RAW_F_ZERO = 10,   // out[0] = fe_is_zero_mod(a), out[1] = fe_maybe_zero_mod(a)
    RAW_F_EQ = 11,     // out[0] = fe_eq_mod(a, b)
    RAW_F_PACK = 12,   // out[0..9) = fe_unpack(fe_pack(a)), out[9..17) = the packed words
    RAW_F_COUNT = 13
};
static constexpr int RAW_F_IN = 36, RAW_F_OUT = 18;

// point ops: in = P.X | P.Y | P.Z | Q.X | Q.Y | Q.Z (6 x 9 limbs; the mixed additions read Q.X, Q.Y as the affine operand),
// out per lane = X | Y | Z | flag (28 words; flag = `rare` of jac_madd_fast, 0 otherwise).  The quad ops return four lanes.
enum {
    RAW_P_ADD = 0, RAW_P_MADD = 1, RAW_P_DBL = 2, RAW_P_MADD_FAST = 3,
    RAW_P_QADD = 4, RAW_P_QMADD = 5, RAW_P_QDBL = 6, RAW_P_COUNT = 7
};
static constexpr int RAW_P_IN = 54, RAW_P_OUT = 28;

ARKBP_HD Fe raw_load_fe(const u32* w) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = w[i];
    return r;
}
ARKBP_HD void raw_store_fe(u32* w, const Fe& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = a.l[i];
}
ARKBP_HD Jac raw_load_jac(const u32* w) {
    Jac r;
    r.X = raw_load_fe(w); r.Y = raw_load_fe(w + 9); r.Z = raw_load_fe(w + 18);
    return r;
}
ARKBP_HD void raw_store_jac(u32* w, const Jac& p, u32 flag) {
    raw_store_fe(w, p.X); raw_store_fe(w + 9, p.Y); raw_store_fe(w + 18, p.Z);
    w[27] = flag;
}

template <class F> ARKBP_HD void raw_field_op(int op, const u32* in, u32* out) {
    const Fe a = raw_load_fe(in), b = raw_load_fe(in + 9), c = raw_load_fe(in + 18), d = raw_load_fe(in + 27);
    for (int i = 0; i < RAW_F_OUT; i++) out[i] = 0;
    Fe r = fe_zero<F>();
    switch (op) {
        case RAW_F_MUL: r = fe_mul<F>(a, b); break;
        case RAW_F_SQR: r = fe_sqr<F>(a); break;
        case RAW_F_MUL2: r = fe_mul2<F>(a, b, c, d); break;
        case RAW_F_SUB2: r = fe_sub<F, 2>(a, b); break;
        case RAW_F_SUB4: r = fe_sub<F, 4>(a, b); break;
        case RAW_F_SUB8: r = fe_sub<F, 8>(a, b); break;
        case RAW_F_SUB16: r = fe_sub<F, 16>(a, b); break;
        case RAW_F_WRED: r = fe_wred<F>(a); break;
        case RAW_F_CANON: r = fe_canon<F>(a); break;
        case RAW_F_NORM: r = fe_norm(a); break;
        case RAW_F_ZERO: out[0] = fe_is_zero_mod<F>(a) ? 1u : 0u; out[1] = fe_maybe_zero_mod<F>(a) ? 1u : 0u; return;
        case RAW_F_EQ: out[0] = fe_eq_mod<F>(a, b) ? 1u : 0u; return;
        case RAW_F_PACK: { u32 w[8]; fe_pack(w, a); r = fe_unpack(w); for (int i = 0; i < 8; i++) out[9 + i] = w[i]; break; }
        default: break;
    }
    raw_store_fe(out, r);
}

// the lane-per-operation forms
template <class C> ARKBP_HD void raw_point_op(int op, const u32* in, u32* out) {
    const Jac P = raw_load_jac(in), Q = raw_load_jac(in + 27);
    Aff A;
    A.x = Q.X; A.y = Q.Y;
    Jac r = jac_inf<C>();
    bool rare = false;
    switch (op) {
        case RAW_P_ADD: r = jac_add<C>(P, Q); break;
        case RAW_P_MADD: r = jac_madd<C>(P, A); break;
        case RAW_P_DBL: r = jac_dbl<C>(P); break;
        case RAW_P_MADD_FAST: r = jac_madd_fast<C>(P, A, rare); break;
        default: break;
    }
    raw_store_jac(out, r, rare ? 1u : 0u);
}

// the four-lanes-per-operation forms: this lane's view (lane = position in the quad); every lane of the quad calls it with the same
// operands.  On the device the exchange is the DPP move, on the CPU the QuadSim stand-in of ecq.cuh (the caller runs the rounds).
template <class C> ARKBP_QD Jac raw_quad_op(int op, const u32* in, u32 lane) {
    const Jac P = raw_load_jac(in), Q = raw_load_jac(in + 27);
    if (op == RAW_P_QADD) return qjac_add<C>(P, Q, lane);
    if (op == RAW_P_QMADD) {
        Aff A;
        A.x = Q.X; A.y = Q.Y;
        return qjac_madd<C>(P, A, lane);
    }
    return qjac_dbl<C>(P, lane);
}

}  // namespace arkbp
