// Kernels of bp_verifier_verify_batch (verify_each.inc): many proofs per call, ONE mega-check per proof (`Verifier::verify`,
// src/r1cs/verifier.rs:549-600, weight 1) instead of one for the batch.
//
// A small statement's check is  sB * B + sBb * B_blinding + <g, G[..N)> + <h, H[..N)>  (fixed bases: a plain sum over the direct
// window tables, small.cuh)  +  sum over the proof's OWN points A_I1 .. S2, V_j, T_i, L_j, R_j (variable bases: 11 + m + 2 lg N of
// them).  k_vfy_batch with one chunk per proof leaves g and h per proof; here
//   k_ve_heads   the two head scalars per proof and the proof's DtJob for k_dt_accum_multi,
//   k_ve_tail    P independent short variable-base MSMs, one workgroup per job,
//   k_ve_check   fixed sum + tail sum per proof, the point and the verdict flag.
#pragma once
#include "small_batch.cuh"

namespace arkbp {

// ---- job layout and digit extraction of k_ve_tail (plain functions: tests reach them on the host through bp_debug_ve_plan) ----------
// Job p owns terms [toff[p], toff[p + 1]) of the points / scalars arrays.  A workgroup has 64 quads; quad w forms the sum of WINDOW w
// (the w-th 4-bit digit of every scalar, least significant first) in four BIT-PLANE accumulators: plane b collects the points whose
// digit has bit b set, so the window's sum is  pl0 + 2 pl1 + 4 pl2 + 8 pl3  and no look-up is indexed by the digit.  The 64 window sums
// meet in two Horner passes: quad j < 16 folds windows 4j .. 4j + 3 into a GROUP sum (12 doublings), then quad 0 folds the 16 group sums
// (240 doublings):  result = sum_w 16^w * window[w].
static constexpr u32 VE_WINDOWS = 64, VE_PLANES = 4, VE_GROUP = 4, VE_GROUPS = VE_WINDOWS / VE_GROUP;
ARKBP_HD u32 ve_window_word(u32 w) { return w >> 3; }                 // which of the eight canonical words holds window w
ARKBP_HD u32 ve_window_shift(u32 w) { return 4u * (w & 7u); }
ARKBP_HD u32 ve_digit(const u32* k /* 8 canonical words */, u32 w) { return (k[ve_window_word(w)] >> ve_window_shift(w)) & 15u; }
ARKBP_HD u32 ve_plane_bit(u32 digit, u32 b) { return (digit >> b) & 1u; }
ARKBP_HD u32 ve_job_first(const u32* toff, u32 p) { return toff[p]; }
ARKBP_HD u32 ve_job_terms(const u32* toff, u32 p) { return toff[p + 1] - toff[p]; }
ARKBP_HD u32 ve_window_of_lane(u32 tid) { return tid >> 2; }           // lanes 4w .. 4w + 3 are the quad of window w
ARKBP_HD u32 ve_group_of_window(u32 w) { return w / VE_GROUP; }
ARKBP_HD u32 ve_group_slot(u32 g) { return VE_WINDOWS + g; }           // LDS slot of group sum g (slots 0 .. 63: the window sums)

#if defined(__HIPCC__)
// this lane's pick of three replicated points by a quad-uniform index (no register indexing)
__device__ __forceinline__ Jac ve_pick3(u32 i, const Jac& a0, const Jac& a1, const Jac& a2) {
    Jac r;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        r.X.l[j] = i == 0 ? a0.X.l[j] : i == 1 ? a1.X.l[j] : a2.X.l[j];
        r.Y.l[j] = i == 0 ? a0.Y.l[j] : i == 1 ? a1.Y.l[j] : a2.Y.l[j];
        r.Z.l[j] = i == 0 ? a0.Z.l[j] : i == 1 ? a1.Z.l[j] : a2.Z.l[j];
    }
    return r;
}

// grid (P), 256 lanes.  pts: resident affine points (16 words; the identity is all-zero), sc: canonical 256-bit integers (8 words),
// toff: P + 1 prefix offsets; out: P x 24 ark words (Jacobian, Z = 0 words: identity).  Every addition is complete (qjac_madd /
// qjac_add / qjac_dbl handle identity, equal and opposite operands quad-uniformly): a one-phase proof carries identity A_I2, A_O2, S2,
// and whoever wrote the proof chooses its points.  A job without terms gives the identity.  max_terms bounds the term loop.
template <class C> __global__ void __launch_bounds__(256)
k_ve_tail(const u32* __restrict__ pts, const u32* __restrict__ sc, const u32* __restrict__ toff, u32 max_terms, u32* __restrict__ out) {
    __shared__ u32 sh[(VE_WINDOWS + VE_GROUPS) * 27];
    constexpr u32 NS = VE_WINDOWS + VE_GROUPS;
    const u32 p = blockIdx.x, tid = threadIdx.x, q = tid & 3u, w = ve_window_of_lane(tid);
    const u32 t0 = ve_job_first(toff, p), nt = min(ve_job_terms(toff, p), max_terms);
    const u32 wi = ve_window_word(w), sh4 = ve_window_shift(w);
    Jac a0 = jac_inf<C>(), a1 = a0, a2 = a0, a3 = a0;
    // the next term's point and scalar word are requested before this term's additions
    Raw16 raw_n = {};
    u32 word_n = 0;
    if (nt) { raw_n = load_raw16(pts + (size_t)t0 * 16); word_n = sc[(size_t)t0 * 8 + wi]; }
#pragma unroll 1
    for (u32 t = 0; t < nt; t++) {
        const Aff P = aff_from_raw(raw_n);
        const u32 d = (word_n >> sh4) & 15u;
        const u32 tn = t0 + min(t + 1u, nt - 1u);
        raw_n = load_raw16(pts + (size_t)tn * 16);
        word_n = sc[(size_t)tn * 8 + wi];
        if (ve_plane_bit(d, 0)) a0 = qjac_madd<C>(a0, P, q);   // (quad-uniform: the four lanes hold the same digit)
        if (ve_plane_bit(d, 1)) a1 = qjac_madd<C>(a1, P, q);
        if (ve_plane_bit(d, 2)) a2 = qjac_madd<C>(a2, P, q);
        if (ve_plane_bit(d, 3)) a3 = qjac_madd<C>(a3, P, q);
    }
    // window sum = ((pl3 * 2 + pl2) * 2 + pl1) * 2 + pl0
    Jac S = a3;
#pragma unroll 1
    for (u32 b = 0; b < VE_PLANES - 1; b++) S = qjac_add<C>(qjac_dbl<C>(S, q), ve_pick3(b, a2, a1, a0), q);
    if (q == 0) lds_put_jac(sh, NS, w, S);
    __syncthreads();
    // two Horner passes over LDS slots: pass 0, quad j < 16: slots 4j .. 4j + 3 -> slot 64 + j (4 doublings per step); pass 1, quad 0:
    // slots 64 .. 79 -> the result (16 doublings per step)
#pragma unroll 1
    for (u32 pass = 0; pass < 2; pass++) {
        const u32 first = pass ? ve_group_slot(0) : w * VE_GROUP, cnt = pass ? VE_GROUPS : VE_GROUP, ndbl = pass ? 4u * VE_GROUP : 4u;
        const bool mine = pass ? w == 0 : w < VE_GROUPS;
        if (mine) {
            S = lds_get_jac(sh, NS, first + cnt - 1u);
#pragma unroll 1
            for (u32 i = cnt - 1u; i-- > 0;) {
#pragma unroll 1
                for (u32 j = 0; j < ndbl; j++) S = qjac_dbl<C>(S, q);
                S = qjac_add<C>(S, lds_get_jac(sh, NS, first + i), q);
            }
            if (pass == 0 && q == 0) lds_put_jac(sh, NS, ve_group_slot(w), S);
        }
        __syncthreads();
    }
    if (tid == 0) store_jac_ark<C>(out + (size_t)p * 24, S);
}

// One lane per proof: heads[p] = canonical [sB_p + sum_blocks d_part[p][block], sBb_p] (heads_in: ark words; d_part: what k_vfy_batch
// leaves per (proof, block) with one chunk per proof and alpha = 1: r x^2 (wc + delta) partials), and the proof's table-sum job:
// heads over B, B_blinding | the g row over G[0..N) | the h row over H[0..N) (rows: canonical resident values, DtSeg::resident = 1;
// padding elements carry non-zero g / h, so all N entries are terms).
template <class C> __global__ void __launch_bounds__(64)
k_ve_heads(const u32* __restrict__ heads_in, const u32* __restrict__ d_part, u32 nblk, u32 P, u32 N, u32 base_G, u32 base_H, const u32* __restrict__ g_rows,
           const u32* __restrict__ h_rows, u32* __restrict__ heads, DtJob* __restrict__ jobs) {
    typedef typename C::Fr F;
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    u32 w[8];
    load_words8(w, heads_in + (size_t)p * 16);
    Fe sB = fe_wred<F>(fe_load_ark<F>(w));
#pragma unroll 1
    for (u32 b = 0; b < nblk; b++) sB = fe_addr<F>(sB, load_fe_dev<F>(d_part + ((size_t)p * nblk + b) * 8));
    store_fe_canon<F>(heads + (size_t)p * 16, sB);
    load_words8(w, heads_in + (size_t)p * 16 + 8);
    store_fe_canon<F>(heads + (size_t)p * 16 + 8, fe_load_ark<F>(w));
    DtJob jb;
    jb.seg[0] = DtSeg{heads + (size_t)p * 16, 0u, 2u, 0u, 0u, 0u};
    jb.seg[1] = DtSeg{g_rows + (size_t)p * N * 8, base_G, N, 1u, 0u, 0u};
    jb.seg[2] = DtSeg{h_rows + (size_t)p * N * 8, base_H, N, 1u, 0u, 0u};
    jb.nseg = 3; jb.terms = 2u + 2u * N; jb.has_imm = 0; jb.imm_base = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) jb.imm[i] = 0;
    jobs[p] = jb;
}

// One lane per proof: check[p] = fixed[p] + tail[p] (complete Jacobian addition), 24 ark words (Z = 0 words: identity), flag[p] = 1
// iff it is the identity — `mega_check.is_zero()` (verifier.rs:595).
template <class C> __global__ void __launch_bounds__(64)
k_ve_check(const u32* __restrict__ fixed, const u32* __restrict__ tail, u32 P, u32* __restrict__ out, u32* __restrict__ flags) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const Jac r = jac_add<C>(load_jac_ark<C>(fixed + (size_t)p * 24), load_jac_ark<C>(tail + (size_t)p * 24));
    store_jac_ark<C>(out + (size_t)p * 24, r);
    flags[p] = jac_is_inf(r) ? 1u : 0u;
}
#endif  // __HIPCC__

}  // namespace arkbp
