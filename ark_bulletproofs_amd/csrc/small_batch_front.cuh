// The stages IN FRONT of the inner-product argument for a group of bp_prover_prove_batch (prove_batch.inc): witness import, flatten,
// t(x) and l(x) / r(x) for all B proofs of a group in one launch each, proof = blockIdx.y.  The commitments of a group are table
// sums and go through k_dt_accum_multi (small_batch.cuh).
//
// As small_batch.cuh states: the per-proof operands come from a descriptor array in device memory, and every workgroup reads its
// descriptor ONCE at the top into wave-uniform registers (blockIdx.y is uniform: scalar loads).  The arithmetic is the single-proof
// kernels' own (the *_body device functions of r1cs.cuh); only where the pointers come from differs.
//
// Two kinds of memory: the group ARENA holds what derives from the witness (per-proof slices at equal offsets, wiped when the group
// is done), the AUX buffer holds what is public (constraint indices, coefficient and power tables, the descriptors themselves).
#pragma once
#include "small_batch.cuh"
#include "blind.cuh"

namespace arkbp {

// One proof's public operands: word offsets into the aux buffer, its sizes, and where its witness lies in the pinned staging.
struct PfDesc {
    unsigned long long in_off;   // words: [a_L | a_R | a_O | s_L | s_R], n scalars each (ark words; without the last two for k_pf_import's nvec = 3)
    u32 moff, ment, mc, coefs;   // merged CSC (k_r1cs_flatten) and the coefficient table (resident words)
    u32 ztab, Z, ypow;           // z^(2^j) (32), the split power table (256 + nzhi), y^(2^k) | y^-(2^k) (64): resident words
    u32 n, n1, nzhi, pad;
};
// the challenges the evaluation needs, known one Fiat-Shamir step later than the descriptor: ark words
struct PfXu {
    u32 x[8], u[8];
};
// Where a group's per-proof vectors lie (as DtRoundGeom: one set of byte offsets serves every proof) and the group's t(x) sums.
struct PfGeom {
    char* arena;
    unsigned long long per_proof;
    u32 aL, aR, aO, sL, sR, wL, wR, wO, tpart;   // witness, flattened weights, t(x) partials
    u32 a, b, cG, cH;                            // what the lockstep rounds read (DtRoundGeom a_in, b_in, cG, cH)
    u32* tsum;                                   // [B][6] ark words
};

// a_L, a_R, a_O, s_L, s_R of every proof: ark words in pinned staging -> resident form in the proof's slices.  grid (ceil(5 max n / 256), B).
// descs == nullptr: every proof has `cnt_all` scalars per vector, packed proof after proof (a group's phase 1).
// nvec = 3: the staging holds a_L, a_R, a_O only and k_blind_expand_multi writes s_L, s_R (BP_BLINDING_EXPANDED); grid ceil(nvec max n / 256).
template <class F> __global__ void __launch_bounds__(256)
k_pf_import(const u32* __restrict__ in, const PfDesc* __restrict__ descs, u32 cnt_all, u32 nvec, PfGeom geo) {
    u32 cnt = cnt_all;
    size_t src = (size_t)blockIdx.y * nvec * cnt_all * 8u;
    if (descs) { cnt = descs[blockIdx.y].n; src = (size_t)descs[blockIdx.y].in_off; }
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nvec * cnt) return;
    const u32 v = t / cnt, i = t - v * cnt;
    const u32 off = v == 0 ? geo.aL : v == 1 ? geo.aR : v == 2 ? geo.aO : v == 3 ? geo.sL : geo.sR;
    u32* out = (u32*)(geo.arena + (size_t)blockIdx.y * geo.per_proof + off) + (size_t)i * 8;
    u32 w[8];
    load_words8(w, in + src + (size_t)t * 8);
    store_fe_dev<F>(out, fe_load_ark<F>(w));
}

// grid (ceil(max(256, max nzhi) / 256), B)
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_ztables_multi(u32* __restrict__ aux, const PfDesc* __restrict__ descs) {
    const PfDesc* __restrict__ dp = descs + blockIdx.y;
    const u32 ztab = dp->ztab, Z = dp->Z, nzhi = dp->nzhi;
    r1cs_ztables_body<C>(aux + ztab, nzhi, aux + Z);
}

// grid (ceil(max n / 256), B)
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_flatten_multi(const u32* __restrict__ aux, const PfDesc* __restrict__ descs, PfGeom geo) {
    const PfDesc* __restrict__ dp = descs + blockIdx.y;
    const u32 moff = dp->moff, ment = dp->ment, mc = dp->mc, coefs = dp->coefs, Z = dp->Z, n = dp->n;
    char* const base = geo.arena + (size_t)blockIdx.y * geo.per_proof;
    r1cs_flatten_body<C>(aux + moff, aux + ment, aux + mc, aux + coefs, aux + Z, n, (u32*)(base + geo.wL), (u32*)(base + geo.wR), (u32*)(base + geo.wO));
}

// grid (gb, B), gb = ceil(max n / 256).  gb == 1: the six sums go straight to tsum (ark words); otherwise to the proof's partial
// slots (workgroups past a proof's own n write zeros) and k_r1cs_sum_multi adds them.
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_poly_t_multi(const u32* __restrict__ aux, const PfDesc* __restrict__ descs, PfGeom geo) {
    __shared__ u32 sh[9 * 256];
    const PfDesc* __restrict__ dp = descs + blockIdx.y;
    const u32 ypow = dp->ypow, n = dp->n;
    char* const base = geo.arena + (size_t)blockIdx.y * geo.per_proof;
    r1cs_poly_t_body<C>((const u32*)(base + geo.aL), (const u32*)(base + geo.aR), (const u32*)(base + geo.aO), (const u32*)(base + geo.sL),
                        (const u32*)(base + geo.sR), (const u32*)(base + geo.wL), (const u32*)(base + geo.wR), (const u32*)(base + geo.wO), aux + ypow, n,
                        (u32*)(base + geo.tpart) + (size_t)blockIdx.x * 6 * 8, gridDim.x == 1 ? geo.tsum + (size_t)blockIdx.y * 6 * 8 : (u32*)nullptr, sh);
}
// grid (B)
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_sum_multi(PfGeom geo, u32 nparts) {
    __shared__ u32 sh[9 * 256];
    r1cs_sum_body<C>((const u32*)(geo.arena + (size_t)blockIdx.x * geo.per_proof + geo.tpart), nparts, 6u, geo.tsum + (size_t)blockIdx.x * 6 * 8, sh);
}

// grid (ceil(N / 256), B): a, b and the G / H factor vectors straight into the slots the lockstep rounds read
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_poly_eval_multi(const u32* __restrict__ aux, const PfDesc* __restrict__ descs, const PfXu* __restrict__ xus, PfGeom geo, u32 N) {
    const PfDesc* __restrict__ dp = descs + blockIdx.y;
    const PfXu* __restrict__ xp = xus + blockIdx.y;
    const u32 ypow = dp->ypow, n = dp->n, n1 = dp->n1;
    u32 xw[8], uw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { xw[j] = xp->x[j]; uw[j] = xp->u[j]; }
    char* const base = geo.arena + (size_t)blockIdx.y * geo.per_proof;
    r1cs_poly_eval_body<C>((const u32*)(base + geo.aL), (const u32*)(base + geo.aR), (const u32*)(base + geo.aO), (const u32*)(base + geo.sL),
                           (const u32*)(base + geo.sR), (const u32*)(base + geo.wL), (const u32*)(base + geo.wR), (const u32*)(base + geo.wO), aux + ypow, n, n1, N,
                           xw, uw, (u32*)(base + geo.a), (u32*)(base + geo.b), (u32*)(base + geo.cG), (u32*)(base + geo.cH));
}

}  // namespace arkbp
