// A like-prover's witness from device memory (include/arkbp.h: bp_prover_assign_multipliers_dev, bp_witness_range_bits_dev).
//
//   k_wit_take           the handle's own copy of the caller's a_L, a_R (ark Montgomery words in, the same words out) and the
//                        "every word below r" check of bp_prover_assign_multipliers, in the one pass
//   k_r1cs_import_gate   the resident route of prove_upload_phase: the handle's ark words -> resident a_L, a_R and a_O = a_L * a_R
//                        (k_scalars_import twice and k_r1cs_gate_out, without the two extra trips through memory)
//   k_wit_range_bits     the witness of the range gadget (host_proto.hpp range_gadget) from 64-bit values
//
// All three: one lane per element, 256 lanes per workgroup, grid = ceil(lanes / 256), every lane at or beyond the count returns before
// it touches memory.  The counts are below 2^31 (the host checks), so the 32-bit lane index cannot wrap.
#pragma once
#include "r1cs.cuh"

namespace arkbp {

// 256-bit ark word (8 x 32 bit, little endian) at or above the modulus of F?
template <class F> __device__ __forceinline__ bool wit_geq_p(const u32 w[8]) {
    bool geq = true;   // equal so far, from the top word down
    bool decided = false;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        const u32 p = F::P[k];
        if (!decided && w[k] != p) { geq = w[k] > p; decided = true; }
    }
    return geq;
}

// out_l[i] = in_l[i], out_r[i] = in_r[i] for i < n (8 words each).  res: [flag of left, flag of right, smallest failing index of left,
// of right]; the host sets it to [0, 0, ~0, ~0] in front.  A word at or above r ORs its vector's flag and lowers its vector's index:
// a valid witness issues no atomic.  Grid: ceil(n / 256) x 256, lane i owns multiplier i; 64 B read and 64 B written per lane, bound
// by memory; in and out never alias (out is the call's own allocation).
template <class F> __global__ void __launch_bounds__(256)
k_wit_take(const u32* __restrict__ in_l, const u32* __restrict__ in_r, u32* __restrict__ out_l, u32* __restrict__ out_r, u32 n, u32* __restrict__ res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * 8;
    u32 l[8], r[8];
    load_words8(l, in_l + o); load_words8(r, in_r + o);
    store_words8(out_l + o, l); store_words8(out_r + o, r);
    if (wit_geq_p<F>(l)) { atomicOr(res + 0, 1u); atomicMin(res + 2, i); }
    if (wit_geq_p<F>(r)) { atomicOr(res + 1, 1u); atomicMin(res + 3, i); }
}

// aL[i], aR[i] = the resident form of ark_l[i], ark_r[i] (what k_scalars_import writes for the same words: fe_load_ark, then the
// canonical packed store — a pseudo-Mersenne field's plain residue included), aO[i] = aL[i] * aR[i], for i < n.  The three outputs
// are the ctx's workspaces at the phase's offset; nothing beyond n is touched (the routes' padding stays theirs).  Grid:
// ceil(n / 256) x 256, one lane per multiplier; 64 B read, 96 B written and one fe_mul (plus the two conversions) per lane: bound by
// memory.
template <class F> __global__ void __launch_bounds__(256)
k_r1cs_import_gate(const u32* __restrict__ ark_l, const u32* __restrict__ ark_r, u32* __restrict__ aL, u32* __restrict__ aR, u32* __restrict__ aO, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * 8;
    u32 wl[8], wr[8];
    load_words8(wl, ark_l + o); load_words8(wr, ark_r + o);
    const Fe l = fe_load_ark<F>(wl), r = fe_load_ark<F>(wr);
    store_fe_dev<F>(aL + o, l);
    store_fe_dev<F>(aR + o, r);
    store_fe_dev<F>(aO + o, fe_mul<F>(l, r));
}

// Lane t < total = count * nbits: value j = t / nbits, bit i = t % nbits; left[t] = 1 - bit, right[t] = bit as ark Montgomery words
// (one = 2^256 mod r = F::R1, zero = 0: no field arithmetic).  Only bits below nbits <= 64 are looked at.  Grid: ceil(total / 256) x
// 256; 8 B read (shared by the nbits lanes of a value) and 64 B written per lane, nothing beyond `total` elements is touched.
template <class F> __global__ void __launch_bounds__(256)
k_wit_range_bits(const u64* __restrict__ values, u32 total, u32 nbits, u32* __restrict__ left, u32* __restrict__ right) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 j = t / nbits, i = t - j * nbits;
    const bool bit = (values[j] >> i) & 1;
    u32 one[8], zero[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { one[k] = F::R1[k]; zero[k] = 0; }
    store_words8(left + (size_t)t * 8, bit ? zero : one);
    store_words8(right + (size_t)t * 8, bit ? one : zero);
}

}  // namespace arkbp
