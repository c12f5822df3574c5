// Blinding vectors from a key (BP_BLINDING_EXPANDED, include/arkbp.h bp_prover_set_blinding): the prover's s_L, s_R of a phase are
// not 2c sequential draws from the TranscriptRng but the expansion of ONE drawn scalar kappa, computed where the vectors are used.
//
//   key          the 32 canonical little-endian bytes of kappa
//   W(key, t)    the ChaCha20 block of `key` at 64-bit block counter t, stream 0 (rand_chacha 0.3's layout, as host::ChaChaRng and
//                vfe.hip's chacha20_block), its 16 words read as ONE little-endian 512-bit integer, reduced mod r.  No rejection: the
//                bias of a 512-bit value mod a 255 / 256-bit r is below 2^-255.  A zero result stays zero.
//   s_L[first + j] = W(key, 2j),  s_R[first + j] = W(key, 2j + 1)      for the phase-local index j < c; counters stay below 2^32
//
// One lane per output scalar: 10 double rounds (about 1 300 VALU instructions) and two field products per 32 bytes written, nothing
// read but the key: no LDS, no cross-lane traffic.  The value leaves through store_fe_dev, so the words are exactly those
// k_scalars_import writes for the same scalar.
//
// blind_scalar is host-callable so that the arithmetic can be checked without a device; the host twin the tests compare against is
// an independent implementation on 64-bit Montgomery words (r1cs_host.inc host_blind_scalar).
#pragma once
#include "fp29.cuh"

namespace arkbp {

struct BlindKey {
    u32 k[8];
};
// one expansion job of the multi-member form: 64 bytes, read once per workgroup
struct BlindDesc {
    u32 key[8];
    u32 slot;           // which per-proof slice of the arena
    u32 first, count;   // the scalars s_L[first .. first + count), s_R[first .. first + count)
    u32 pad[5];
};

ARKBP_HD u32 blind_rotl(u32 v, int c) { return (v << c) | (v >> (32 - c)); }
ARKBP_HD void blind_chacha_block(const u32 key[8], u32 ctr, u32 out[16]) {
    const u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], ctr, 0u, 0u, 0u};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = in[i];
#define ARKBP_BQR(a, b, c, d)                                                                                                                 \
    x[a] += x[b]; x[d] = blind_rotl(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = blind_rotl(x[b] ^ x[c], 12);                                        \
    x[a] += x[b]; x[d] = blind_rotl(x[d] ^ x[a], 8); x[c] += x[d]; x[b] = blind_rotl(x[b] ^ x[c], 7);
#pragma unroll 1
    for (int i = 0; i < 10; i++) {
        ARKBP_BQR(0, 4, 8, 12) ARKBP_BQR(1, 5, 9, 13) ARKBP_BQR(2, 6, 10, 14) ARKBP_BQR(3, 7, 11, 15)
        ARKBP_BQR(0, 5, 10, 15) ARKBP_BQR(1, 6, 11, 12) ARKBP_BQR(2, 7, 8, 13) ARKBP_BQR(3, 4, 9, 14)
    }
#undef ARKBP_BQR
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}

// W(key, t) in the resident form: L = 1, below 2^261 (what store_fe_dev / fe_canon take).
// lo + hi * 2^256 with both halves loaded as plain 256-bit integers (fe_load_canon: V < 2.01) and 2^256 as the square of 2^128; the
// product is L = 1, V < 1.07, the sum after the carry pass L = 1, V < 3.1.
template <class F> ARKBP_HD Fe blind_scalar(const u32 key[8], u32 t) {
    u32 blk[16];
    blind_chacha_block(key, t, blk);
    const u32 w128[8] = {0u, 0u, 0u, 0u, 1u, 0u, 0u, 0u};
    const Fe p128 = fe_load_canon<F>(w128);
    const Fe p256 = fe_mul<F>(p128, p128);
    const Fe lo = fe_load_canon<F>(blk), hi = fe_load_canon<F>(blk + 8);
    return fe_norm(fe_add(lo, fe_mul<F>(hi, p256)));
}

}  // namespace arkbp

#if defined(__HIPCC__)
#include "fe_io.cuh"

namespace arkbp {

// s_L[0 .. count) and s_R[0 .. count) at the caller's pointers for the phase-local indices j0 .. j0 + count - 1: lane t < count
// writes s_L[t] = W(key, 2 (j0 + t)), lane count + t writes s_R[t] = W(key, 2 (j0 + t) + 1).  grid ceil(2 count / 256); j0 + count <= 2^31.
template <class F> __global__ void __launch_bounds__(256)
k_blind_expand(BlindKey key, u32 j0, u32 count, u32* __restrict__ sL, u32* __restrict__ sR) {
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    if (t >= 2ull * count) return;
    const u32 v = t >= count ? 1u : 0u, i = (u32)(t - (u64)v * count);
    store_fe_dev<F>((v ? sR : sL) + (size_t)i * 8, blind_scalar<F>(key.k, 2u * (j0 + i) + v));
}

// The same for the jobs of a front group (prove_batch.inc) in one launch: job = blockIdx.y, its key, range and destination slice from
// the descriptor array in device memory.  grid (ceil(2 max count / 256), jobs); the phase-local index of s_L[first + i] is i.
template <class F> __global__ void __launch_bounds__(256)
k_blind_expand_multi(const BlindDesc* __restrict__ descs, char* __restrict__ arena, unsigned long long per_proof, u32 off_sL, u32 off_sR) {
    const BlindDesc* __restrict__ dp = descs + blockIdx.y;
    const u32 count = dp->count, first = dp->first, slot = dp->slot;
    const u32 t = blockIdx.x * 256u + threadIdx.x;   // (a group's vectors are at most 2^14 long)
    if (t >= 2u * count) return;
    u32 key[8];
#pragma unroll
    for (int j = 0; j < 8; j++) key[j] = dp->key[j];
    const u32 v = t >= count ? 1u : 0u, i = t - v * count;
    u32* out = (u32*)(arena + (size_t)slot * per_proof + (v ? off_sR : off_sL)) + (size_t)(first + i) * 8;
    store_fe_dev<F>(out, blind_scalar<F>(key, 2u * i + v));
}

}  // namespace arkbp
#endif
