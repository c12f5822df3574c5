// Witness check (include/arkbp.h: bp_prover_check, bp_prover_set_check): does the resident witness satisfy the recorded constraint
// system?  The flatten kernels (r1cs.cuh) walk the constraints by COLUMN (HostCsc); these walk them by ROW, the recorder's own order.
//
//   gate i        a_L[i] * a_R[i] == a_O[i]  (mod r), one lane per multiplier
//   constraint k  sum of coefficient * variable over its terms == 0  (mod r)
//
// The host cuts every row into PIECES of at most WC_PIECE terms (host::build_row_index, prove_steps.hpp): no lane walks an unbounded
// row.  k_r1cs_check has one lane per gate and per piece: a one-piece row is decided there, a piece of a longer row stores its partial
// sum.  k_r1cs_check_long — launched only when such rows exist — sums the pieces of each long row, one workgroup per row.
// Comparisons are between canonical representatives (fe_is_zero_mod reduces fully before it decides).
// Results: four words per statement — violated gates, smallest violated gate, violated constraints, smallest violated constraint —
// updated with atomicAdd / atomicMin by the lanes that FOUND a violation only: a satisfied witness issues no atomic.
// Every loop is bounded by a launch argument or the constant WC_PIECE; the only traffic between workgroups is those atomics.
#pragma once
#include "r1cs.cuh"

namespace arkbp {

#define BP_WITNESS_CHECK_PIECE 256
static constexpr u32 WC_PIECE = BP_WITNESS_CHECK_PIECE;   // most terms one lane walks (bp_witness_check_piece())
static constexpr u32 WC_LONG = 0x80000000u;                // piece word: bit 31 = piece of a multi-piece row, low bits = its partial slot (else: the row)
static constexpr int WC_KIND_SHIFT = 29;                   // term word: (variable kind << 29) | index; kinds as host::VKind
static constexpr u32 WC_INDEX_MASK = (1u << WC_KIND_SHIFT) - 1;

// One statement's operands.  The witness pointers are the resident vectors wherever the route keeps them (the ctx's single-proof
// workspaces, a front group's arena slices, the check's own upload); everything else lies in the check's index block.
struct WcDesc {
    const u32 *aL, *aR, *aO;   // n resident scalars each
    const u32* v;              // committed values, resident scalars
    const u32* coefs;          // de-duplicated coefficient table, resident scalars (HostCsc's convention: +-1 are flags of the id word)
    const u32* poff;           // npieces + 1 term offsets
    const u32* pinfo;          // npieces piece words
    const u32* tvar;           // term words
    const u32* tcid;           // coefficient ids: bit 31 = +1, bit 30 = -1, else an index into coefs
    const u32* lrow;           // per long row: row index, first partial slot, pieces
    u32* partial;              // one resident scalar per piece of a long row
    u32* res;                  // bad gates, first bad gate, bad constraints, first bad constraint
    u32 n, npieces, nlong, pad;
};

template <class C> __device__ __forceinline__ void r1cs_check_body(const WcDesc& d, u32 i) {
    typedef typename C::Fr F;
    if (i < d.n) {
        const size_t o = (size_t)i * 8;
        const Fe p = fe_mul<F>(load_fe_dev<F>(d.aL + o), load_fe_dev<F>(d.aR + o));
        if (!fe_eq_mod<F>(p, load_fe_dev<F>(d.aO + o))) { atomicAdd(d.res + 0, 1u); atomicMin(d.res + 1, i); }
    }
    if (i < d.npieces) {
        const u32 info = d.pinfo[i];
        const u32 e0 = d.poff[i];
        u32 e1 = d.poff[i + 1];
        if (e1 - e0 > WC_PIECE) e1 = e0 + WC_PIECE;   // (the host never cuts longer pieces: a bound the kernel does not take on trust)
        Fe acc = fe_zero<F>();
        for (u32 e = e0; e < e1; e++) {
            const u32 tv = d.tvar[e], cid = d.tcid[e], kind = tv >> WC_KIND_SHIFT;
            const size_t o = (size_t)(tv & WC_INDEX_MASK) * 8;
            Fe val;
            if (kind >= 4u) val = fe_one<F>();
            else val = load_fe_dev<F>((kind == 0u ? d.v : kind == 1u ? d.aL : kind == 2u ? d.aR : d.aO) + o);
            Fe term;
            if (cid & 0x80000000u) term = val;
            else if (cid & 0x40000000u) term = fe_wred<F>(fe_neg<F, 4>(val));
            else term = fe_mul<F>(val, load_fe_dev<F>(d.coefs + (size_t)cid * 8));
            acc = fe_addr<F>(acc, term);
        }
        if (info & WC_LONG) store_fe_dev<F>(d.partial + (size_t)(info & ~WC_LONG) * 8, acc);
        else if (!fe_is_zero_mod<F>(acc)) { atomicAdd(d.res + 2, 1u); atomicMin(d.res + 3, info); }
    }
}
// one workgroup per long row r (uniform over the workgroup); max_pieces bounds the walk over its partial sums
template <class C> __device__ __forceinline__ void r1cs_check_long_body(const WcDesc& d, u32 r, u32 max_pieces, u32* __restrict__ sh) {
    typedef typename C::Fr F;
    if (r >= d.nlong) return;
    const u32 row = d.lrow[3 * r], first = d.lrow[3 * r + 1];
    u32 cnt = d.lrow[3 * r + 2];
    if (cnt > max_pieces) cnt = max_pieces;
    Fe s = fe_zero<F>();
    for (u32 j = threadIdx.x; j < cnt; j += 256) s = fe_addr<F>(s, load_fe_dev<F>(d.partial + (size_t)(first + j) * 8));
    s = block_sum_fe<F>(s, sh);
    if (threadIdx.x == 0 && !fe_is_zero_mod<F>(s)) { atomicAdd(d.res + 2, 1u); atomicMin(d.res + 3, row); }
}

// grid ceil(max(n, npieces) / 256)
template <class C> __global__ void __launch_bounds__(256) k_r1cs_check(WcDesc d) {
    r1cs_check_body<C>(d, blockIdx.x * blockDim.x + threadIdx.x);
}
// grid nlong
template <class C> __global__ void __launch_bounds__(256) k_r1cs_check_long(WcDesc d, u32 max_pieces) {
    __shared__ u32 sh[9 * 256];
    r1cs_check_long_body<C>(d, blockIdx.x, max_pieces, sh);
}
// statement = blockIdx.y, descriptors in device memory (read once per workgroup: blockIdx.y is uniform).  grid (ceil(max over the
// statements of max(n, npieces) / 256), B)
template <class C> __global__ void __launch_bounds__(256) k_r1cs_check_multi(const WcDesc* __restrict__ descs) {
    const WcDesc d = descs[blockIdx.y];
    r1cs_check_body<C>(d, blockIdx.x * blockDim.x + threadIdx.x);
}
// grid (max nlong, B)
template <class C> __global__ void __launch_bounds__(256) k_r1cs_check_long_multi(const WcDesc* __restrict__ descs, u32 max_pieces) {
    __shared__ u32 sh[9 * 256];
    const WcDesc d = descs[blockIdx.y];
    r1cs_check_long_body<C>(d, blockIdx.x, max_pieces, sh);
}

}  // namespace arkbp
