// Batched forms of the small-statement kernels (small.cuh) for bp_prover_prove_batch: B proofs of one padded size N run their
// inner-product arguments in LOCKSTEP — one launch per stage serves all B, one host wait per Fiat-Shamir round.
//
// The per-proof operands come from descriptor arrays in device memory (uploaded from the pinned staging slab together with the
// round's challenges), not from kernel arguments: a launch serves thousands of proofs.  Every workgroup reads its descriptor ONCE
// into wave-uniform registers at the top (blockIdx.y is uniform, so these are scalar loads); the loops never index the array again.
// The single-proof kernels are unchanged.
#pragma once
#include "small.cuh"

namespace arkbp {

// k_dt_accum over many MSMs: grid (nblk, njobs), job blockIdx.y.  out: [njobs][nblk] points (ark words); with nblk == 1 these are
// the results.  The body is k_dt_accum's without the immediate term (jobs here have has_imm = 0: a round's c * w rides as a run of
// one term); only where the job comes from differs.
template <class C> __global__ void __launch_bounds__(256)
k_dt_accum_multi(const u32* __restrict__ tab, const DtJob* __restrict__ jobs, u32* __restrict__ out) {
    typedef typename C::Fr Fr;
    __shared__ u32 sh[64 * 27];
    const DtJob* __restrict__ jp = jobs + blockIdx.y;
    const u32 nseg = jp->nseg;
    const u32 units = jp->terms * DT_UNITS_PER_TERM;
    const u32* sc_[DT_MAXSEG];
    u32 base0_[DT_MAXSEG], count_[DT_MAXSEG], res_[DT_MAXSEG], fn_[DT_MAXSEG], fh_[DT_MAXSEG];
#pragma unroll
    for (int i = 0; i < DT_MAXSEG; i++) {
        sc_[i] = jp->seg[i].sc; base0_[i] = jp->seg[i].base0; count_[i] = jp->seg[i].count; res_[i] = jp->seg[i].resident; fn_[i] = jp->seg[i].fold_n;
        fh_[i] = jp->seg[i].fold_hi;
    }
    const u32 q = threadIdx.x & 3u, nquads = gridDim.x * 64u;
    Jac acc = jac_inf<C>();
#pragma unroll 1
    for (u32 un = blockIdx.x * 64u + (threadIdx.x >> 2); un < units; un += nquads) {
        u32 term = un / DT_UNITS_PER_TERM;
        const u32 w0 = (un % DT_UNITS_PER_TERM) * DT_UNIT;
        u32 word, base;
        {
            int s = 0;
            if (nseg > 1 && term >= count_[0]) { term -= count_[0]; s = 1; if (nseg > 2 && term >= count_[1]) { term -= count_[1]; s = 2; } }
            const u32* scp = s == 0 ? sc_[0] : s == 1 ? sc_[1] : sc_[2];
            const u32 b0 = s == 0 ? base0_[0] : s == 1 ? base0_[1] : base0_[2], res = s == 0 ? res_[0] : s == 1 ? res_[1] : res_[2];
            const u32 fn = s == 0 ? fn_[0] : s == 1 ? fn_[1] : fn_[2], fh = s == 0 ? fh_[0] : s == 1 ? fh_[1] : fh_[2];
            if (fn) term = (term / fn) * 2u * fn + (term % fn) + (fh ? fn : 0u);
            base = b0 + term;
            if (res) {
                u32 k[8];
                load_words8(k, scp + (size_t)term * 8);
                if (res == 1) fe_store_canon<Fr>(k, fe_unpack(k)); else fe_store_canon<Fr>(k, fe_load_ark<Fr>(k));
                word = k[0];
#pragma unroll
                for (int j = 1; j < 8; j++) word = (w0 >> 3) == (u32)j ? k[j] : word;
            } else {
                word = scp[(size_t)term * 8 + (w0 >> 3)];
            }
        }
        const u32 dig = (word >> (4u * (w0 & 7u))) & 0xffffu;
        const u32* T = tab + ((size_t)base * DT_WINDOWS + w0) * DT_ENT * 16;
        const u32 d0 = dig & 15u, d1 = (dig >> 4) & 15u, d2 = (dig >> 8) & 15u, d3 = (dig >> 12) & 15u;
        const Aff p0 = load_aff_dev(T + ((size_t)0 * DT_ENT + (d0 ? d0 - 1u : 0u)) * 16);
        const Aff p1 = load_aff_dev(T + ((size_t)1 * DT_ENT + (d1 ? d1 - 1u : 0u)) * 16);
        const Aff p2 = load_aff_dev(T + ((size_t)2 * DT_ENT + (d2 ? d2 - 1u : 0u)) * 16);
        const Aff p3 = load_aff_dev(T + ((size_t)3 * DT_ENT + (d3 ? d3 - 1u : 0u)) * 16);
        if (d0) acc = qjac_madd<C>(acc, p0, q);
        if (d1) acc = qjac_madd<C>(acc, p1, q);
        if (d2) acc = qjac_madd<C>(acc, p2, q);
        if (d3) acc = qjac_madd<C>(acc, p3, q);
    }
    acc = dt_quad_tree<C>(acc, sh);
    if (threadIdx.x == 0) store_jac_ark<C>(out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 24, acc);
}

// Where a group's per-proof vectors lie: proof j's vector at byte offset `off` is arena + j * per_proof + off, its ticket counter at
// counters + 16 j.  a_in / b_in hold the current vectors (twice the round's length when a fold is pending), a_out / b_out receive the
// folded ones; the host swaps the pairs between rounds.  (Kernel arguments, not descriptor fields: the layout is the same for every
// proof, so one set of offsets serves the whole group.)
struct DtRoundGeom {
    char* arena;
    u32* counters;
    unsigned long long per_proof;
    u32 a_in, b_in, a_out, b_out, cG, cH, sL, sR, partials;
};
// One proof's scalars of a lockstep round: u, ui = the previous round's challenge and its inverse, qw = the proof's w (c * Q = (c * w) * B);
// ark words
struct DtRoundDesc {
    u32 u[8], ui[8], qw[8];
};

// k_dt_round for a group: grid (gf, B), proof blockIdx.y.  n, n0 and whether a fold is pending are the same for every proof of a
// group (equal padded sizes, same round).  Each proof has its own ticket counter and partial-sum slots (zero at the group's start;
// the last workgroup of a proof leaves its counter at zero again).
template <class C> __global__ void __launch_bounds__(256)
k_dt_round_multi(const DtRoundDesc* __restrict__ descs, DtRoundGeom geo, u32 n, u32 n0, int do_fold) {
    typedef typename C::Fr F;
    __shared__ u32 sh[9 * 256];
    const DtRoundDesc* __restrict__ dp = descs + blockIdx.y;
    char* const base = geo.arena + (size_t)blockIdx.y * geo.per_proof;
    const u32* __restrict__ a_in = (const u32*)(base + geo.a_in);
    const u32* __restrict__ b_in = (const u32*)(base + geo.b_in);
    u32* __restrict__ a_out = (u32*)(base + geo.a_out);
    u32* __restrict__ b_out = (u32*)(base + geo.b_out);
    u32* __restrict__ cG = (u32*)(base + geo.cG);
    u32* __restrict__ cH = (u32*)(base + geo.cH);
    u32* __restrict__ sL = (u32*)(base + geo.sL);
    u32* __restrict__ sR = (u32*)(base + geo.sR);
    u32* __restrict__ partials = (u32*)(base + geo.partials);
    u32* __restrict__ counter = geo.counters + (size_t)blockIdx.y * 16;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    Fe u = fe_zero<F>(), ui = fe_zero<F>();
    if (do_fold) {
        u32 w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = dp->u[j];
        u = fe_load_ark<F>(w);
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = dp->ui[j];
        ui = fe_load_ark<F>(w);
    }
    auto A = [&](u32 i) -> Fe {
        const Fe lo = load_fe_dev<F>(a_in + (size_t)i * 8);
        if (!do_fold) return lo;
        return fe_norm(fe_add(fe_mul<F>(lo, u), fe_mul<F>(ui, load_fe_dev<F>(a_in + (size_t)(2 * n + i) * 8))));
    };
    auto B = [&](u32 i) -> Fe {
        const Fe lo = load_fe_dev<F>(b_in + (size_t)i * 8);
        if (!do_fold) return lo;
        return fe_norm(fe_add(fe_mul<F>(lo, ui), fe_mul<F>(u, load_fe_dev<F>(b_in + (size_t)(2 * n + i) * 8))));
    };
    Fe pl = fe_zero<F>(), pr = fe_zero<F>();
    if (t < n0) {
        Fe g = load_fe_dev<F>(cG + (size_t)t * 8), h = load_fe_dev<F>(cH + (size_t)t * 8);
        if (do_fold) {
            const bool lo_prev = (t & (4 * n - 1)) < 2 * n;
            g = fe_mul<F>(g, lo_prev ? ui : u);
            h = fe_mul<F>(h, lo_prev ? u : ui);
            store_fe_dev<F>(cG + (size_t)t * 8, g);
            store_fe_dev<F>(cH + (size_t)t * 8, h);
        }
        const u32 r = t & (2 * n - 1);
        const bool lo = r < n;
        const u32 idx = lo ? r + n : r - n;
        const Fe ai = A(idx), bi = B(idx);
        store_fe_canon<F>((lo ? sR : sL) + (size_t)t * 8, fe_mul<F>(ai, g));
        store_fe_canon<F>((lo ? sL : sR) + (size_t)(n0 + t) * 8, fe_mul<F>(bi, h));
        if (t < 2 * n) {
            const Fe at = A(t), bt = B(t);
            if (do_fold) { store_fe_dev<F>(a_out + (size_t)t * 8, at); store_fe_dev<F>(b_out + (size_t)t * 8, bt); }
            if (t < n) { pl = fe_mul<F>(at, bi); pr = fe_mul<F>(ai, bt); }
        }
    }
    pl = block_sum_fe<F>(fe_wred<F>(pl), sh);
    pr = block_sum_fe<F>(fe_wred<F>(pr), sh);
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) {
            store_fe_dev<F>(partials + (size_t)blockIdx.x * 16, pl);
            store_fe_dev<F>(partials + (size_t)blockIdx.x * 16 + 8, pr);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            sh[0] = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const bool last = sh[0] == gridDim.x - 1u;
        __syncthreads();
        if (!last) return;
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        pl = fe_zero<F>(); pr = fe_zero<F>();
        for (u32 j = threadIdx.x; j < gridDim.x; j += 256) {
            pl = fe_addr<F>(pl, load_fe_dev<F>(partials + (size_t)j * 16));
            pr = fe_addr<F>(pr, load_fe_dev<F>(partials + (size_t)j * 16 + 8));
        }
        pl = block_sum_fe<F>(pl, sh);
        pr = block_sum_fe<F>(pr, sh);
        if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        u32* oL = sL + (size_t)2 * n0 * 8;
        u32* oR = sR + (size_t)2 * n0 * 8;
        store_fe_canon<F>(oL, pl);
        store_fe_canon<F>(oR, pr);
        u32 w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = dp->qw[j];
        const Fe qv = fe_load_ark<F>(w);
        store_fe_canon<F>(oL + 8, fe_mul<F>(pl, qv));
        store_fe_canon<F>(oR + 8, fe_mul<F>(pr, qv));
    }
}

// After the last round: a[0] <- a[0] * u + u^-1 * a[1], b[0] <- b[0] * u^-1 + u * b[1] (k_ipa_fold_ab with n = 1) for every proof of
// the group, exported as ark words: out[k] = a_k (8 words), b_k (8 words).  One lane per proof.
template <class C> __global__ void __launch_bounds__(64)
k_dt_ab_final_multi(const DtRoundDesc* __restrict__ descs, DtRoundGeom geo, u32 count, u32* __restrict__ out) {
    typedef typename C::Fr F;
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const DtRoundDesc* dp = descs + k;
    const char* const base = geo.arena + (size_t)k * geo.per_proof;
    const u32* a_in = (const u32*)(base + geo.a_in);
    const u32* b_in = (const u32*)(base + geo.b_in);
    u32 w[8];
    load_words8(w, dp->u);
    const Fe u = fe_load_ark<F>(w);
    load_words8(w, dp->ui);
    const Fe ui = fe_load_ark<F>(w);
    const Fe a = fe_norm(fe_add(fe_mul<F>(load_fe_dev<F>(a_in), u), fe_mul<F>(ui, load_fe_dev<F>(a_in + 8))));
    const Fe b = fe_norm(fe_add(fe_mul<F>(load_fe_dev<F>(b_in), ui), fe_mul<F>(u, load_fe_dev<F>(b_in + 8))));
    fe_store_ark<F>(w, a); store_words8(out + (size_t)k * 16, w);
    fe_store_ark<F>(w, b); store_words8(out + (size_t)k * 16 + 8, w);
}

}  // namespace arkbp
