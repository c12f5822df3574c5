// Kernels of bp_msm_batch (msm_batch.inc): many independent variable-base MSMs per call, for jobs too long for k_ve_tail's bit planes
// (vfy_each.cuh: four additions per term and wave) and too short for the five-launch pipeline of msm_run.
//
// A job of n terms is cut into S = ceil(n / slice) SLICES of near-equal length; the host writes one table entry (job, first term,
// terms) per slice, in job order.
//   k_msb_accum     one workgroup per slice, the 64-quad layout of k_ve_tail (quad w = window w, 4-bit unsigned digits): every quad
//                   adds each term's point into bucket[w][digit] in LDS — ONE addition per term and quad, whatever the digit —, then
//                   reduces its own 15 buckets by the running-sum rule and writes one window sum per (slice, window);
//   k_msb_combine   one workgroup per job: quad w adds window w's partial sums over the job's slices, then the two Horner passes of
//                   k_ve_tail (16 group sums, one chain) give the job's point.
// Input and output conventions are k_ve_tail's (pts: resident affine points, 16 words, identity all-zero; sc: canonical 256-bit
// integers, 8 words; out: 24 ark words per job, Jacobian, Z = 0 words: identity), so a caller of k_ve_tail can adopt them.
// No two quads share a bucket: no atomics, nothing between workgroups.  Every addition is a complete one (ecq.cuh): callers choose
// their points, so identity bases and equal or opposite operands meet in a bucket, in the running sum and in the combine step.
#pragma once
#include "vfy_each.cuh"

namespace arkbp {

// ---- slicing, bucket layout and digits (plain functions: the host planner and the kernels call the same ones; tests reach them on the
// host through bp_debug_msm_batch_plan) -----------------------------------------------------------------------------------------------
static constexpr u32 MSB_BUCKETS = 15;                                   // digits 1 .. 15 (digit 0 adds nothing)
static constexpr u32 MSB_SLOTS = MSB_BUCKETS * VE_WINDOWS;               // LDS slots of a workgroup: 960 x 27 words = 103,680 B
static constexpr u32 MSB_PART_WORDS = VE_WINDOWS * 27;                   // a slice's 64 window sums in global memory
static constexpr u32 MSB_ROUTE_SHORT = 0, MSB_ROUTE_BUCKETED = 1, MSB_ROUTE_SINGLE = 2;
ARKBP_HD u32 msb_route(u64 n, u64 short_max, u64 batch_max, bool sharded) {
    if (sharded) return MSB_ROUTE_SINGLE;
    if (n <= short_max) return MSB_ROUTE_SHORT;
    return n <= batch_max ? MSB_ROUTE_BUCKETED : MSB_ROUTE_SINGLE;
}
// the slice cap when the caller names none: the call's T bucketed terms spread over half the CUs of an MI355X (256; one workgroup fits a
// CU, and slices per job round up: 128 keeps a call with few jobs inside ONE round of workgroups), within what was measured, 64 .. 512
static constexpr u32 MSB_FILL_SLICES = 128, MSB_SLICE_MIN = 64, MSB_SLICE_MAX = 512;
ARKBP_HD u32 msb_auto_slice(u64 T) {
    const u64 L = (T + MSB_FILL_SLICES - 1u) / MSB_FILL_SLICES;
    return L < MSB_SLICE_MIN ? MSB_SLICE_MIN : L > MSB_SLICE_MAX ? MSB_SLICE_MAX : (u32)L;
}
ARKBP_HD u32 msb_slice_count(u32 n, u32 slice) { return n ? (n + slice - 1u) / slice : 0u; }
// slice s of S over n terms: the first n % S slices are one term longer than the others (none longer than ceil(n / S) <= slice)
ARKBP_HD u32 msb_slice_first(u32 n, u32 S, u32 s) { const u32 base = n / S, rem = n % S; return s * base + (s < rem ? s : rem); }
ARKBP_HD u32 msb_slice_terms(u32 n, u32 S, u32 s) { return n / S + (s < n % S ? 1u : 0u); }
ARKBP_HD u32 msb_digit(const u32* k /* 8 canonical words */, u32 w) { return ve_digit(k, w); }   // unsigned: no sign, no carry window
// bucket-major: the 16 quads of a wave (consecutive windows) touch consecutive words of a row, whatever their digits
ARKBP_HD u32 msb_bucket_slot(u32 w, u32 digit /* 1 .. 15 */) { return (digit - 1u) * VE_WINDOWS + w; }
ARKBP_HD size_t msb_part_index(u32 slice, u32 limb /* 0 .. 26: X, Y, Z */, u32 w) { return ((size_t)slice * 27u + limb) * VE_WINDOWS + w; }

struct MsbSlice { u32 job, first, terms; };          // job: index into the group's out; first: index into pts / sc
struct MsbJob { u32 job, first_slice, nslices; };    // one per bucketed job

#if defined(__HIPCC__)
__device__ __forceinline__ void msb_part_put(u32* __restrict__ part, u32 slice, u32 w, const Jac& a) {
#pragma unroll
    for (u32 i = 0; i < 9; i++) {
        part[msb_part_index(slice, i, w)] = a.X.l[i]; part[msb_part_index(slice, 9 + i, w)] = a.Y.l[i]; part[msb_part_index(slice, 18 + i, w)] = a.Z.l[i];
    }
}
__device__ __forceinline__ Jac msb_part_get(const u32* __restrict__ part, u32 slice, u32 w) {
    Jac o;
#pragma unroll
    for (u32 i = 0; i < 9; i++) {
        o.X.l[i] = part[msb_part_index(slice, i, w)]; o.Y.l[i] = part[msb_part_index(slice, 9 + i, w)]; o.Z.l[i] = part[msb_part_index(slice, 18 + i, w)];
    }
    return o;
}

// grid (slices), 256 lanes, 103,680 B of LDS (one workgroup per CU).  part: slices x 64 x 27 words (msb_part_index).  max_terms bounds
// the term loop.  A quad's buckets are read and written by that quad alone: no barrier inside the walk.
template <class C> __global__ void __launch_bounds__(256)
k_msb_accum(const u32* __restrict__ pts, const u32* __restrict__ sc, const MsbSlice* __restrict__ slices, u32 max_terms, u32* __restrict__ part) {
    __shared__ u32 sh[MSB_SLOTS * 27];
    const u32 s = blockIdx.x, tid = threadIdx.x, q = tid & 3u, w = ve_window_of_lane(tid);
    const u32 t0 = slices[s].first, nt = min(slices[s].terms, max_terms);
    const u32 wi = ve_window_word(w), sh4 = ve_window_shift(w);
    {
        const Jac inf = jac_inf<C>();
#pragma unroll 1
        for (u32 slot = tid; slot < MSB_SLOTS; slot += 256u) lds_put_jac(sh, MSB_SLOTS, slot, inf);
    }
    __syncthreads();
    // the next term's point and scalar word are requested before this term's addition
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
        if (d) {   // (quad-uniform: the four lanes hold the same digit)
            const u32 slot = msb_bucket_slot(w, d);
            // all four lanes store the (replicated) sum: each lane later reads what it wrote itself
            lds_put_jac(sh, MSB_SLOTS, slot, qjac_madd<C>(lds_get_jac(sh, MSB_SLOTS, slot), P, q));
        }
    }
    // running sum: run = b15, b15 + b14, ..; the window's sum = sum of the 15 runs = sum_d d * b_d   (28 additions)
    Jac run = lds_get_jac(sh, MSB_SLOTS, msb_bucket_slot(w, MSB_BUCKETS)), sum = run;
#pragma unroll 1
    for (u32 d = MSB_BUCKETS - 1u; d >= 1u; d--) {
        run = qjac_add<C>(run, lds_get_jac(sh, MSB_SLOTS, msb_bucket_slot(w, d)), q);
        sum = qjac_add<C>(sum, run, q);
    }
    if (q == 0) msb_part_put(part, s, w, sum);
}

// grid (bucketed jobs), 256 lanes.  max_slices bounds the slice loop.
template <class C> __global__ void __launch_bounds__(256)
k_msb_combine(const u32* __restrict__ part, const MsbJob* __restrict__ jobs, u32 max_slices, u32* __restrict__ out) {
    __shared__ u32 sh[(VE_WINDOWS + VE_GROUPS) * 27];
    constexpr u32 NS = VE_WINDOWS + VE_GROUPS;
    const u32 tid = threadIdx.x, q = tid & 3u, w = ve_window_of_lane(tid);
    const MsbJob jb = jobs[blockIdx.x];
    const u32 ns = min(jb.nslices, max_slices);
    Jac S = jac_inf<C>();
#pragma unroll 1
    for (u32 i = 0; i < ns; i++) S = qjac_add<C>(S, msb_part_get(part, jb.first_slice + i, w), q);
    if (q == 0) lds_put_jac(sh, NS, w, S);
    __syncthreads();
    // the two Horner passes of k_ve_tail: pass 0, quad j < 16: slots 4j .. 4j + 3 -> slot 64 + j (4 doublings per step); pass 1, quad 0:
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
    if (tid == 0) store_jac_ark<C>(out + (size_t)jb.job * 24, S);
}
#endif  // __HIPCC__

}  // namespace arkbp
