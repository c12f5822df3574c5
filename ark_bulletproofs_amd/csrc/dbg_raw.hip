// Kernels of the raw-representative unit ops (dbg_raw.cuh; bp_debug_field_raw / bp_debug_point_raw in arkbp.hip launch them through the
// two functions at the end).  A translation unit of its own: unit-test kernels stay out of the code object of the product kernels.
#include <hip/hip_runtime.h>
#include "dbg_raw.cuh"

namespace arkbp {

// one case per lane
template <class F> __global__ void k_dbg_field_raw(int op, const u32* in, u32* out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    raw_field_op<F>(op, in + (size_t)i * RAW_F_IN, out + (size_t)i * RAW_F_OUT);
}
template <class C> __global__ void k_dbg_point_raw(int op, const u32* in, u32* out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    raw_point_op<C>(op, in + (size_t)i * RAW_P_IN, out + (size_t)i * RAW_P_OUT);
}
// the quad ops take FOUR adjacent lanes per case with replicated operands (64 different cases per 256-thread block, so neighbouring
// quads hold different data and diverge) and return every lane's result
template <class C> __global__ void __launch_bounds__(256) k_dbg_quad_raw(int op, const u32* in, u32* out, u32 n) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 i = t >> 2;              // quad-uniform: the four lanes of a case leave together
    if (i >= n) return;
    const Jac r = raw_quad_op<C>(op, in + (size_t)i * RAW_P_IN, t & 3u);
    raw_store_jac(out + (size_t)t * RAW_P_OUT, r, 0);
}

// in: n x RAW_F_IN words, out: n x RAW_F_OUT words (device pointers)
int dbg_raw_launch_field(hipStream_t st, int field, int op, const u32* in, u32* out, u32 n) {
    const u32 gb = (n + 63) / 64;
    switch (field) {
        case 0: hipLaunchKernelGGL(k_dbg_field_raw<SecqFq>, dim3(gb), dim3(64), 0, st, op, in, out, n); break;
        case 1: hipLaunchKernelGGL(k_dbg_field_raw<SecqFr>, dim3(gb), dim3(64), 0, st, op, in, out, n); break;
        case 2: hipLaunchKernelGGL(k_dbg_field_raw<ZorroFq>, dim3(gb), dim3(64), 0, st, op, in, out, n); break;
        default: hipLaunchKernelGGL(k_dbg_field_raw<ZorroFr>, dim3(gb), dim3(64), 0, st, op, in, out, n); break;
    }
    return 0;
}
// in: n x RAW_P_IN words, out: n x RAW_P_OUT words (ops below RAW_P_QADD) or n x 4 x RAW_P_OUT (the quad ops)
int dbg_raw_launch_point(hipStream_t st, int curve, int op, const u32* in, u32* out, u32 n) {
    if (op < RAW_P_QADD) {
        const u32 gb = (n + 63) / 64;
        if (curve == 0) hipLaunchKernelGGL(k_dbg_point_raw<Secq>, dim3(gb), dim3(64), 0, st, op, in, out, n);
        else hipLaunchKernelGGL(k_dbg_point_raw<Zorro>, dim3(gb), dim3(64), 0, st, op, in, out, n);
    } else {
        const u32 gb = (u32)(((size_t)n * 4 + 255) / 256);
        if (curve == 0) hipLaunchKernelGGL(k_dbg_quad_raw<Secq>, dim3(gb), dim3(256), 0, st, op, in, out, n);
        else hipLaunchKernelGGL(k_dbg_quad_raw<Zorro>, dim3(gb), dim3(256), 0, st, op, in, out, n);
    }
    return 0;
}

}  // namespace arkbp
