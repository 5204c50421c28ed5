// Shared helpers for the gfx950 kernels of the GridNext f∘g hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// The C ABI: every entry point's declaration, the status codes, the form codes and the batch item structs.  Each definition below
// GNX_EXPORT is checked against its declaration there by the compiler.
#include "../../include/gridnext_hip.h"

#define GNX_EXPORT extern "C" __attribute__((visibility("default")))

static inline int gnx_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GNX_OK : GNX_ERR_LAUNCH;
}

static inline int gnx_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// More than 64 KB of dynamic LDS has to be allowed per kernel.  Called in front of the launch of Kernel with the bytes that
// launch needs - or, where one fixed maximum covers every launch of the kernel, with that maximum, so the runtime is asked
// once and never again from a step captured into a graph.  The bytes already allowed are kept per kernel and per PROCESS,
// not per device: looking the device up would cost a runtime call on every launch.
template <auto Kernel>
int gnx_allow_lds(size_t bytes) {
    static size_t allowed = 64 * 1024;
    if (bytes > allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)bytes) != hipSuccess)
            return GNX_ERR_LAUNCH;
        allowed = bytes;
    }
    return GNX_OK;
}

// 64-lane wavefront reductions (shuffles, no LDS)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sum for blockDim.x a multiple of 64 (<= 1024); result valid in every thread.
__device__ __forceinline__ float block_sum(float v, float* lds /* >= 16 floats */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) lds[wid] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += lds[i];   // fixed order: deterministic
    return r;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
