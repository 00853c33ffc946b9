// The trainers' optimizer step: torch.optim.Adam (no amsgrad, no maximize, weight decay = L2 added to the gradient) as ONE streaming pass.
//
// The host computes every scalar in double and rounds it to float once (AdamScalars); per element, in float32 and without contraction
// (-ffp-contract=off: the bits are fixed by the order written here, tests/adam_ref.py restates it in numpy):
//     g' = wd != 0 ? g + wd * p : g
//     m' = m + w1 * (g' - m)                       w1 = 1 - beta1
//     v' = v * beta2 + (w2 * g') * g'              w2 = 1 - beta2   (in DOUBLE, then rounded: 1 - (float)beta2 is off by 6e-5 relative)
//     p' = p - step_size * (m' / (sqrtf(v') / bc2 + eps))          step_size = lr / (1 - beta1^step), bc2 = sqrt(1 - beta2^step)
//
//   adam_vec4_kernel     4 parameters per thread, 16-byte loads and stores: every pointer 16-byte aligned
//   adam_scalar_kernel   one parameter per thread: unaligned buffers, and the tail of the vector kernel
//   ngp_adam_kernel      8 parameters per thread of NGPBRDF's mlp.params, and in the same pass the half copy the forward reads (d_w / d_grid of the
//                        handle), rounded to nearest even as ngp_params_cast_kernel does: the step leaves the handle refreshed, 30 B per parameter
// Plain streaming kernels: no LDS, no atomics.  All three give the same bits for the same element.
#pragma once
#include <hip/hip_runtime.h>

#include "iris_ngp.h"

namespace iris {

struct AdamScalars {
    float w1, w2, beta2, step_size, bc2, eps, wd;
};

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamScalars& s) {
    if (s.wd != 0.f) g = g + s.wd * p;
    m = m + s.w1 * (g - m);
    v = v * s.beta2 + (s.w2 * g) * g;
    p = p - s.step_size * (m / (sqrtf(v) / s.bc2 + s.eps));
}

__device__ __forceinline__ void adam_update4(float4& p, const float4& g, float4& m, float4& v, const AdamScalars& s) {
    adam_update(p.x, g.x, m.x, v.x, s);
    adam_update(p.y, g.y, m.y, v.y, s);
    adam_update(p.z, g.z, m.z, v.z, s);
    adam_update(p.w, g.w, m.w, v.w, s);
}

__global__ __launch_bounds__(256) void adam_vec4_kernel(float4* __restrict__ param, const float4* __restrict__ grad, float4* __restrict__ exp_avg,
                                                        float4* __restrict__ exp_avg_sq, int64_t n4, AdamScalars s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 p = param[i], m = exp_avg[i], v = exp_avg_sq[i];
        const float4 g = grad[i];
        adam_update4(p, g, m, v, s);
        param[i] = p; exp_avg[i] = m; exp_avg_sq[i] = v;
    }
}

// elements [i0, n)
__global__ __launch_bounds__(256) void adam_scalar_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                          float* __restrict__ exp_avg_sq, int64_t i0, int64_t n, AdamScalars s) {
    for (int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float p = param[i], m = exp_avg[i], v = exp_avg_sq[i];
        adam_update(p, grad[i], m, v, s);
        param[i] = p; exp_avg[i] = m; exp_avg_sq[i] = v;
    }
}

// n8 = n_params / 8 (kNgpMlpParams % 8 == 0: a thread's 8 parameters never straddle the matrices and the tables)
__global__ __launch_bounds__(256) void ngp_adam_kernel(float4* __restrict__ param, const float4* __restrict__ grad, float4* __restrict__ exp_avg,
                                                       float4* __restrict__ exp_avg_sq, int64_t n8, AdamScalars s, _Float16* __restrict__ w,
                                                       _Float16* __restrict__ grid) {
    static_assert(kNgpMlpParams % 8 == 0, "8 parameters per thread");
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        float4 p0 = param[2 * i], p1 = param[2 * i + 1], m0 = exp_avg[2 * i], m1 = exp_avg[2 * i + 1], v0 = exp_avg_sq[2 * i], v1 = exp_avg_sq[2 * i + 1];
        const float4 g0 = grad[2 * i], g1 = grad[2 * i + 1];
        adam_update4(p0, g0, m0, v0, s);
        adam_update4(p1, g1, m1, v1, s);
        param[2 * i] = p0; param[2 * i + 1] = p1;
        exp_avg[2 * i] = m0; exp_avg[2 * i + 1] = m1;
        exp_avg_sq[2 * i] = v0; exp_avg_sq[2 * i + 1] = v1;
        iris_h8 o;
        o[0] = (_Float16)p0.x; o[1] = (_Float16)p0.y; o[2] = (_Float16)p0.z; o[3] = (_Float16)p0.w;
        o[4] = (_Float16)p1.x; o[5] = (_Float16)p1.y; o[6] = (_Float16)p1.z; o[7] = (_Float16)p1.w;
        _Float16* dst = i * 8 < kNgpMlpParams ? w + i * 8 : grid + (i * 8 - kNgpMlpParams);
        *reinterpret_cast<iris_h8*>(dst) = o;
    }
}

}  // namespace iris
