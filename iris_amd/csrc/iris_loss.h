// The trainers' albedo regulariser (train_brdf_crf.py:292-306 with utils/loss.py:14-37; initialize.py:188-201), forward and backward.
//
// Reference: T_s = mean over segment s of the albedo prior t (three torch_scatter calls with unit weights), tbar_i = T_s(i), then
//     initialize.py:      loss = mean over the 3N entries of (a - tbar)^2
//     train_brdf_crf.py:  k = dot(tbar, a) / dot(tbar, tbar) fetched with .item() (so: a constant of the backward), loss = la * mean (k tbar - a)^2
// The scale multiplies the prior, not the albedo.  dot(tbar, tbar) = 0 gives k = NaN and a NaN loss, as the reference.
//
// Here everything works in the SORTED space of iris_prop.h (`order`, `runs`: neither is rebuilt) and k never leaves the device:
//   means    one wave per run start: lane l sums the priors at positions start + l, start + l + 64, ... in that order, xor butterfly, divides by c:
//            means[start] = (T.x, T.y, T.z, 0)
//   dots     (scale-invariant mode) one thread per position: (tbar . a, tbar . tbar) over the three channels, each workgroup reduced to one float2
//   terms    one thread per position: every workgroup first sums the dots' partials in the same fixed order (the same bits in every workgroup) -> k,
//            then |k tbar - a|^2 over the three channels, each workgroup reduced to one float; workgroup 0 stores k.  Mode mse is k = 1 (1 * tbar is exact).
//   sum      prop_sum_kernel over the workgroups' partials -> loss
//   backward one thread per position: g_albedo[order[p]] = coef gbar (a - k tbar): plain stores, every pixel once
// The grids are functions of N alone and every reduction has a fixed order: no atomics, two calls on the same inputs agree bit for bit.
// order, runs, the means' rows and the partials are read by consecutive lanes at consecutive positions; albedo, the prior and the gradient are the
// 12-byte rows of pixel order[p] (96 KB each at the trainer's batch of 8192: resident in L2).
//
// The photometric step loss of the emitter and initialisation stages (train_emitter.py:189-195, initialize.py:180-184, 206) with the response model
// frozen: L = L_sum / n_calls, rgb = crf(L, e) (iris_crf.h's lookup, the bits of iris_crf_fwd), d = rgb - gt,
//     loss = sum d^2 / (3 B),   psnr = -10 log10(max(loss, 1e-5)),   dL_sum = ((2 d) / (3 B)) * (slope e) / n_calls
// with `slope e` what iris_crf_bwd multiplies into its cotangent (0 outside the clip's closed interval and on a flat segment).
//   terms    one thread per pixel (grid-stride beyond 4096 workgroups), the knots and the table in LDS; the gradient's three words go out as plain
//            stores; d^2 is formed and summed in double: xor butterfly per wave, the four waves' sums added in wave order -> one double per workgroup
//   finish   one workgroup adds the partials in a fixed order -> loss, psnr
// The grid is a function of B alone and nothing is added atomically: loss and gradient are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iris_crf.h"
#include "iris_prop.h"

namespace iris {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 4096;     // partials per call at most; the grid is min(ceil(N / 256), 4096): a function of N alone

// the workgroup's 256 values summed as a tree in LDS; every thread returns the same bits
__device__ __forceinline__ float loss_block_sum(float v, float* part) {
    __syncthreads();                                       // `part` may still be read from the previous use
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = kLossThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void loss_seg_means_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ prior,
                                                             int n, float4* __restrict__ means) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    for (int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n; p += nwaves) {
        const int2 run = runs[p];
        if (run.x != p) continue;
        const int end = run.x + run.y;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int q = run.x + lane; q < end; q += 256) {     // four members per trip, their loads in flight together; added in position order
            f3 t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qj = q + 64 * j;
                t[j] = qj < end ? ld3(prior + order[qj] * 3) : mk3(0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (q + 64 * j < end) { sx += t[j].x; sy += t[j].y; sz += t[j].z; }
        }
        sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
        const float c = (float)run.y;
        if (lane == 0) means[p] = make_float4(sx / c, sy / c, sz / c, 0.f);
    }
}

// partials[block] = sum over the workgroup's positions of (tbar . a, tbar . tbar)
__global__ __launch_bounds__(kLossThreads) void loss_dots_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ albedo,
                                                                 const float4* __restrict__ means, int n, float2* __restrict__ partials) {
    __shared__ float part[kLossThreads];
    float ta = 0.f, tt = 0.f;
    for (int p = blockIdx.x * kLossThreads + threadIdx.x; p < n; p += gridDim.x * kLossThreads) {
        const float4 T = means[runs[p].x];
        const f3 a = ld3(albedo + order[p] * 3);
        ta += (T.x * a.x + T.y * a.y) + T.z * a.z;
        tt += (T.x * T.x + T.y * T.y) + T.z * T.z;
    }
    ta = loss_block_sum(ta, part);
    tt = loss_block_sum(tt, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(ta, tt);
}

// dots: the n_dots partials of loss_dots_kernel, or NULL for k = 1.  partials[block] = sum over the workgroup's positions of |k tbar - a|^2; k_out[0] = k.
__global__ __launch_bounds__(kLossThreads) void loss_terms_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ albedo,
                                                                  const float4* __restrict__ means, const float2* __restrict__ dots, int n_dots, int n,
                                                                  float* __restrict__ partials, float* __restrict__ k_out) {
    __shared__ float part[kLossThreads];
    float k = 1.f;
    if (dots) {
        float ta = 0.f, tt = 0.f;
        for (int b = threadIdx.x; b < n_dots; b += kLossThreads) { const float2 d = dots[b]; ta += d.x; tt += d.y; }
        ta = loss_block_sum(ta, part);
        tt = loss_block_sum(tt, part);
        k = ta / tt;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) k_out[0] = k;
    float s = 0.f;
    for (int p = blockIdx.x * kLossThreads + threadIdx.x; p < n; p += gridDim.x * kLossThreads) {
        const float4 T = means[runs[p].x];
        const f3 a = ld3(albedo + order[p] * 3);
        const float dx = k * T.x - a.x, dy = k * T.y - a.y, dz = k * T.z - a.z;
        s += (dx * dx + dy * dy) + dz * dz;
    }
    s = loss_block_sum(s, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// g_albedo[order[p]] = coef gbar (a - k tbar), coef = weight 2 / (3 N)
__global__ void loss_albedo_bwd_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ albedo,
                                       const float4* __restrict__ means, const float* __restrict__ k_in, const float* __restrict__ gbar, float coef, int n,
                                       float* __restrict__ g_albedo) {
    const float k = k_in[0], g = coef * gbar[0];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const float4 T = means[runs[p].x];
        const int64_t i = order[p];
        const f3 a = ld3(albedo + i * 3);
        g_albedo[i * 3] = g * (a.x - k * T.x);
        g_albedo[i * 3 + 1] = g * (a.y - k * T.y);
        g_albedo[i * 3 + 2] = g * (a.z - k * T.z);
    }
}

// ---- the photometric step loss
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the workgroup's sum: waves 0, 1, 2, 3 in that order; valid in thread 0
__device__ __forceinline__ double loss_block_sum_f64(double v, double* part) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kLossThreads / 64; ++w) s += part[w];
    return s;
}

// partials[block] = sum over the workgroup's pixels and channels of d^2; g[i][c] = ((2 d) / three_b) * (slope e) / n_calls
__global__ __launch_bounds__(kLossThreads) void loss_photometric_kernel(CrfArgs a, const float* __restrict__ L_sum, float n_calls, const float* __restrict__ gt,
                                                                        float three_b, double* __restrict__ partials, float* __restrict__ g) {
    extern __shared__ float crf_lds[];
    __shared__ double part[kLossThreads / 64];
    float *sp = crf_lds, *sv = crf_lds + a.n;
    crf_load_tables(a, sp, sv);
    double sq = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.B; i += (int64_t)gridDim.x * blockDim.x) {
        const float e = crf_exposure(a, i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = (L_sum[i * 3 + c] / n_calls) * e;
            const CrfSeg s = crf_segment_uniform(sp, a.n, crf_clip(x));
            const float* v = sv + c * a.n;
            const float d = crf_value(v, s) - gt[i * 3 + c];
            sq += (double)d * (double)d;
            const float slope = s.flat ? 0.f : (v[s.r] - v[s.l]) / (s.dl + s.dr);
            const float se = (x >= 0.f && x <= 1.f) ? slope * e : 0.f;         // iris_crf_bwd's factor on a cotangent of one
            g[i * 3 + c] = (((2.f * d) / three_b) * se) / n_calls;
        }
    }
    sq = loss_block_sum_f64(sq, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = sq;
}
// out[0] = loss = sum partials / three_b, out[1] = psnr: one workgroup, fixed order
__global__ __launch_bounds__(kLossThreads) void loss_photometric_finish_kernel(const double* __restrict__ partials, int n, double three_b, float* __restrict__ loss,
                                                                               float* __restrict__ psnr) {
    __shared__ double part[kLossThreads / 64];
    double s = 0.0;
    for (int t = threadIdx.x; t < n; t += kLossThreads) s += partials[t];
    s = loss_block_sum_f64(s, part);
    if (threadIdx.x == 0) {
        const float l = (float)(s / three_b);
        loss[0] = l;
        psnr[0] = (float)(-10.0 * log10((double)fmaxf(l, 1e-5f)));
    }
}

}  // namespace iris
