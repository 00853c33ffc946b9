// Material metrics on the device: the sums behind the reference's material table (utils/metric_brdf.py:32-92) of N views of H x W pixels, one launch per
// batch of views.  Ground truth as the synthetic scene's EXR maps hold it (raw float32), estimates as the render stage writes them: emission float32,
// a_prime / kd / roughness either the PNGs' 8-bit code values or the float32 maps, quantised here as render.save_png does.
//
// The reference compares x / 255 values in float32.  51 / 255 and 255 / 255 round to float32 0.2 and 1, so its clamps and its `== 1` test are tests of the
// CODE VALUE, and its squared errors are (integer difference)^2 / 255^2: the contract is stated in code values and is exact.  Every float operation is one
// correctly rounded float32 operation (the build has -ffp-contract=off):
//     q(x)  = (int)(min(max(x, 0), 1) * 255.f)                    NaN -> 0 (fmaxf), one multiply, truncation        (save_png; metric_brdf.py:36,40)
//     T(p)  = truncation toward zero of p, saturating, NaN -> 0
//     m     = ((emit_gt.r + emit_gt.g) + emit_gt.b) > 0;  m_est the same of emit                                    (:34, :70)
//     A_gt_c = m ? 0 : q(albedo_gt_c);     A_c = m ? 0 : albedo_c                                                   (:36-37, :55-56)
//     R_gt  = m ? 0 : clamp(T(rough_gt * 255.f), 51, 255)         (no clamp before the multiply: the reference has none)   (:44-45)
//     R     = m ? 0 : clamp(rough, 51, 255)                                                                         (:65-67)
//     diff  = R_gt == 255                                                                                           (:47)
//     K_gt_c = (m || !diff) ? 0 : q(kd_gt_c);   K_c = (m || !diff) ? 0 : kd_c                                       (:40-41, :48, :59-61)
// A float32 estimate x stands for the code q(x).  Per view eight 8-byte words:
//     [0] S_albedo = sum (A - A_gt)^2   [1] S_kd = sum (K - K_gt)^2   (pixels and channels)   [2] S_rough = sum (R - R_gt)^2            uint64
//     [3] n_gt = sum m   [4] n_est = sum m_est   [5] n_and   [6] n_or                                                                    uint64
//     [7] S_emit = sum over the 3 H W values of (log((double)emit + 1.0) - log((double)emit_gt + 1.0))^2                                 float64
// A term of S_emit that is NaN or inf makes the sum so, as the reference's mean does.
//
//   chunk kernel  one workgroup of 256 threads per chunk of 512 consecutive pixels of ONE view (a workgroup never spans two views).  Every map's part of
//                 the chunk is contiguous in memory: it is copied to LDS in 16-byte vectors at 16-byte-aligned ADDRESSES, whatever the alignment of
//                 the chunk's first element (a view of 3-byte pixels starts at byte n H W 3: any alignment), the ragged first and last vector element by
//                 element; nothing outside the chunk is read.  The LDS image keeps the address's phase (element e at slot e + phase), so the LDS stores
//                 are aligned vectors too.  Thread t then owns pixels t and t + 256 of the chunk, in that order; a pixel's LDS words are 3 apart between
//                 neighbouring lanes (no bank conflict).
//   sums          every thread accumulates its pixels in ascending order: the seven integers in uint32 (see the static_assert: a whole chunk's sum of
//                 squares fits), S_emit in double; the workgroup adds its threads in a fixed binary tree (stride 128, 64, ..., 1) and stores its eight
//                 words with plain stores into slab [view][chunk][8] of the workspace.
//   slab kernel   one workgroup per view: thread t adds chunks t, t + 256, ... in ascending order (uint64 / double), the same tree adds the threads.
//                 No atomics anywhere: a shape gives the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iris {

constexpr int kMmThreads = 256;
constexpr int kMmChunk = 512;                                   // pixels of a chunk
constexpr int kMmWords = 8;
constexpr int64_t kMmMaxPixels = (int64_t)1 << 30;              // H W of a view (the size guard of the host: pixel indices are ints, a view's sums stay below 2^48)
static_assert((uint64_t)kMmChunk * 3 * 255 * 255 < ((uint64_t)1 << 32), "a chunk's sum of squared code differences fits the uint32 partials");
static_assert((uint64_t)kMmMaxPixels * 3 * 255 * 255 < ((uint64_t)1 << 63), "a view's sum fits the uint64 totals");
static_assert(kMmChunk % kMmThreads == 0, "every thread owns the same number of pixels of a full chunk");

struct MmArgs {
    const float* emit_gt; const float* albedo_gt; const float* kd_gt; const float* rough_gt;
    const float* emit;
    const void* albedo; const void* kd; const void* rough;
    int albedo_u8, kd_u8, rough_u8;
    int HW, chunks;                                 // pixels of a view, chunks of a view
    uint64_t* slabs;                                // (N, chunks, 8)
};

// `count` elements from src -> lds[phase + e], phase = the element offset of src inside its 16-byte granule (returned).  16-byte loads and LDS stores at
// aligned addresses for the granules that lie inside [src, src + count), element loads for the others.  lds: 16-byte aligned, 16 / sizeof(T) + count
// + 16 / sizeof(T) elements.  src is aligned to sizeof(T).
template <typename T>
__device__ __forceinline__ int mm_stage(const T* __restrict__ src, int count, T* lds) {
    constexpr int E = 16 / (int)sizeof(T);
    const int ph = (int)(((uintptr_t)src & 15) / sizeof(T));
    const int end = ph + count;
    for (int e0 = threadIdx.x * E; e0 < end; e0 += kMmThreads * E) {
        if (e0 >= ph && e0 + E <= end) {
            *reinterpret_cast<uint4*>(lds + e0) = *reinterpret_cast<const uint4*>(src + (e0 - ph));
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int e = e0 + i;
                if (e >= ph && e < end) lds[e] = src[e - ph];
            }
        }
    }
    return ph;
}

__device__ __forceinline__ int mm_q(float x) { return (int)(fminf(fmaxf(x, 0.f), 1.f) * 255.f); }
// clamp(T(p), 51, 255): p < 51 (or NaN) -> 51, p >= 255 -> 255, else the truncation
__device__ __forceinline__ int mm_rough_code(float p) { return p >= 255.f ? 255 : (p >= 51.f ? (int)p : 51); }
__device__ __forceinline__ int mm_code(const void* lds, int i, int is_u8) {
    return is_u8 ? (int)reinterpret_cast<const uint8_t*>(lds)[i] : mm_q(reinterpret_cast<const float*>(lds)[i]);
}

constexpr int kMmSlot3 = 3 * kMmChunk + 8;          // floats of a staged 3-channel map: phase (<= 3) + 3 kMmChunk, rounded up to whole vectors
constexpr int kMmSlot1 = kMmChunk + 8;

__global__ __launch_bounds__(kMmThreads) void matmetrics_chunk_kernel(MmArgs g) {
    static_assert(kMmSlot3 * sizeof(float) >= 3 * kMmChunk + 32 && kMmSlot1 * sizeof(float) >= kMmChunk + 32, "an 8-bit map fits the slot of its float32 form");
    static_assert((6 * kMmSlot3 + 2 * kMmSlot1) * sizeof(float) >= (size_t)kMmWords * kMmThreads * sizeof(uint64_t), "the reduction reuses the maps' LDS");
    __shared__ __align__(16) float lds[6 * kMmSlot3 + 2 * kMmSlot1];
    float* const l_eg = lds;
    float* const l_ag = lds + kMmSlot3;
    float* const l_kg = lds + 2 * kMmSlot3;
    float* const l_e = lds + 3 * kMmSlot3;
    float* const l_a = lds + 4 * kMmSlot3;
    float* const l_k = lds + 5 * kMmSlot3;
    float* const l_rg = lds + 6 * kMmSlot3;
    float* const l_r = lds + 6 * kMmSlot3 + kMmSlot1;

    const int tid = threadIdx.x;
    const int n = blockIdx.x / g.chunks, chunk = blockIdx.x % g.chunks;
    const int p0 = chunk * kMmChunk;
    const int cnt = min(kMmChunk, g.HW - p0);
    const int64_t first = (int64_t)n * g.HW + p0;                 // the chunk's first pixel in the stack

    const int o_eg = mm_stage(g.emit_gt + first * 3, cnt * 3, l_eg);
    const int o_ag = mm_stage(g.albedo_gt + first * 3, cnt * 3, l_ag);
    const int o_kg = mm_stage(g.kd_gt + first * 3, cnt * 3, l_kg);
    const int o_rg = mm_stage(g.rough_gt + first, cnt, l_rg);
    const int o_e = mm_stage(g.emit + first * 3, cnt * 3, l_e);
    const int o_a = g.albedo_u8 ? mm_stage((const uint8_t*)g.albedo + first * 3, cnt * 3, (uint8_t*)l_a) : mm_stage((const float*)g.albedo + first * 3, cnt * 3, l_a);
    const int o_k = g.kd_u8 ? mm_stage((const uint8_t*)g.kd + first * 3, cnt * 3, (uint8_t*)l_k) : mm_stage((const float*)g.kd + first * 3, cnt * 3, l_k);
    const int o_r = g.rough_u8 ? mm_stage((const uint8_t*)g.rough + first, cnt, (uint8_t*)l_r) : mm_stage((const float*)g.rough + first, cnt, l_r);
    __syncthreads();

    uint32_t s_albedo = 0, s_kd = 0, s_rough = 0, n_gt = 0, n_est = 0, n_and = 0, n_or = 0;
    double s_emit = 0.0;
#pragma unroll 1
    for (int p = tid; p < cnt; p += kMmThreads) {
        const float* eg = l_eg + o_eg + 3 * p;
        const float* e = l_e + o_e + 3 * p;
        const bool m = ((eg[0] + eg[1]) + eg[2]) > 0.f;
        const bool m_est = ((e[0] + e[1]) + e[2]) > 0.f;
        n_gt += m; n_est += m_est; n_and += (m && m_est); n_or += (m || m_est);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = log((double)e[c] + 1.0) - log((double)eg[c] + 1.0);
            s_emit += d * d;
        }
        if (!m) {
            const int r_gt = mm_rough_code(l_rg[o_rg + p] * 255.f);
            const int r_code = mm_code(l_r, o_r + p, g.rough_u8);
            const int r = min(max(r_code, 51), 255);
            s_rough += (uint32_t)((r - r_gt) * (r - r_gt));
            const bool diff = r_gt == 255;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int da = mm_code(l_a, o_a + 3 * p + c, g.albedo_u8) - mm_q(l_ag[o_ag + 3 * p + c]);
                s_albedo += (uint32_t)(da * da);
                if (diff) {
                    const int dk = mm_code(l_k, o_k + 3 * p + c, g.kd_u8) - mm_q(l_kg[o_kg + 3 * p + c]);
                    s_kd += (uint32_t)(dk * dk);
                }
            }
        }
    }

    // ---- workgroup sum, fixed tree; the maps' LDS is free now
    __syncthreads();
    uint32_t* red = reinterpret_cast<uint32_t*>(lds);                         // (7, kMmThreads)
    double* red_d = reinterpret_cast<double*>(red + 7 * kMmThreads);          // (kMmThreads)
    red[0 * kMmThreads + tid] = s_albedo; red[1 * kMmThreads + tid] = s_kd; red[2 * kMmThreads + tid] = s_rough; red[3 * kMmThreads + tid] = n_gt;
    red[4 * kMmThreads + tid] = n_est; red[5 * kMmThreads + tid] = n_and; red[6 * kMmThreads + tid] = n_or;
    red_d[tid] = s_emit;
    __syncthreads();
    for (int o = kMmThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < 7; ++q) red[q * kMmThreads + tid] += red[q * kMmThreads + tid + o];
            red_d[tid] += red_d[tid + o];
        }
        __syncthreads();
    }
    uint64_t* out = g.slabs + (int64_t)blockIdx.x * kMmWords;
    if (tid < 7) out[tid] = (uint64_t)red[tid * kMmThreads];
    if (tid == 7) reinterpret_cast<double*>(out)[7] = red_d[0];
}

// sums (N, 8) from slabs (N, chunks, 8): words 0..6 uint64, word 7 a double
__global__ __launch_bounds__(kMmThreads) void matmetrics_slab_sum_kernel(const uint64_t* __restrict__ slabs, int chunks, uint64_t* __restrict__ sums) {
    __shared__ uint64_t red[7 * kMmThreads];
    __shared__ double red_d[kMmThreads];
    const int tid = threadIdx.x;
    const uint64_t* mine = slabs + (int64_t)blockIdx.x * chunks * kMmWords;
    uint64_t acc[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) acc[q] = 0;
    double acc_d = 0.0;
    for (int t = tid; t < chunks; t += kMmThreads) {
#pragma unroll
        for (int q = 0; q < 7; ++q) acc[q] += mine[(int64_t)t * kMmWords + q];
        acc_d += reinterpret_cast<const double*>(mine)[(int64_t)t * kMmWords + 7];
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) red[q * kMmThreads + tid] = acc[q];
    red_d[tid] = acc_d;
    __syncthreads();
    for (int o = kMmThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < 7; ++q) red[q * kMmThreads + tid] += red[q * kMmThreads + tid + o];
            red_d[tid] += red_d[tid + o];
        }
        __syncthreads();
    }
    uint64_t* out = sums + (int64_t)blockIdx.x * kMmWords;
    if (tid < 7) out[tid] = red[tid * kMmThreads];
    if (tid == 7) reinterpret_cast<double*>(out)[7] = red_d[0];
}

}  // namespace iris
