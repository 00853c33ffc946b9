// The trainers' validation (train_brdf_crf.py:331-499; the same lines stand in train_emitter.py and initialize.py): the number Lightning logs as val/loss and
// the material maps of the validation images.
//
// ---- iris_val_kd_loss: validation_step (:456-499) after the material network, for a stack of N views of H x W pixels
// albedo (N HW, 3), metallic (N HW): the network's outputs at the pixel-centre primary hits, for ALL pixels (what it returns for a miss is never used);
// valid (N HW) u8.  Per pixel and channel c, every operation one correctly rounded float32 operation (the build has -ffp-contract=off):
//     est = valid ? albedo_c * (1.0f - metallic) : 0                                   (:478-481: albedo[valid] = albedo_ over zeros -- a SELECT)
//     d   = gt_c * m - est * m                                                         (:489-491)
//     q   = d * d
// Ground truth, one of two modes:
//     synthetic  gt (N HW, 3) float32 (DiffCol), emit (N HW, 3) float32;  m = ((e0 + e1) + e2 == 0) ? 1 : 0
//                (:461 tests mean(-1) == 0, the rounded sum over 3; the test of the SUM is the same test except for a sum of exactly +-2^-149, the one
//                float32 whose third rounds to zero)
//     ldr        gt (N HW, 3) the photograph's 8-bit codes, read through `lut`, 256 float32 the caller passes (utils.validation.gamma_table: rgb^(1/2.2) clamped,
//                :486), staged in LDS;  m = 1 (:463)
// Per view S_n = sum over pixels and channels of (double)q; val/loss = S / (3 HW), the mean NF.mse_loss takes (:491).
//
//   chunk kernel  iris_matmetrics.h's layout: one workgroup of 256 threads per chunk of 512 consecutive pixels of ONE view, every map's part of the chunk copied
//                 to LDS in 16-byte vectors at 16-byte aligned addresses (mm_stage), thread t then owns pixels t and t + 256, channels 0, 1, 2 in that order,
//                 and adds its (at most) six q in that order into one double.  The workgroup adds its threads in a fixed binary tree (stride 128, ..., 1) and
//                 stores ONE double with a plain store into slab [view][chunk] of the workspace.
//   slab kernel   one workgroup per view: thread t adds chunks t, t + 256, ... in ascending order, the same tree adds the threads.
// No atomics: the order of every addition is a function of (H W) alone, so S_n is the same bits on every call, and for a view alone or at any row of a stack.
//
// ---- iris_val_intrinsics: validation()'s material maps (:372-396) after the material network, ONE launch over iris_render_primary's outputs
// Per sample i = b * spp + s:
//     emission_ = e0 >= 0 ? radiance[e0] : 0                                           (:388)
//     keep      = (valid_next | e0 >= 0) & ((emission_.r + emission_.g) + emission_.b == 0)        (:378, :389)
//     albedo_ = keep ? albedo : 0;  roughness_ = keep ? roughness : 0;  metallic_ = keep ? metallic : 0;  emission_ unmasked            (:393-396)
// Per pixel  map[b] += (x_0 + x_1 + ... + x_{spp-1}) * (1.0f / spp), samples added in increasing s in float32: iris_render_intrinsics' summation contract
// and its mapping (one lane per sample, the sums formed in order through lane reads; iris_render.h).
// Two deliberate differences.  From iris_render_intrinsics: a masked sample counts as 0, not as the default material (1, 1, 0), and there is no kd, a_prime
// or slf map.  From the reference: the mask is a SELECT where the reference multiplies by 0 (:393-395); the two differ only where the network returns a
// non-finite value at a masked sample (0 * inf = NaN there, 0 here).
#pragma once
#include "iris_matmetrics.h"
#include "iris_pt.h"

namespace iris {

struct ValLossArgs {
    const float* albedo; const float* metallic; const uint8_t* valid;
    const void* gt; const float* emit; const float* lut;        // gt: float32, or u8 codes read through lut (gt_u8)
    int gt_u8;
    int HW, chunks;                                             // pixels of a view, chunks of a view
    double* slabs;                                              // (N, chunks)
};

constexpr int kValLut = 256;

__global__ __launch_bounds__(kMmThreads) void val_loss_chunk_kernel(ValLossArgs g) {
    static_assert(kMmSlot3 * sizeof(float) >= 3 * kMmChunk + 32 && kMmSlot1 * sizeof(float) >= kMmChunk + 32, "an 8-bit map fits the slot of its float32 form");
    static_assert((3 * kMmSlot3 + 2 * kMmSlot1) * sizeof(float) >= (size_t)kMmThreads * sizeof(double), "the reduction reuses the maps' LDS");
    __shared__ __align__(16) float lds[3 * kMmSlot3 + 2 * kMmSlot1];
    __shared__ float l_lut[kValLut];
    float* const l_a = lds;
    float* const l_g = lds + kMmSlot3;
    float* const l_e = lds + 2 * kMmSlot3;
    float* const l_m = lds + 3 * kMmSlot3;
    uint8_t* const l_v = reinterpret_cast<uint8_t*>(lds + 3 * kMmSlot3 + kMmSlot1);

    const int tid = threadIdx.x;
    const int n = blockIdx.x / g.chunks, chunk = blockIdx.x % g.chunks;
    const int p0 = chunk * kMmChunk;
    const int cnt = min(kMmChunk, g.HW - p0);
    const int64_t first = (int64_t)n * g.HW + p0;                 // the chunk's first pixel in the stack

    const int o_a = mm_stage(g.albedo + first * 3, cnt * 3, l_a);
    const int o_m = mm_stage(g.metallic + first, cnt, l_m);
    const int o_v = mm_stage(g.valid + first, cnt, l_v);
    int o_g, o_e = 0;
    if (g.gt_u8) {
        o_g = mm_stage((const uint8_t*)g.gt + first * 3, cnt * 3, (uint8_t*)l_g);
        l_lut[tid] = g.lut[tid];                                  // (kMmThreads == kValLut)
    } else {
        o_g = mm_stage((const float*)g.gt + first * 3, cnt * 3, l_g);
        o_e = mm_stage(g.emit + first * 3, cnt * 3, l_e);
    }
    static_assert(kMmThreads == kValLut, "one table entry per thread");
    __syncthreads();

    double s = 0.0;
#pragma unroll 1
    for (int p = tid; p < cnt; p += kMmThreads) {
        const bool valid = l_v[o_v + p] != 0;
        const float om = 1.0f - l_m[o_m + p];
        float m = 1.0f;
        if (!g.gt_u8) {
            const float* e = l_e + o_e + 3 * p;
            m = ((e[0] + e[1]) + e[2] == 0.f) ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gt = g.gt_u8 ? l_lut[reinterpret_cast<const uint8_t*>(l_g)[o_g + 3 * p + c]] : l_g[o_g + 3 * p + c];
            const float est = valid ? l_a[o_a + 3 * p + c] * om : 0.f;
            const float d = gt * m - est * m;
            const float q = d * d;
            s += (double)q;
        }
    }

    // ---- workgroup sum, fixed tree; the maps' LDS is free now
    __syncthreads();
    double* red = reinterpret_cast<double*>(lds);
    red[tid] = s;
    __syncthreads();
    for (int o = kMmThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) g.slabs[blockIdx.x] = red[0];
}

// sums (N) from slabs (N, chunks)
__global__ __launch_bounds__(kMmThreads) void val_loss_slab_sum_kernel(const double* __restrict__ slabs, int chunks, double* __restrict__ sums) {
    __shared__ double red[kMmThreads];
    const int tid = threadIdx.x;
    const double* mine = slabs + (int64_t)blockIdx.x * chunks;
    double acc = 0.0;
    for (int t = tid; t < chunks; t += kMmThreads) acc += mine[t];
    red[tid] = acc;
    __syncthreads();
    for (int o = kMmThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) sums[blockIdx.x] = red[0];
}

struct ValMapsArgs {
    const float* radiance; int64_t n_rad;                    // (n_rad,3): the emitter's radiance tensor, indexed by emitter ordinal
    int64_t B; int spp, lpp;
    const float *albedo, *rough, *metal;                     // (N,3), (N), (N); N = B * spp
    const int32_t* e0; const uint8_t* valid_next;            // (N), (N)
    float *albedo_map, *roughness, *metallic, *emission;     // (B,3),(B),(B),(B,3): += into the caller's maps
};

constexpr int kValTerms = 8;          // albedo 3, roughness 1, metallic 1, emission 3

__device__ __forceinline__ void val_sample_terms(const ValMapsArgs& a, int64_t i, float (&x)[kValTerms]) {
    const int ord = a.e0[i];
    f3 em = mk3(0.f, 0.f, 0.f);
    if (ord >= 0 && (int64_t)ord < a.n_rad) em = ld3(a.radiance + (int64_t)ord * 3);
    const bool vis = a.valid_next[i] != 0 || ord >= 0;
    const bool keep = vis && ((em.x + em.y) + em.z == 0.f);
    const f3 alb = ld3(a.albedo + i * 3);
    x[0] = keep ? alb.x : 0.f; x[1] = keep ? alb.y : 0.f; x[2] = keep ? alb.z : 0.f;
    x[3] = keep ? a.rough[i] : 0.f;
    x[4] = keep ? a.metal[i] : 0.f;
    x[5] = em.x; x[6] = em.y; x[7] = em.z;
}

__global__ __launch_bounds__(256) void val_intrinsics_kernel(ValMapsArgs a) {
    const int lpp = a.lpp, spp = a.spp;
    const int lane = threadIdx.x & 63, sub = lane / lpp, sl = lane - sub * lpp, ppw = 64 / lpp;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_groups = (a.B + ppw - 1) / ppw;
    const float inv = 1.0f / (float)spp;
    for (int64_t g = wave; g < n_groups; g += n_waves) {
        const int64_t b = g * ppw + sub;
        float acc[kValTerms];
#pragma unroll
        for (int c = 0; c < kValTerms; ++c) acc[c] = 0.f;
        for (int s0 = 0; s0 < spp; s0 += lpp) {                      // (spp > 64: rounds of 64 samples, still in order)
            const int sidx = s0 + sl;
            float x[kValTerms];
#pragma unroll
            for (int c = 0; c < kValTerms; ++c) x[c] = 0.f;
            if (b < a.B && sidx < spp) val_sample_terms(a, b * spp + sidx, x);
            const int n = min(lpp, spp - s0);                        // (wave-uniform)
            for (int k = 0; k < n; ++k) {                            // the sequential sum, by every lane of the group (lane reads within the group)
                const int src = sub * lpp + k;
#pragma unroll
                for (int c = 0; c < kValTerms; ++c) acc[c] += __shfl(x[c], src);
            }
        }
        if (b < a.B && sl == 0) {
            a.albedo_map[b * 3] += acc[0] * inv; a.albedo_map[b * 3 + 1] += acc[1] * inv; a.albedo_map[b * 3 + 2] += acc[2] * inv;
            a.roughness[b] += acc[3] * inv;
            a.metallic[b] += acc[4] * inv;
            a.emission[b * 3] += acc[5] * inv; a.emission[b * 3 + 1] += acc[6] * inv; a.emission[b * 3 + 2] += acc[7] * inv;
        }
    }
}

}  // namespace iris
