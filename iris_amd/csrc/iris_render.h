// The render stage (render.py:157-279): the scene intrinsics the reference averages over jittered primary rays next to its path-traced image (render.py:178-220).
//
// The head -- render.py:179-184: ds = normalize(rays_d + dxdu*du + dydv*dv) with du, dv in [0,1) (NO -0.5, unlike path_tracing_single, utils/path_tracing.py:338-339),
// ray_intersect, the primary hit's emitter ordinal -- is iris_render_primary: pt_primary_kernel (iris_hip.hip) with the jitter offset 0 instead of 0.5, through the
// shared device function pt_jitter_dir (iris_pt.h).  The material network runs between the head and this file's kernel, where the reference calls it (render.py:186).
//
// render_intrinsics_kernel is the body of render.py:189-220 as ONE launch.  Per sample i = b * spp + s (pixel-major):
//   kd_       = albedo * (1 - metallic)                                             (:192)
//   ks_       = 0.04 * (1 - metallic) + albedo * metallic                           (:193)
//   g0, g1    = sample_specular(u2, wo, nrm, roughness_)[2:]                        (:196-197; the sampled direction is not traced and not stored)
//   a_prime_  = (g0 * ks_ + g1) + kd_                                               (:198)
//   emission_ = e0 >= 0 ? radiance[e0] : 0                                          (:201 eval_emitter without roughness: no radiance cache)
//   vis       = valid_next | (e0 >= 0)                                              (:184 ray_intersect's valid, rebuilt from the head's outputs)
//   keep      = vis & ((emission_.r + emission_.g) + emission_.b == 0)              (:202,:208; an emitter triangle whose radiance row sums to zero stays a surface)
//   !keep: kd_ = a_prime_ = 1, roughness_ = 1, metallic_ = 0                        (:209-212; SELECTED, never computed-then-overwritten with arithmetic: a miss has
//                                                                                    a zero normal, its GGX terms may be non-finite and are simply not chosen)
//   slf_      = VoxelSLF lookup at pos, UNCONDITIONALLY                             (:205: the reference does not mask it; an empty voxel gives 0; for a miss the
//                                                                                    position is what the intersector returns for a miss -- (0,0,0) here -- and the
//                                                                                    voxel that point falls into is read like any other)
// SUMMATION ORDER (part of the contract, include/iris_hip.h):
//   map[b] += (x_0 + x_1 + ... + x_{spp-1}) * (1.0f / spp)       samples added in increasing s, in float32, -ffp-contract=off
// i.e. what `map += x.reshape(-1, spp, C).mean(1)` computes with a sequential sum.  No atomics; every output element is written by one thread: bitwise reproducible.
//
// Mapping: pt_accumulate_fwd_kernel's.  One LANE per (pixel, sample), lpp = min(64, next power of two >= spp) lanes per pixel, 64 / lpp pixels per wave.  The inputs are
// sample-major (69 B per sample over nine arrays): consecutive lanes read consecutive samples, so every array is read in full lines (lanes sl >= spp of a group are
// idle: spp = 5 uses 5 of 8), where a thread per pixel would read rows spp * 12 B apart and touch a line per lane.  The per-sample terms -- the expensive part, the GGX
// sampler with its double-precision sin / cos -- run in parallel, and the 14 sums of a pixel are then formed in the order s = 0, 1, ... by every lane of the group
// through lane reads: the same sequential float sum as a one-thread-per-pixel loop.  spp > 64: rounds of 64 samples, still in order.
#pragma once
#include "iris_pt.h"

namespace iris {

struct RenderArgs {
    SlfDev slf;
    const float* radiance; int64_t n_rad;                    // (n_rad,3): the emitter's radiance tensor itself, indexed by emitter ordinal (n_rad: the emitter handle's row count)
    int64_t B; int spp, lpp;
    const float *pos, *nrm, *wo, *albedo, *rough, *metal, *u2;   // (N,3) x4, (N), (N), (N,2); N = B * spp
    const int32_t* e0; const uint8_t* valid_next;            // (N), (N)
    float *kd, *a_prime, *roughness, *metallic, *emission, *slf_out;   // (B,3),(B,3),(B),(B),(B,3),(B,3): += into the caller's maps
};

constexpr int kRenderTerms = 14;      // kd 3, a_prime 3, roughness 1, metallic 1, emission 3, slf 3

__device__ __forceinline__ void render_sample_terms(const RenderArgs& a, int64_t i, float (&x)[kRenderTerms]) {
    const f3 p = ld3(a.pos + i * 3), n = ld3(a.nrm + i * 3), wo = ld3(a.wo + i * 3), alb = ld3(a.albedo + i * 3);
    const float rough = a.rough[i], metal = a.metal[i];
    const float om = 1.f - metal;
    const f3 kd = mk3(alb.x * om, alb.y * om, alb.z * om);
    const f3 ks = mk3(0.04f * om + alb.x * metal, 0.04f * om + alb.y * metal, 0.04f * om + alb.z * metal);
    f3 t, b;                                                 // sample_specular_kernel's sequence (model/brdf.py:112-136) with per-sample roughness
    normal_space(n, t, b);
    const f3 d = specular_sampler(a.u2[i * 2], a.u2[i * 2 + 1], rough, wo, n, t, b);
    const SpecW w = specular_weights(d, wo, n, rough, false);
    const f3 ap = mk3((w.g0 * ks.x + w.g1) + kd.x, (w.g0 * ks.y + w.g1) + kd.y, (w.g0 * ks.z + w.g1) + kd.z);
    const int ord = a.e0[i];
    f3 em = mk3(0.f, 0.f, 0.f);
    if (ord >= 0 && (int64_t)ord < a.n_rad) em = ld3(a.radiance + (int64_t)ord * 3);
    const bool vis = a.valid_next[i] != 0 || ord >= 0;
    const bool keep = vis && ((em.x + em.y) + em.z == 0.f);
    const f3 s = slf_forward(a.slf, p);
    x[0] = keep ? kd.x : 1.f; x[1] = keep ? kd.y : 1.f; x[2] = keep ? kd.z : 1.f;
    x[3] = keep ? ap.x : 1.f; x[4] = keep ? ap.y : 1.f; x[5] = keep ? ap.z : 1.f;
    x[6] = keep ? rough : 1.f;
    x[7] = keep ? metal : 0.f;
    x[8] = em.x; x[9] = em.y; x[10] = em.z;
    x[11] = s.x; x[12] = s.y; x[13] = s.z;
}

__global__ __launch_bounds__(256) void render_intrinsics_kernel(RenderArgs a) {
    const int lpp = a.lpp, spp = a.spp;
    const int lane = threadIdx.x & 63, sub = lane / lpp, sl = lane - sub * lpp, ppw = 64 / lpp;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_groups = (a.B + ppw - 1) / ppw;
    const float inv = 1.0f / (float)spp;
    for (int64_t g = wave; g < n_groups; g += n_waves) {
        const int64_t b = g * ppw + sub;
        float acc[kRenderTerms];
#pragma unroll
        for (int c = 0; c < kRenderTerms; ++c) acc[c] = 0.f;
        for (int s0 = 0; s0 < spp; s0 += lpp) {                      // (spp > 64: rounds of 64 samples, still in order)
            const int sidx = s0 + sl;
            float x[kRenderTerms];
#pragma unroll
            for (int c = 0; c < kRenderTerms; ++c) x[c] = 0.f;
            if (b < a.B && sidx < spp) render_sample_terms(a, b * spp + sidx, x);
            const int n = min(lpp, spp - s0);                        // (wave-uniform)
            for (int k = 0; k < n; ++k) {                            // the sequential sum, by every lane of the group (lane reads within the group)
                const int src = sub * lpp + k;
#pragma unroll
                for (int c = 0; c < kRenderTerms; ++c) acc[c] += __shfl(x[c], src);
            }
        }
        if (b < a.B && sl == 0) {
            a.kd[b * 3] += acc[0] * inv; a.kd[b * 3 + 1] += acc[1] * inv; a.kd[b * 3 + 2] += acc[2] * inv;
            a.a_prime[b * 3] += acc[3] * inv; a.a_prime[b * 3 + 1] += acc[4] * inv; a.a_prime[b * 3 + 2] += acc[5] * inv;
            a.roughness[b] += acc[6] * inv;
            a.metallic[b] += acc[7] * inv;
            a.emission[b * 3] += acc[8] * inv; a.emission[b * 3 + 1] += acc[9] * inv; a.emission[b * 3 + 2] += acc[10] * inv;
            a.slf_out[b * 3] += acc[11] * inv; a.slf_out[b * 3 + 1] += acc[12] * inv; a.slf_out[b * 3 + 2] += acc[13] * inv;
        }
    }
}

}  // namespace iris
