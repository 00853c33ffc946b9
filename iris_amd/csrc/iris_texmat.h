// The exported textures read back: a bilinear fetch from albedo.png / rm.png at a triangle's UVs, and the material that goes
// from a position to that fetch in one launch (closest triangle -> UV -> fetch).  tests/texmat_ref.py restates the fetch in numpy.
//
//   uv          b0 = (1 - b1) - b2;  uv = ((b0 vt[ft[t][0]]) + (b1 vt[ft[t][1]])) + (b2 vt[ft[t][2]]), float32, no fused multiply-add.
//   texel       the rasteriser's convention (iris_texture.h): texel (r, c) has its centre at u = (c + .5) / W, v = (r + .5) / H, row 0 at v ~ 0.
//               x = u W - 0.5, y = v H - 0.5 (float32), clamped to [0, W - 1] / [0, H - 1] (a NaN becomes 0);  x0 = floor(x), x1 = min(x0 + 1, W - 1), fx = x - x0.
//   taps        byte / 255 as a float32 division;  top = t00 + fx (t01 - t00), bot = t10 + fx (t11 - t10), out = top + fy (bot - top): four equal taps give
//               exactly their value.
//   material    albedo = the three channels of the albedo image, linear (no sRGB curve: the export wrote linear values); roughness = max(channel 0 of the rm
//               image, 0.02) -- the network's floor, which trunc(0.02 * 255) / 255 lies below --; metallic = channel 1.
//   no triangle tri < 0 (or >= F, or a face whose ft names a vertex outside vt): zeros, roughness 0.02.
// Uncovered texels are read as they are: it is the export's --dilate >= 1 that keeps black out of the taps at a chart's border.
#pragma once
#include "iris_closest.h"

namespace iris {

constexpr int kTexThreads = 256;
constexpr float kTexRoughnessMin = 0.02f;

struct TexDev {
    const int32_t* ft;          // (F, 3)
    const float* vt;            // (n_vt, 2)
    const uint8_t* albedo;      // (H, W, 3)
    const uint8_t* rm;          // (H, W, 3)
    int64_t F, n_vt;
    int H, W;
};

__device__ __forceinline__ float tex_lerp(float t00, float t01, float t10, float t11, float fx, float fy) {
    const float top = t00 + fx * (t01 - t00), bot = t10 + fx * (t11 - t10);
    return top + fy * (bot - top);
}

// the four taps of one lookup: columns x0 / x1, rows y0 / y1 and the two weights, shared by the 8-bit fetch and the float texels
struct TexTaps {
    int x0, x1, y0, y1;
    float fx, fy;
};

// false: no triangle (tri outside [0, F), or a face whose ft names a vertex outside vt: the Python layer refuses such a table, the kernel only stays in bounds)
__device__ __forceinline__ bool tex_taps(const int32_t* __restrict__ ft, const float* __restrict__ vt, int64_t F, int64_t n_vt, int H, int W, int64_t tri, float b1,
                                         float b2, TexTaps& p) {
    if (tri < 0 || tri >= F) return false;
    const int i0 = ft[tri * 3], i1 = ft[tri * 3 + 1], i2 = ft[tri * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vt || i1 >= n_vt || i2 >= n_vt) return false;
    const float b0 = (1.0f - b1) - b2;
    const float u = ((b0 * vt[(int64_t)i0 * 2]) + (b1 * vt[(int64_t)i1 * 2])) + (b2 * vt[(int64_t)i2 * 2]);
    const float v = ((b0 * vt[(int64_t)i0 * 2 + 1]) + (b1 * vt[(int64_t)i1 * 2 + 1])) + (b2 * vt[(int64_t)i2 * 2 + 1]);
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    x = x > 0.f ? (x < (float)(W - 1) ? x : (float)(W - 1)) : 0.f;             // (a NaN fails the first comparison)
    y = y > 0.f ? (y < (float)(H - 1) ? y : (float)(H - 1)) : 0.f;
    const float xf = floorf(x), yf = floorf(y);
    p.x0 = (int)xf; p.y0 = (int)yf; p.x1 = min(p.x0 + 1, W - 1); p.y1 = min(p.y0 + 1, H - 1);
    p.fx = x - xf; p.fy = y - yf;
    return true;
}

// out: albedo r, g, b, roughness, metallic
__device__ __forceinline__ void tex_fetch(const TexDev& t, int64_t tri, float b1, float b2, float out[5]) {
    out[0] = out[1] = out[2] = out[4] = 0.f; out[3] = kTexRoughnessMin;
    TexTaps p;
    if (!tex_taps(t.ft, t.vt, t.F, t.n_vt, t.H, t.W, tri, b1, b2, p)) return;
    const int x0 = p.x0, x1 = p.x1, y0 = p.y0, y1 = p.y1;
    const float fx = p.fx, fy = p.fy;
    const int64_t o00 = ((int64_t)y0 * t.W + x0) * 3, o01 = ((int64_t)y0 * t.W + x1) * 3, o10 = ((int64_t)y1 * t.W + x0) * 3, o11 = ((int64_t)y1 * t.W + x1) * 3;
#define IRIS_TAP(IMG, O, CH) ((float)(IMG)[(O) + (CH)] / 255.0f)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        out[ch] = tex_lerp(IRIS_TAP(t.albedo, o00, ch), IRIS_TAP(t.albedo, o01, ch), IRIS_TAP(t.albedo, o10, ch), IRIS_TAP(t.albedo, o11, ch), fx, fy);
    out[3] = fmaxf(tex_lerp(IRIS_TAP(t.rm, o00, 0), IRIS_TAP(t.rm, o01, 0), IRIS_TAP(t.rm, o10, 0), IRIS_TAP(t.rm, o11, 0), fx, fy), kTexRoughnessMin);
    out[4] = tex_lerp(IRIS_TAP(t.rm, o00, 1), IRIS_TAP(t.rm, o01, 1), IRIS_TAP(t.rm, o10, 1), IRIS_TAP(t.rm, o11, 1), fx, fy);
#undef IRIS_TAP
}

__device__ __forceinline__ void tex_store(const float m[5], int64_t i, float* __restrict__ albedo, float* __restrict__ rough, float* __restrict__ metal) {
    albedo[i * 3] = m[0]; albedo[i * 3 + 1] = m[1]; albedo[i * 3 + 2] = m[2];
    rough[i] = m[3];
    metal[i] = m[4];
}

__global__ __launch_bounds__(kTexThreads) void texture_sample_kernel(TexDev t, const int64_t* __restrict__ tri, const float* __restrict__ bary, int64_t B,
                                                                     float* __restrict__ albedo, float* __restrict__ rough, float* __restrict__ metal) {
    for (int64_t i = blockIdx.x * (int64_t)kTexThreads + threadIdx.x; i < B; i += (int64_t)gridDim.x * kTexThreads) {
        float m[5];
        tex_fetch(t, tri[i], bary[i * 2], bary[i * 2 + 1], m);
        tex_store(m, i, albedo, rough, metal);
    }
}

// position -> material: closest_point_kernel's query, then texture_sample_kernel's fetch at its (tri, bary): the two-call composition, bit for bit
__global__ __launch_bounds__(kBlock) void texture_material_kernel(SceneDev sc, TexDev t, const float* __restrict__ xs, int64_t B, float* __restrict__ albedo,
                                                                  float* __restrict__ rough, float* __restrict__ metal) {
    __shared__ uint32_t s_refs[kStackLds * kBlock];
    __shared__ uint32_t s_bounds[kStackLds * kBlock];
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < B; i += (int64_t)gridDim.x * kBlock) {
        const Closest c = closest_query(sc, ld3(xs + i * 3), s_refs + threadIdx.x, s_bounds + threadIdx.x);
        float m[5];
        tex_fetch(t, c.slot >= 0 ? (int64_t)c.id : (int64_t)-1, c.b1, c.b2, m);
        tex_store(m, i, albedo, rough, metal);
    }
}

// ---- the trainable texture: float32 texels (H, W, 5) = albedo r, g, b, roughness, metallic per texel; tests/texfit_ref.py restates both
//   forward     tex_fetch with the taps read as they are (no / 255): the same tex_taps, the same tex_lerp, roughness = max(lerp, 0.02).  With texels = byte / 255
//               (a float32 division) the result is iris_texture_sample's bit for bit.
//   backward    g_texels += the transpose of the lerp: w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy), w10 = (1 - fx) fy, w11 = fx fy in float32, tap (y, x) gets w g per
//               channel; where the clamp makes x1 == x0 or y1 == y0 the weights land on one texel and sum there.  The roughness gradient passes only where the
//               interpolated value (recomputed from the texels, the forward's bits) is > 0.02.  A row without a triangle adds nothing.  Nothing flows to bary, vt
//               or the positions.
// The adds are float atomicAdd on global memory (one global_atomic_add_f32 each on gfx950, no compare-and-swap loop), twenty per point: a texel's five
// channels are 20 contiguous bytes, the two x-taps of a row 40.  The order in which they arrive is not fixed, so the gradient is REPRODUCIBLE TO ROUNDING, NOT
// BIT FOR BIT: per texel channel within (n + 4) 2^-24 sum |w g| of the exact sum over its n contributions.
struct TexelsDev {
    const int32_t* ft;          // (F, 3)
    const float* vt;            // (n_vt, 2)
    const float* texels;        // (H, W, 5)
    int64_t F, n_vt;
    int H, W;
};
constexpr int kTexelChannels = 5;

__global__ __launch_bounds__(kTexThreads) void texture_sample_f32_kernel(TexelsDev t, const int64_t* __restrict__ tri, const float* __restrict__ bary, int64_t B,
                                                                         float* __restrict__ albedo, float* __restrict__ rough, float* __restrict__ metal) {
    for (int64_t i = blockIdx.x * (int64_t)kTexThreads + threadIdx.x; i < B; i += (int64_t)gridDim.x * kTexThreads) {
        float m[5] = {0.f, 0.f, 0.f, kTexRoughnessMin, 0.f};
        TexTaps p;
        if (tex_taps(t.ft, t.vt, t.F, t.n_vt, t.H, t.W, tri[i], bary[i * 2], bary[i * 2 + 1], p)) {
            const float* t00 = t.texels + ((int64_t)p.y0 * t.W + p.x0) * kTexelChannels, *t01 = t.texels + ((int64_t)p.y0 * t.W + p.x1) * kTexelChannels;
            const float* t10 = t.texels + ((int64_t)p.y1 * t.W + p.x0) * kTexelChannels, *t11 = t.texels + ((int64_t)p.y1 * t.W + p.x1) * kTexelChannels;
#pragma unroll
            for (int ch = 0; ch < kTexelChannels; ++ch) m[ch] = tex_lerp(t00[ch], t01[ch], t10[ch], t11[ch], p.fx, p.fy);
            m[3] = fmaxf(m[3], kTexRoughnessMin);
        }
        tex_store(m, i, albedo, rough, metal);
    }
}

__global__ __launch_bounds__(kTexThreads) void texture_sample_f32_bwd_kernel(TexelsDev t, const int64_t* __restrict__ tri, const float* __restrict__ bary, int64_t B,
                                                                             const float* __restrict__ g_albedo, const float* __restrict__ g_rough,
                                                                             const float* __restrict__ g_metal, float* __restrict__ g_texels) {
    for (int64_t i = blockIdx.x * (int64_t)kTexThreads + threadIdx.x; i < B; i += (int64_t)gridDim.x * kTexThreads) {
        TexTaps p;
        if (!tex_taps(t.ft, t.vt, t.F, t.n_vt, t.H, t.W, tri[i], bary[i * 2], bary[i * 2 + 1], p)) continue;
        const int64_t o00 = ((int64_t)p.y0 * t.W + p.x0) * kTexelChannels, o01 = ((int64_t)p.y0 * t.W + p.x1) * kTexelChannels;
        const int64_t o10 = ((int64_t)p.y1 * t.W + p.x0) * kTexelChannels, o11 = ((int64_t)p.y1 * t.W + p.x1) * kTexelChannels;
        const float r = tex_lerp(t.texels[o00 + 3], t.texels[o01 + 3], t.texels[o10 + 3], t.texels[o11 + 3], p.fx, p.fy);
        const float g[kTexelChannels] = {g_albedo[i * 3], g_albedo[i * 3 + 1], g_albedo[i * 3 + 2], r > kTexRoughnessMin ? g_rough[i] : 0.f, g_metal[i]};
        const float ax = 1.0f - p.fx, ay = 1.0f - p.fy;
        const float w00 = ax * ay, w01 = p.fx * ay, w10 = ax * p.fy, w11 = p.fx * p.fy;
#pragma unroll
        for (int ch = 0; ch < kTexelChannels; ++ch) {
            atomicAdd(g_texels + o00 + ch, w00 * g[ch]);
            atomicAdd(g_texels + o01 + ch, w01 * g[ch]);
            atomicAdd(g_texels + o10 + ch, w10 * g[ch]);
            atomicAdd(g_texels + o11 + ch, w11 * g[ch]);
        }
    }
}

}  // namespace iris
