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

// out: albedo r, g, b, roughness, metallic
__device__ __forceinline__ void tex_fetch(const TexDev& t, int64_t tri, float b1, float b2, float out[5]) {
    out[0] = out[1] = out[2] = out[4] = 0.f; out[3] = kTexRoughnessMin;
    if (tri < 0 || tri >= t.F) return;
    const int i0 = t.ft[tri * 3], i1 = t.ft[tri * 3 + 1], i2 = t.ft[tri * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= t.n_vt || i1 >= t.n_vt || i2 >= t.n_vt) return;      // (the Python layer refuses such a table: the kernel only stays in bounds)
    const float b0 = (1.0f - b1) - b2;
    const float u = ((b0 * t.vt[(int64_t)i0 * 2]) + (b1 * t.vt[(int64_t)i1 * 2])) + (b2 * t.vt[(int64_t)i2 * 2]);
    const float v = ((b0 * t.vt[(int64_t)i0 * 2 + 1]) + (b1 * t.vt[(int64_t)i1 * 2 + 1])) + (b2 * t.vt[(int64_t)i2 * 2 + 1]);
    float x = u * (float)t.W - 0.5f, y = v * (float)t.H - 0.5f;
    x = x > 0.f ? (x < (float)(t.W - 1) ? x : (float)(t.W - 1)) : 0.f;         // (a NaN fails the first comparison)
    y = y > 0.f ? (y < (float)(t.H - 1) ? y : (float)(t.H - 1)) : 0.f;
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, t.W - 1), y1 = min(y0 + 1, t.H - 1);
    const float fx = x - xf, fy = y - yf;
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

}  // namespace iris
