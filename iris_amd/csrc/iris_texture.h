// Texture export (reference: utils/export.py): the UV-space rasteriser that stands where nvdiffrast's GL rasteriser + interpolate stand in the reference, and
// the quantisation of the material network's outputs into albedo.png / rm.png.  nvdiffrast is third party: parity with it is unpinned.  The contract is this
// project's own, and it is EXACT: integer coverage, one stated float order.  tests/uv_raster_ref.py restates it in numpy.
//
//   layout      texture of H rows x W columns; texel (r, c) has its centre at u = (c + .5) / W, v = (r + .5) / H; row 0 is v ~ 0 (no flip).
//   snapping    X = llrint((double)u * W * 256), Y = llrint((double)v * H * 256): 1 / 256 texel.  A centre is (256 c + 128, 256 r + 128).
//   edges       int64, E_ab(p) = (bx - ax)(py - ay) - (by - ay)(px - ax);  A = E_01(v2);  A == 0 covers nothing;  all three times sign(A): inside is >= 0.
//               With |u|, |v| <= 2 and H, W <= 8192 every value stays below 2^47.
//   ties        E == 0 is inside only where the triangle's interior lies on the +x side of that edge, or, for an edge whose inward normal has no x component,
//               on the +y side: here E(p) = gx px + gy py + c with (gx, gy) the inward normal, so the edge keeps its zeros iff gx > 0 || (gx == 0 && gy > 0).
//   overlap     the lowest face index wins (integer atomicMin: order independent, deterministic); an uncovered texel has id -1.
//   barycentric b0 = (float)((double)E_12 / (double)|A|), b1 = (float)((double)E_20 / (double)|A|), b2 = 1.0f - b0 - b1      (weights of vertices 0, 1, 2)
//   position    per component, float32, no fused multiply-add (the build has -ffp-contract=off): ((b0 * v0) + (b1 * v1)) + (b2 * v2), v0..v2 named by f[face].
//   quantise    clamp to [0, 1] with NaN -> 0, float32 product with 255, truncated; uncovered texels 0 in every channel.
//
// Raster schedule: ids start as 0xFFFFFFFF (= -1 as int32, the largest uint32), every covering triangle does an unsigned atomicMin with its index.
//   class kernel  one lane per triangle: snap, orient, clip the bounding box of texel centres to the texture.  A box of at most `small_max` texels is walked by
//                 that lane (the ~4-texel triangles of a dense scan).  A larger one is queued: one 64-bit atomicAdd on the workspace header hands out the queue
//                 slot (high 24 bits) and the first work item (low 40 bits) TOGETHER, so the slots' first items ascend and a binary search finds an item's slot.
//   span kernel   a fixed grid of waves strides over the work items.  An item is kUvChunkSegs consecutive 64-texel row segments of ONE queued triangle's box
//                 (row-major): the wave sets the triangle up once, then its 64 lanes take 64 neighbouring texels of a row, so a wave's atomics are contiguous
//                 and no lane ever loops over a 500 x 500 box.
// A triangle that names a vertex outside [0, n_vt) covers nothing (the Python layer rejects such input before upload; the kernels only stay in bounds).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iris {

constexpr int kUvSub = 256;                 // sub-texel grid
constexpr int kUvThreads = 256;
constexpr int kUvChunkSegs = 16;            // 64-texel row segments per work item of the span kernel
constexpr int kUvSpanBlocks = 1024;         // the span kernel's fixed grid (the item count is known on the device only)
constexpr int kUvSlotBits = 24, kUvItemBits = 40;
// Boxes of at most this many texels stay with the lane that classified them.  Chosen by tools/bench_texture.py (profiles/texture_export.json; the table is in
// EXPERIMENTS.md): at 2048^2 the lane class is the faster one up to boxes of 166 texels and the slower one from 419 texels on.
constexpr int kUvSmallMaxTexels = 256;

enum { kUvModeAuto = 0, kUvModeAllSmall = 1, kUvModeAllLarge = 2 };

struct UvEdge { int64_t gx, gy, c; };       // E(px, py) = gx px + gy py + c, oriented: the inside is E >= 0
struct UvTri {
    UvEdge e[3];                            // edges 01, 12, 20
    int64_t area;                           // |A|
    int bias[3];                            // 0: the edge keeps its zeros, 1: it does not
    int c0, c1, r0, r1;                     // texel centres inside the clipped bounding box (empty when c0 > c1 or r0 > r1)
};

__device__ __forceinline__ int64_t uv_snap(float u, int n) { return llrint((double)u * (double)n * (double)kUvSub); }

// -> false when the triangle covers nothing (bad index, zero area, box without a texel centre of the texture)
__device__ __forceinline__ bool uv_setup(const float* __restrict__ vt, int64_t n_vt, const int32_t* __restrict__ ft, int64_t face, int H, int W, UvTri& t) {
    const int i0 = ft[face * 3], i1 = ft[face * 3 + 1], i2 = ft[face * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vt || i1 >= n_vt || i2 >= n_vt) return false;
    const int64_t x[3] = {uv_snap(vt[(int64_t)i0 * 2], W), uv_snap(vt[(int64_t)i1 * 2], W), uv_snap(vt[(int64_t)i2 * 2], W)};
    const int64_t y[3] = {uv_snap(vt[(int64_t)i0 * 2 + 1], H), uv_snap(vt[(int64_t)i1 * 2 + 1], H), uv_snap(vt[(int64_t)i2 * 2 + 1], H)};
    const int64_t A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
    if (A == 0) return false;
    const int64_t s = A > 0 ? 1 : -1;
    t.area = A * s;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = k, b = (k + 1) % 3;
        const int64_t gx = -s * (y[b] - y[a]), gy = s * (x[b] - x[a]);
        t.e[k] = {gx, gy, -(gx * x[a] + gy * y[a])};
        t.bias[k] = (gx > 0 || (gx == 0 && gy > 0)) ? 0 : 1;
    }
    const int64_t xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
    const int64_t ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
    // centres 256 c + 128 in [xmin, xmax]: c from ceil((xmin - 128) / 256) to floor((xmax - 128) / 256)   (>> of a negative int64 floors)
    t.c0 = (int)max((int64_t)0, (xmin - kUvSub / 2 + kUvSub - 1) >> 8);
    t.c1 = (int)min((int64_t)W - 1, (xmax - kUvSub / 2) >> 8);
    t.r0 = (int)max((int64_t)0, (ymin - kUvSub / 2 + kUvSub - 1) >> 8);
    t.r1 = (int)min((int64_t)H - 1, (ymax - kUvSub / 2) >> 8);
    return t.c0 <= t.c1 && t.r0 <= t.r1;
}

__device__ __forceinline__ int64_t uv_edge(const UvEdge& e, int64_t px, int64_t py) { return e.gx * px + e.gy * py + e.c; }
__device__ __forceinline__ bool uv_inside(const UvTri& t, int64_t px, int64_t py) {
    return uv_edge(t.e[0], px, py) >= t.bias[0] && uv_edge(t.e[1], px, py) >= t.bias[1] && uv_edge(t.e[2], px, py) >= t.bias[2];
}

struct UvQueue {                // the workspace: header (slot count << 40 | item count), then the queued triangles' first items and face indices
    unsigned long long* head;
    int64_t* first;             // (capacity)
    int32_t* face;              // (capacity)
    int64_t capacity;
};

__global__ __launch_bounds__(kUvThreads) void uv_class_kernel(const float* __restrict__ vt, int64_t n_vt, const int32_t* __restrict__ ft, int64_t F, int H, int W,
                                                              uint32_t* __restrict__ ids, UvQueue q, int64_t small_max) {
    const int64_t face = blockIdx.x * (int64_t)kUvThreads + threadIdx.x;
    if (face >= F) return;
    UvTri t;
    if (!uv_setup(vt, n_vt, ft, face, H, W, t)) return;
    const int cols = t.c1 - t.c0 + 1, rows = t.r1 - t.r0 + 1;
    if ((int64_t)cols * rows > small_max) {
        const int64_t segs = (int64_t)rows * ((cols + 63) / 64);
        const unsigned long long items = (unsigned long long)((segs + kUvChunkSegs - 1) / kUvChunkSegs);
        const unsigned long long old = atomicAdd(q.head, (1ull << kUvItemBits) | items);
        const int64_t slot = (int64_t)(old >> kUvItemBits);
        if (slot < q.capacity) {              // (always: the host sizes the queue for F triangles and keeps F below 2^24 on this path)
            q.first[slot] = (int64_t)(old & ((1ull << kUvItemBits) - 1));
            q.face[slot] = (int32_t)face;
        }
        return;
    }
    for (int r = t.r0; r <= t.r1; ++r) {
        const int64_t py = (int64_t)r * kUvSub + kUvSub / 2;
        int64_t px = (int64_t)t.c0 * kUvSub + kUvSub / 2;
        int64_t e0 = uv_edge(t.e[0], px, py) - t.bias[0], e1 = uv_edge(t.e[1], px, py) - t.bias[1], e2 = uv_edge(t.e[2], px, py) - t.bias[2];
        for (int c = t.c0; c <= t.c1; ++c) {
            if ((e0 | e1 | e2) >= 0) atomicMin(ids + (int64_t)r * W + c, (uint32_t)face);
            e0 += t.e[0].gx * kUvSub; e1 += t.e[1].gx * kUvSub; e2 += t.e[2].gx * kUvSub;
        }
    }
}

__global__ __launch_bounds__(kUvThreads) void uv_span_kernel(const float* __restrict__ vt, int64_t n_vt, const int32_t* __restrict__ ft, int H, int W,
                                                             uint32_t* __restrict__ ids, UvQueue q) {
    const unsigned long long head = *q.head;
    const int64_t n_slots = min((int64_t)(head >> kUvItemBits), q.capacity);
    const int64_t n_items = (int64_t)(head & ((1ull << kUvItemBits) - 1));
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)kUvThreads + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * kUvThreads) >> 6;
    for (int64_t item = wave; item < n_items; item += n_waves) {
        int64_t lo = 0, hi = n_slots - 1;                     // the last slot whose first item is <= item
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (q.first[mid] <= item) lo = mid; else hi = mid - 1;
        }
        const int64_t face = q.face[lo];
        UvTri t;
        if (!uv_setup(vt, n_vt, ft, face, H, W, t)) continue;  // (never: the class kernel queued it)
        const int cols = t.c1 - t.c0 + 1, rows = t.r1 - t.r0 + 1;
        const int spr = (cols + 63) / 64;                      // segments per row
        const int64_t segs = (int64_t)rows * spr;
        const int64_t s0 = (item - q.first[lo]) * kUvChunkSegs, s1 = min(s0 + kUvChunkSegs, segs);
        for (int64_t s = s0; s < s1; ++s) {
            const int r = t.r0 + (int)(s / spr), c = t.c0 + (int)(s % spr) * 64 + lane;
            if (c <= t.c1 && uv_inside(t, (int64_t)c * kUvSub + kUvSub / 2, (int64_t)r * kUvSub + kUvSub / 2))
                atomicMin(ids + (int64_t)r * W + c, (uint32_t)face);
        }
    }
}

// texels [texel0, texel0 + n): barycentrics (n, 2; NULL: not written) and position (n, 3) of the winning triangle; an uncovered texel (or a face whose
// f names a vertex outside [0, n_v)) gets zeros
__global__ __launch_bounds__(kUvThreads) void uv_resolve_kernel(const float* __restrict__ vt, int64_t n_vt, const int32_t* __restrict__ ft, const float* __restrict__ v,
                                                                int64_t n_v, const int32_t* __restrict__ f, int64_t F, int H, int W, const int32_t* __restrict__ ids,
                                                                int64_t texel0, int64_t n, float* __restrict__ bary, float* __restrict__ xyz) {
    const int64_t i = blockIdx.x * (int64_t)kUvThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t texel = texel0 + i;
    const int32_t face = ids[texel];
    float b0 = 0.f, b1 = 0.f, p[3] = {0.f, 0.f, 0.f};
    UvTri t;
    if (face >= 0 && face < F && uv_setup(vt, n_vt, ft, face, H, W, t)) {
        const int64_t px = (texel % W) * kUvSub + kUvSub / 2, py = (texel / W) * kUvSub + kUvSub / 2;
        const double area = (double)t.area;
        b0 = (float)((double)uv_edge(t.e[1], px, py) / area);
        b1 = (float)((double)uv_edge(t.e[2], px, py) / area);
        const float b2 = 1.0f - b0 - b1;
        const int j0 = f[(int64_t)face * 3], j1 = f[(int64_t)face * 3 + 1], j2 = f[(int64_t)face * 3 + 2];
        if (j0 >= 0 && j1 >= 0 && j2 >= 0 && j0 < n_v && j1 < n_v && j2 < n_v) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = ((b0 * v[(int64_t)j0 * 3 + k]) + (b1 * v[(int64_t)j1 * 3 + k])) + (b2 * v[(int64_t)j2 * 3 + k]);
        }
    }
    if (bary) { bary[i * 2] = b0; bary[i * 2 + 1] = b1; }
    xyz[i * 3] = p[0]; xyz[i * 3 + 1] = p[1]; xyz[i * 3 + 2] = p[2];
}

__device__ __forceinline__ uint32_t uv_quant(float x) {
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;        // NaN fails the first comparison: 0
    return (uint32_t)(int)(c * 255.f);
}

// One thread per group of four texels [4 g, 4 g + 4) of the TEXTURE (not of the range): its 12 bytes of either image are three aligned words.  The groups
// that the range covers only in part (its ragged ends) store bytes.
__global__ __launch_bounds__(kUvThreads) void uv_quantize_kernel(const float* __restrict__ albedo, const float* __restrict__ rough, const float* __restrict__ metal,
                                                                 const int32_t* __restrict__ ids, int64_t texel0, int64_t n, uint8_t* __restrict__ albedo_img,
                                                                 uint8_t* __restrict__ rm_img) {
    const int64_t g = texel0 / 4 + blockIdx.x * (int64_t)kUvThreads + threadIdx.x;
    const int64_t first = g * 4;
    if (first >= texel0 + n) return;
    uint32_t a[12], m[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t texel = first + k, i = texel - texel0;
        const bool in_range = i >= 0 && i < n;
        const bool covered = in_range && ids[texel] >= 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a[k * 3 + ch] = covered ? uv_quant(albedo[i * 3 + ch]) : 0u;
        m[k * 3] = covered ? uv_quant(rough[i]) : 0u;
        m[k * 3 + 1] = covered ? uv_quant(metal[i]) : 0u;
        m[k * 3 + 2] = 0u;
    }
    if (first >= texel0 && first + 4 <= texel0 + n) {
        uint32_t* pa = reinterpret_cast<uint32_t*>(albedo_img + first * 3);
        uint32_t* pm = reinterpret_cast<uint32_t*>(rm_img + first * 3);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            pa[w] = a[w * 4] | (a[w * 4 + 1] << 8) | (a[w * 4 + 2] << 16) | (a[w * 4 + 3] << 24);
            pm[w] = m[w * 4] | (m[w * 4 + 1] << 8) | (m[w * 4 + 2] << 16) | (m[w * 4 + 3] << 24);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t texel = first + k;
            if (texel < texel0 || texel >= texel0 + n) continue;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                albedo_img[texel * 3 + ch] = (uint8_t)a[k * 3 + ch];
                rm_img[texel * 3 + ch] = (uint8_t)m[k * 3 + ch];
            }
        }
    }
}

}  // namespace iris
