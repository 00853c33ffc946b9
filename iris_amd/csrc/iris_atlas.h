// The area-proportional UV atlas of the texture export (iris_amd.utils.texture.area_atlas) and the seam dilation of the baked images.  No counterpart in the
// reference, which unwraps with xatlas (third party, not a dependency).  The contract is this project's own and, as the rasteriser's,
// it is EXACT: integers and float64 in one stated order, no square root, no tolerance.  tests/atlas_ref.py restates it in numpy.
//
//   measure     per face, float64 (the float32 vertices converted first), every product and sum rounded on its own (__dmul_rn / __dadd_rn: never fused), sums left
//               to right:  e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2, S = cx^2 + cy^2 + cz^2 (four times the squared area);  l0 = |p2 - p1|^2, l1 = |p0 - p2|^2,
//               l2 = |p1 - p0|^2;  corner = argmax(l0, l1, l2), the first maximum: the vertex opposite the longest edge.  A face that names a vertex outside
//               [0, n_v), or whose S is not finite or not > 0, has S = 0 and corner = 0.
//   ladder      D_j = M[j mod 2] 2^floor(j / 2), M = (1, 1.4142135623730951), j in [-800, 800]: the squared number of texels per unit area.
//   class       a cell of class k is a 2^k x 2^k texel square, KMIN = 2, 2^KMAX = R.  k_f = the smallest k in [KMIN, KMAX] with 4 16^k >= S_f D_j (one rounded
//               product); KMAX when none.  Two faces share a cell: cells_k = ceil(n_k / 2);  j fits when sum_k cells_k 4^k <= R^2.  Every k_f is non-decreasing
//               in j, and so is the sum except where a face that moves up fills the free half of a cell of the next class.  The step used is what ONE stated
//               bisection returns (iris_atlas_classes once per probe): lo = -800 (it must fit), hi = 801, mid = floor((lo + hi) / 2) becomes lo when it fits and
//               hi when not, until hi - lo = 1; j = lo.  It fits and j + 1 does not (or j = 800); a larger step that fits past such a dip is not looked for.
//   place       r = the number of lower-indexed faces of the same class (the caller's stable sort by class gives it); cell r / 2, lower half for even r, upper
//               half for odd r.  Classes from the largest down: base_k = sum_{k' > k} cells_k' 4^k', texel offset o = base_k + (r / 2) 4^k, the cell's corner
//               (x0, y0) = (even bits of o, odd bits of o) compacted: Morton order.  o is a multiple of 4^k, so the cells tile without overlap.
//   in the cell grid_atlas's two triangles, margin 0.25 texel, half gap 0.25 texel at the diagonal; with x1 = x0 + 2^k, y1 = y0 + 2^k
//                   lower  P0 = (x0 + .25, y0 + .25)   P1 = (x1 - .5, y0 + .25)    P2 = (x0 + .25, y1 - .5)
//                   upper  P0 = (x1 - .25, y1 - .25)   P1 = (x0 + .5, y1 - .25)    P2 = (x1 - .25, y0 + .5)
//               mesh corner (corner + i) mod 3 takes P_i (a rotation: the winding is kept, the longest edge lies on the diagonal); UV = texels / R, exact in
//               float32 (multiples of 0.25 below 8192 over a power of two) and on the rasteriser's 1 / 256 grid.
//   dilate      an uncovered texel (ids < 0) takes the bytes of the covered texel within Chebyshev distance n with the smallest squared Euclidean distance, then
//               the smallest row, then the smallest column; none: left alone.  Covered texels are only read, uncovered ones only written: one launch, in place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iris {

constexpr int kAtlasThreads = 256;
constexpr int kAtlasKMin = 2;
constexpr int kAtlasKMaxLimit = 13;             // R <= 8192
constexpr int kAtlasHist = 16;                  // counters of iris_atlas_classes: classes 0 .. 13, then the faces clamped at KMIN (14) and at KMAX (15)
constexpr int kAtlasJMin = -800, kAtlasJMax = 800;
constexpr int kDilateMax = 4;

__device__ __forceinline__ double atlas_sq3(double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
}

__global__ __launch_bounds__(kAtlasThreads) void atlas_measure_kernel(const float* __restrict__ v, int64_t n_v, const int32_t* __restrict__ f, int64_t F,
                                                                      double* __restrict__ S, uint8_t* __restrict__ corner) {
    const int64_t face = blockIdx.x * (int64_t)kAtlasThreads + threadIdx.x;
    if (face >= F) return;
    const int i0 = f[face * 3], i1 = f[face * 3 + 1], i2 = f[face * 3 + 2];
    double s = 0.0;
    int cn = 0;
    if (i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < n_v && i1 < n_v && i2 < n_v) {
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[0][k] = (double)v[(int64_t)i0 * 3 + k];
            p[1][k] = (double)v[(int64_t)i1 * 3 + k];
            p[2][k] = (double)v[(int64_t)i2 * 3 + k];
        }
        double e1[3], e2[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { e1[k] = __dsub_rn(p[1][k], p[0][k]); e2[k] = __dsub_rn(p[2][k], p[0][k]); d[k] = __dsub_rn(p[2][k], p[1][k]); }
        const double cx = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));
        const double cy = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
        const double cz = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
        s = atlas_sq3(cx, cy, cz);
        // l1 = |p0 - p2|^2 = |e2|^2 and l2 = |p1 - p0|^2 = |e1|^2: a difference and its negative have the same square
        const double l0 = atlas_sq3(d[0], d[1], d[2]), l1 = atlas_sq3(e2[0], e2[1], e2[2]), l2 = atlas_sq3(e1[0], e1[1], e1[2]);
        if (l1 > l0) cn = 1;
        if (l2 > (cn ? l1 : l0)) cn = 2;
        if (!(s > 0.0) || !(s <= 1.7976931348623157e308)) { s = 0.0; cn = 0; }          // zero, negative (never), NaN, infinite
    }
    S[face] = s;
    corner[face] = (uint8_t)cn;
}

// k (F) uint8 and the counters hist (kAtlasHist int64, zeroed by the caller).  A fixed grid of at most kAtlasClassBlocks workgroups strides over the faces.  A
// wave's equal classes are counted in the wave and added by one lane (as the pre-bake kernels' for_each_destination) to the workgroup's counters in LDS; the
// workgroup adds its non-zero counters to memory once, at its end.  A room's faces are nearly all of ONE class, and adds to one address are served one after the
// other (what iris_prebake.h measured for its pools); a dozen probes run per atlas, so the counter in memory sees about 14 adds per workgroup instead of one per
// wave.  (One probe of 1.0 M faces: tools/bench_atlas.py, profiles/atlas_area.json.)  Integer atomics only: the counters do not depend on scheduling.  (A
// workgroup sees at most F <= 2^23 faces: its 32-bit counters cannot wrap.)
constexpr int kAtlasClassBlocks = 1024;
__global__ __launch_bounds__(kAtlasThreads) void atlas_classes_kernel(const double* __restrict__ S, int64_t F, double D, int kmax, uint8_t* __restrict__ kcls,
                                                                      unsigned long long* __restrict__ hist) {
    __shared__ unsigned int s_hist[kAtlasHist];
    if (threadIdx.x < kAtlasHist) s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // (the trip count depends on blockIdx alone: every lane of the workgroup takes every turn, so the ballots and the barrier below are uniform)
    for (int64_t first = blockIdx.x * (int64_t)kAtlasThreads; first < F; first += (int64_t)gridDim.x * kAtlasThreads) {
        const int64_t face = first + threadIdx.x;
        int k = -1;
        bool at_min = false, at_max = false;
        if (face < F) {
            const double p = __dmul_rn(S[face], D);
            double thr = 1024.0;                                    // 4 16^KMIN
            k = kAtlasKMin;
            while (k < kmax && !(thr >= p)) { ++k; thr *= 16.0; }   // (exact: powers of two)
            at_min = 64.0 >= p;                                     // 4 16^(KMIN - 1): the rule without its lower clamp would have gone below KMIN
            at_max = !(thr >= p);                                   // here k == kmax: no class in range satisfies the rule
            kcls[face] = (uint8_t)k;
        }
        unsigned long long todo = __ballot(k >= 0);
        while (todo) {
            const int lead = __ffsll(todo) - 1;
            const bool mine = k == __shfl(k, lead);
            const unsigned long long lanes = __ballot(mine);
            if (lane == lead) atomicAdd(&s_hist[k], (unsigned int)__popcll(lanes));
            todo &= ~lanes;
        }
        const unsigned long long n_min = __ballot(at_min), n_max = __ballot(at_max);
        if (lane == 0) {
            if (n_min) atomicAdd(&s_hist[14], (unsigned int)__popcll(n_min));
            if (n_max) atomicAdd(&s_hist[15], (unsigned int)__popcll(n_max));
        }
    }
    __syncthreads();
    if (threadIdx.x < kAtlasHist && s_hist[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
}

struct AtlasTable {                 // per class: where its faces start in the order sorted by (class, face index), and its first texel offset
    int64_t start[kAtlasKMaxLimit + 1];
    int64_t base[kAtlasKMaxLimit + 1];
};

__device__ __forceinline__ uint32_t atlas_even_bits(uint32_t x) {          // bits 0, 2, 4, ... of x, compacted
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

// one lane per position i of `order`, the faces sorted by class with the face index breaking ties (a stable sort of kcls)
__global__ __launch_bounds__(kAtlasThreads) void atlas_place_kernel(const uint8_t* __restrict__ kcls, const uint8_t* __restrict__ corner,
                                                                    const int64_t* __restrict__ order, int64_t F, int R, int kmax, AtlasTable t,
                                                                    float* __restrict__ vt) {
    const int64_t i = blockIdx.x * (int64_t)kAtlasThreads + threadIdx.x;
    if (i >= F) return;
    const int64_t face = order[i];
    if (face < 0 || face >= F) return;                          // (never: order is a permutation.  vt is indexed by it)
    const int k = kcls[face];
    if (k < kAtlasKMin || k > kmax) return;
    const int64_t r = i - t.start[k];
    const int64_t o = t.base[k] + ((r >> 1) << (2 * k));
    if (r < 0 || o < 0 || o + ((int64_t)1 << (2 * k)) > (int64_t)R * R) return;          // (never: the host checked that the classes fit)
    const int x0 = (int)atlas_even_bits((uint32_t)o), y0 = (int)atlas_even_bits((uint32_t)(o >> 1));
    const int x1 = x0 + (1 << k), y1 = y0 + (1 << k);
    int q[3][2];                                                // quarter texels
    if (r & 1) { q[0][0] = 4 * x1 - 1; q[0][1] = 4 * y1 - 1; q[1][0] = 4 * x0 + 2; q[1][1] = 4 * y1 - 1; q[2][0] = 4 * x1 - 1; q[2][1] = 4 * y0 + 2; }
    else       { q[0][0] = 4 * x0 + 1; q[0][1] = 4 * y0 + 1; q[1][0] = 4 * x1 - 2; q[1][1] = 4 * y0 + 1; q[2][0] = 4 * x0 + 1; q[2][1] = 4 * y1 - 2; }
    const float scale = 0.25f / (float)R;                       // exact: R is a power of two
    const int c = corner[face] % 3;
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        const int64_t slot = face * 3 + (c + n) % 3;
        vt[slot * 2] = (float)q[n][0] * scale;                  // exact: an integer below 2^15 times a power of two
        vt[slot * 2 + 1] = (float)q[n][1] * scale;
    }
}

__global__ __launch_bounds__(kAtlasThreads) void texture_dilate_kernel(const int32_t* __restrict__ ids, int H, int W, int n, uint8_t* __restrict__ albedo_img,
                                                                       uint8_t* __restrict__ rm_img) {
    const int64_t texel = blockIdx.x * (int64_t)kAtlasThreads + threadIdx.x;
    if (texel >= (int64_t)H * W || ids[texel] >= 0) return;
    const int r = (int)(texel / W), c = (int)(texel % W);
    int best = 1 << 30;
    int64_t from = -1;
    for (int rr = max(0, r - n); rr <= min(H - 1, r + n); ++rr)
        for (int cc = max(0, c - n); cc <= min(W - 1, c + n); ++cc) {
            const int d = (rr - r) * (rr - r) + (cc - c) * (cc - c);
            if (d < best && ids[(int64_t)rr * W + cc] >= 0) { best = d; from = (int64_t)rr * W + cc; }     // rows, then columns ascend: the first of equals stays
        }
    if (from < 0) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        albedo_img[texel * 3 + ch] = albedo_img[from * 3 + ch];
        rm_img[texel * 3 + ch] = rm_img[from * 3 + ch];
    }
}

}  // namespace iris
