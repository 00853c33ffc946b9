// The camera response model EmorCRF (crf/model_crf.py:32-122): table lookup forward, its gradient, the inverse lookup and the inverse table.
//
// The reference interpolates with torch_interpolations, a third-party package with no ROCm build: parity with it is unpinned.  The interpolator here is
// the project's own contract.  Given non-decreasing knots p[0..n), values v[0..n) and a query q:
//     r = first index with p[r] >= q, clamped to n - 1 (torch.bucketize);  l = max(r - 1, 0)
//     dl = max(q - p[l], 0);  dr = max(p[r] - q, 0);  both zero -> both 1
//     out = (v[l] dr + v[r] dl) / (dl + dr)                                       in this operation order (the build has -ffp-contract=off)
//     d out / d q = (v[r] - v[l]) / (dl + dr), 0 where both were zero;   d out / d v[l] = dr / (dl + dr),  d out / d v[r] = dl / (dl + dr)
// Every operation is one correctly rounded IEEE operation, so the lookups agree with a torch restatement bit for bit.
//
//   lookup    one thread per pixel, three channels each, grid-stride; knots and the (3, n) table in LDS (16 KB at n = 1024).  On the uniform grid the
//             segment is guessed as ceil(q (n - 1)) and then walked against the stored knots until it is bucketize's: a knot of linspace(0, 1, n) in
//             float32 is not the rounding of k / (n - 1), so the guess alone is off by one next to some knots.
//   backward  g_hdr per pixel; g_table is a sum over all pixels into 3 n words: summed per workgroup in an LDS copy (ds_add_f32), every workgroup stores
//             its slab with plain stores, a second kernel adds the slabs in slab order.  No global atomics: all adders of a batch would sit on one 12-KB row.
//             The number of slabs depends on B only, so the sum differs between two runs only by the order of the LDS adds inside a workgroup.
//   inv_table get_inv_crf (:45-55): one workgroup per channel, minimum, sum and prefix sum of the neighbouring differences in LDS, then the knots'
//             values linspace(0, 1, n) interpolated at linspace(0, 1, n) (binary search: these knots are not uniform and, when a gap was added, repeat).
// Every table index is clamped before use: a NaN or infinite input gives some value, never an out-of-range read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iris {

constexpr int kCrfMaxKnots = 1024;      // 3 tables + knots + the backward's accumulator: 28 KB of LDS
constexpr int kCrfThreads = 256;
constexpr int kCrfLookupBlocks = 512;   // grid-stride beyond 131 072 pixels: the 16-KB table load is paid per workgroup
constexpr int kCrfSlabs = 256;          // most workgroups (= partial slabs) of the backward

struct CrfSeg { int l, r; float dl, dr; bool flat; };      // flat: both distances were zero (q on a repeated knot or on p[0])

__device__ __forceinline__ CrfSeg crf_finish(const float* p, int r, int n, float q) {
    CrfSeg s;
    s.r = min(max(r, 0), n - 1);
    s.l = max(s.r - 1, 0);
    s.dl = fmaxf(q - p[s.l], 0.f);
    s.dr = fmaxf(p[s.r] - q, 0.f);
    s.flat = s.dl == 0.f && s.dr == 0.f;
    if (s.flat) s.dl = s.dr = 1.f;
    return s;
}
// uniform knots (p = linspace(0, 1, n) in float32, the precondition include/iris_hip.h states): arithmetic guess, corrected against the knots
// themselves -- one step at most on that grid; on other non-decreasing knots still bucketize's segment, but O(n).  Both walks end at once for a
// NaN: every comparison is false.
__device__ __forceinline__ CrfSeg crf_segment_uniform(const float* p, int n, float q) {
    const float t = ceilf(q * (float)(n - 1));
    int r = t >= 0.f ? (t <= (float)(n - 1) ? (int)t : n - 1) : 0;      // false for a NaN -> 0
    while (r > 0 && p[r - 1] >= q) --r;
    while (r < n - 1 && p[r] < q) ++r;
    return crf_finish(p, r, n, q);
}
// any non-decreasing knots: lower bound
__device__ __forceinline__ CrfSeg crf_segment_search(const float* p, int n, float q) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (p[mid] < q) lo = mid + 1; else hi = mid; }
    return crf_finish(p, lo, n, q);
}
__device__ __forceinline__ float crf_value(const float* v, const CrfSeg& s) { return (v[s.l] * s.dr + v[s.r] * s.dl) / (s.dl + s.dr); }
__device__ __forceinline__ float crf_clip(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

struct CrfArgs {
    const float* grid;       // (n) knots: linspace(0, 1, n) as the caller's torch made it
    const float* table;      // (3, n)
    const float* exposure;   // n_exposure values, or NULL: exposure_value
    int64_t n_exposure, B;
    float exposure_value;
    int n;
};
__device__ __forceinline__ float crf_exposure(const CrfArgs& a, int64_t i) {
    return a.exposure ? a.exposure[a.n_exposure > 1 ? i : 0] : a.exposure_value;
}
// sp[0..n) = knots, sv[0..3n) = table
__device__ __forceinline__ void crf_load_tables(const CrfArgs& a, float* sp, float* sv) {
    for (int t = threadIdx.x; t < a.n; t += blockDim.x) sp[t] = a.grid[t];
    for (int t = threadIdx.x; t < 3 * a.n; t += blockDim.x) sv[t] = a.table[t];
    __syncthreads();
}

// INV = false: out = interp(table[c], clip(in * e));  INV = true: out = interp(table[c], clip(in)) / e
template <bool INV>
__global__ __launch_bounds__(kCrfThreads) void crf_lookup_kernel(CrfArgs a, const float* __restrict__ in, float* __restrict__ out) {
    extern __shared__ float crf_lds[];
    float *sp = crf_lds, *sv = crf_lds + a.n;
    crf_load_tables(a, sp, sv);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.B; i += (int64_t)gridDim.x * blockDim.x) {
        const float e = crf_exposure(a, i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = in[i * 3 + c];
            const float q = crf_clip(INV ? x : x * e);
            const float y = crf_value(sv + c * a.n, crf_segment_uniform(sp, a.n, q));
            out[i * 3 + c] = INV ? y / e : y;
        }
    }
}

// g_hdr (B, 3) and / or this workgroup's slab (3 n) of g_table; either may be NULL
__global__ __launch_bounds__(kCrfThreads) void crf_bwd_kernel(CrfArgs a, const float* __restrict__ hdr, const float* __restrict__ g_ldr, float* __restrict__ g_hdr,
                                                              float* __restrict__ slabs) {
    extern __shared__ float crf_lds[];
    float *sp = crf_lds, *sv = crf_lds + a.n, *acc = crf_lds + 4 * a.n;
    if (slabs)
        for (int t = threadIdx.x; t < 3 * a.n; t += blockDim.x) acc[t] = 0.f;
    crf_load_tables(a, sp, sv);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.B; i += (int64_t)gridDim.x * blockDim.x) {
        const float e = crf_exposure(a, i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = hdr[i * 3 + c] * e, g = g_ldr[i * 3 + c];
            const CrfSeg s = crf_segment_uniform(sp, a.n, crf_clip(x));
            const float den = s.dl + s.dr;
            if (g_hdr) {
                const float* v = sv + c * a.n;
                const float slope = s.flat ? 0.f : (v[s.r] - v[s.l]) / den;
                g_hdr[i * 3 + c] = (x >= 0.f && x <= 1.f) ? g * slope * e : 0.f;        // torch.clip passes the gradient on the closed interval
            }
            if (slabs) {
                atomicAdd(acc + c * a.n + s.l, g * (s.dr / den));        // ds_add_f32 (seen in the gfx950 assembly of this build's flags: six, no compare-and-swap loop)
                atomicAdd(acc + c * a.n + s.r, g * (s.dl / den));
            }
        }
    }
    if (slabs) {
        __syncthreads();
        float* mine = slabs + (int64_t)blockIdx.x * 3 * a.n;
        for (int t = threadIdx.x; t < 3 * a.n; t += blockDim.x) mine[t] = acc[t];
    }
}
// g_table[t] = slab 0 + slab 1 + ... in that order
__global__ void crf_slab_sum_kernel(const float* __restrict__ slabs, int n_slabs, int m, float* __restrict__ g_table) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < n_slabs; ++k) s += slabs[(int64_t)k * m + t];
        g_table[t] = s;
    }
}

// get_inv_crf: block c handles channel c with kCrfMaxKnots threads, thread t owns difference t = crf[t + 1] - crf[t] (t < n - 1)
__global__ __launch_bounds__(kCrfMaxKnots) void crf_inv_table_kernel(const float* __restrict__ grid, const float* __restrict__ table, int n, float* __restrict__ inv) {
    __shared__ float knots[kCrfMaxKnots], red[kCrfMaxKnots], scan[2][kCrfMaxKnots], sx[kCrfMaxKnots];
    const int t = threadIdx.x, m = n - 1;
    const float* crf = table + (int64_t)blockIdx.x * n;
    float d = t < m ? crf[t + 1] - crf[t] : 0.f;
    if (t < n) sx[t] = grid[t];
    red[t] = t < m ? d : INFINITY;
    __syncthreads();
    for (int o = kCrfMaxKnots / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = fminf(red[t], red[t + o]);
        __syncthreads();
    }
    const float dmin = red[0];
    __syncthreads();
    if (dmin < 0.f && t < m) d += -dmin;
    red[t] = d;                                   // 0 beyond the last difference
    __syncthreads();
    for (int o = kCrfMaxKnots / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    d = d / red[0];
    int cur = 0;
    scan[0][t] = d;
    __syncthreads();
    for (int o = 1; o < kCrfMaxKnots; o <<= 1) {  // inclusive prefix sum, Hillis-Steele
        scan[cur ^ 1][t] = t >= o ? scan[cur][t - o] + scan[cur][t] : scan[cur][t];
        cur ^= 1;
        __syncthreads();
    }
    if (t == 0) knots[0] = 0.f;
    if (t < m) knots[t + 1] = scan[cur][t];
    __syncthreads();
    if (t < n) inv[(int64_t)blockIdx.x * n + t] = crf_value(sx, crf_segment_search(knots, n, sx[t]));
}

}  // namespace iris
