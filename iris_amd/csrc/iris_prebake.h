// 5c-11: the stages BEFORE the bake (slf_bake.py, slf_refine.py, extract_emitter_ldr.py) -- one view's primary hits pooled where they land.
//
// The reference, and this project's first version of these stages, compose a pass over a view from a ray generator, ray_intersect (five full-size
// outputs), two boolean-mask compactions (each a host synchronisation), the response model's inverse over a float copy of the photograph, and a scatter.
// pool_view_kernel is that pass as one launch, one thread per pixel:
//     ray        view_ray (iris_batch.h): the ViewRays in the kernel arguments, a camera row or explicit origins / directions
//     hit        the trace_bvh4 instantiation intersect_kernel gets from with_trace, hit_vertices, hit_position; a miss contributes to nothing
//     radiance   3 bytes of an 8-bit photograph through a 3 x 256 table in LDS (the decode float(double(u) / 255), and behind it the inverse response of
//                that value when a response model is given: 768 lookups per workgroup instead of three per pixel, the same bits), or three floats
//                of a float32 store through the same crf_segment_uniform / crf_value / crf_clip arithmetic as crf_lookup_kernel<true>; then / exposure
//     sinks      any of: bounds (min and max over the coordinates of the hit positions), occupancy histogram, voxel pool, triangle pool
// Nothing else is written: no valid mask, no compacted copies, no float photograph.
//
// Atomics.  A 1080p view is about 2 M hits x 16 B = 32 MB of atomically added bytes per pass; over the chip-wide rate for well-spread adds that is well under a
// millisecond.  Measured, it is not: neighbouring pixels share their destination, and the per-lane form is bound by adds to ONE address (see
// for_each_destination below, which combines a wave's equal destinations first; the per-lane form stays behind iris_debug_set("pool_combine", 0) as the
// comparison arm, and in the three kernels whose bodies pool_hist / pool_voxel / pool_triangle are).  The bounds have one destination by construction: they
// are reduced in the wave (shuffles) and in the workgroup (LDS), and one lane issues two integer atomics per workgroup.  Float sums equal a sequential scatter
// up to summation order; counts, histogram and bounds are exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iris_batch.h"
#include "iris_crf.h"
#include "iris_device.h"
#include "iris_prop.h"      // wave_sum
#include "iris_trace.h"

namespace iris {

// ---- the three pooling bodies (also the bodies of voxel_histogram_kernel, slf_scatter_add_kernel and scatter_add_rows_kernel) ----
// slf_bake.py:104-110: hist[x + y*H + z*H*H] += 1 (float counts, exact below 2^24); s carries H, vmin and den only
__device__ __forceinline__ void pool_hist(float* __restrict__ hist, const SlfDev& s, f3 p) {
    const int cx = voxel_coord(p.x, s), cy = voxel_coord(p.y, s), cz = voxel_coord(p.z, s);
    atomicAdd(hist + ((int64_t)cz * s.H + cy) * s.H + cx, 1.0f);
}
// VoxelSLF.scatter_add (model/slf.py:56-61); a position whose voxel is empty (index -1) is dropped
__device__ __forceinline__ void pool_voxel(const SlfDev& s, f3 p, f3 rgb, float* __restrict__ acc, unsigned long long* __restrict__ count) {
    const int j = slf_index(s, p);
    if (j < 0) return;
    atomicAdd(acc + (int64_t)j * 3, rgb.x); atomicAdd(acc + (int64_t)j * 3 + 1, rgb.y); atomicAdd(acc + (int64_t)j * 3 + 2, rgb.z);
    atomicAdd(count + j, 1ull);
}
// extract_emitter_ldr.py:90-95: out[j] += rgb, count[j] += 1; j outside [0, F) skipped
__device__ __forceinline__ void pool_triangle(int64_t j, int64_t F, f3 rgb, float* __restrict__ out, float* __restrict__ count) {
    if (j < 0 || j >= F) return;
    atomicAdd(out + j * 3, rgb.x); atomicAdd(out + j * 3 + 1, rgb.y); atomicAdd(out + j * 3 + 2, rgb.z);
    if (count) atomicAdd(count + j, 1.0f);
}

// ---- min / max of finite floats kept in a float word, by integer atomics ----
// For x >= 0 the bits of a float order as signed integers do; for x < 0 as unsigned integers, reversed.  A non-negative candidate therefore goes through
// the signed atomic (any negative word compares below it, as it must), a negative one through the reversed unsigned atomic (any non-negative word compares
// below it as unsigned).  -0 is made +0 first (its bits are INT_MIN): the word's VALUE is exact, a zero's sign is not kept.
__device__ __forceinline__ void atomic_min_float(float* addr, float x) {
    x = x + 0.0f;
    if (x >= 0.f) atomicMin((int*)addr, __float_as_int(x));
    else atomicMax((unsigned int*)addr, __float_as_uint(x));
}
__device__ __forceinline__ void atomic_max_float(float* addr, float x) {
    x = x + 0.0f;
    if (x >= 0.f) atomicMax((int*)addr, __float_as_int(x));
    else atomicMin((unsigned int*)addr, __float_as_uint(x));
}

// ---- equal destinations combined in the wave before the atomic ----
// Neighbouring pixels land in the same voxel and on the same triangle: at 1080p in the bench scene the 2.07 M hits of a view share 4 807 voxels, and the
// 64 lanes of a wave-instruction carry a handful of distinct addresses.  Adds to ONE address are served one after the other at the memory side: measured
// (tools/bench_prebake.py, profiles/prebake_1080p.json) the per-lane form spends 1.7 ms of a 1.96-ms voxel-pool pass in its atomics, not the "well under a
// millisecond" that bytes over the chip-wide rate gives -- that rate is for adders spread over rows.  for_each_destination calls body(mine, lanes, leader) once
// per distinct key >= 0 in the wave, in uniform control flow (every lane of the wave takes part, a lane without a destination with key -1): the members sum in
// the wave and the leader issues one set of atomics.  Sums are still sums of the same terms in another order; counts are the members' count, exact.
template <class Body>
__device__ __forceinline__ void for_each_destination(long long key, Body&& body) {
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int lead = __ffsll(todo) - 1;
        const bool mine = key == __shfl(key, lead);
        const unsigned long long lanes = __ballot(mine);
        body(mine, lanes, (int)(threadIdx.x & 63) == lead);
        todo &= ~lanes;
    }
}
// one wave's adds of (rgb, 1) to row `key` of a (rows, 3) sum and a count of type C (key < 0: none)
template <class C>
__device__ __forceinline__ void pool_rows_combined(long long key, f3 rgb, float* __restrict__ sum, C* __restrict__ count) {
    for_each_destination(key, [&](bool mine, unsigned long long lanes, bool leader) {
        const float sx = wave_sum(mine ? rgb.x : 0.f);
        const float sy = wave_sum(mine ? rgb.y : 0.f);
        const float sz = wave_sum(mine ? rgb.z : 0.f);
        if (leader) {
            atomicAdd(sum + key * 3, sx); atomicAdd(sum + key * 3 + 1, sy); atomicAdd(sum + key * 3 + 2, sz);
            if (count) atomicAdd(count + key, (C)__popcll(lanes));
        }
    });
}

struct PoolViewArgs {
    ViewRays rays;
    // radiance (NULL: none; the pooling sinks need it)
    const void* rgb; int rgb_u8;
    CrfArgs crf;                  // grid NULL: no response model; table = the (3, n) INVERSE table; exposure as crf_exposure reads it
    // sinks
    float* bounds;                // [min, max]
    float* hist; SlfDev hist_grid;
    int has_slf; SlfDev slf; float* slf_acc; unsigned long long* slf_count;
    float* tri_sum; float* tri_count; int64_t n_tri;
    int combine;                  // equal destinations summed in the wave first (iris_debug_set("pool_combine"): the per-lane form for comparison)
};

template <int LAYOUT, bool JOINT>
__global__ __launch_bounds__(kBlock) void pool_view_kernel(SceneDev sc, PoolViewArgs a) {
    __shared__ uint32_t s_stack[kStackLds * kBlock];
    __shared__ float s_lut[3 * 256];
    __shared__ float s_lo[kBlock / 64], s_hi[kBlock / 64];
    const bool want_rgb = a.rgb && (a.has_slf || a.tri_sum);
    const bool crf = a.crf.grid != nullptr;
    if (want_rgb && a.rgb_u8) {
        // u -> np.float32(u / 255.0) (pixel_batch_kernel's table), then, per channel, what crf_lookup_kernel<true> makes of that value before its division
        for (int t = threadIdx.x; t < 3 * 256; t += kBlock) {
            const int c = t >> 8;
            const float x = (float)((double)(t & 255) / 255.0);
            s_lut[t] = crf ? crf_value(a.crf.table + c * a.crf.n, crf_segment_uniform(a.crf.grid, a.crf.n, crf_clip(x))) : x;
        }
        __syncthreads();
    }
    float lo = INFINITY, hi = -INFINITY;
    // (the loop's bound is the workgroup's, not the lane's: every lane stays for the wave-wide steps below, a lane past the end as a miss)
    for (int64_t base = blockIdx.x * (int64_t)kBlock; base < a.rays.B; base += (int64_t)gridDim.x * kBlock) {
        const int64_t i = base + threadIdx.x;
        Hit h; h.slot = -1; h.id = -1;
        f3 p = mk3(0.f, 0.f, 0.f), rgb = mk3(0.f, 0.f, 0.f);
        if (i < a.rays.B) {
            const Ray r = view_ray(a.rays, i);
            h = trace_bvh4<LAYOUT, false, kStackLds, false, JOINT>(sc, r.o, r.d, s_stack + threadIdx.x);
        }
        const bool hit = h.slot >= 0;
        if (hit) {
            f3 p0, p1, p2;
            hit_vertices(sc, h, p0, p1, p2);
            p = hit_position(h, p0, p1, p2);
            if (a.bounds) {
                lo = fminf(lo, fminf(p.x, fminf(p.y, p.z)));
                hi = fmaxf(hi, fmaxf(p.x, fmaxf(p.y, p.z)));
            }
            if (want_rgb) {
                if (a.rgb_u8) {
                    const uint8_t* u = (const uint8_t*)a.rgb + i * 3;
                    rgb = mk3(s_lut[u[0]], s_lut[256 + u[1]], s_lut[512 + u[2]]);
                } else {
                    rgb = ld3((const float*)a.rgb + i * 3);
                    if (crf) {
                        rgb.x = crf_value(a.crf.table, crf_segment_uniform(a.crf.grid, a.crf.n, crf_clip(rgb.x)));
                        rgb.y = crf_value(a.crf.table + a.crf.n, crf_segment_uniform(a.crf.grid, a.crf.n, crf_clip(rgb.y)));
                        rgb.z = crf_value(a.crf.table + 2 * a.crf.n, crf_segment_uniform(a.crf.grid, a.crf.n, crf_clip(rgb.z)));
                    }
                }
                if (crf) {
                    const float e = crf_exposure(a.crf, i);
                    rgb = mk3(rgb.x / e, rgb.y / e, rgb.z / e);
                }
            }
        }
        if (!a.combine) {
            if (hit) {
                if (a.hist) pool_hist(a.hist, a.hist_grid, p);
                if (want_rgb && a.has_slf) pool_voxel(a.slf, p, rgb, a.slf_acc, a.slf_count);
                if (want_rgb && a.tri_sum) pool_triangle(h.id, a.n_tri, rgb, a.tri_sum, a.tri_count);
            }
            continue;
        }
        // the same three sinks with the wave's equal destinations combined; the branches are uniform, every lane of the wave is here
        if (a.hist) {
            long long key = -1;
            if (hit) {
                const SlfDev& s = a.hist_grid;
                key = ((long long)voxel_coord(p.z, s) * s.H + voxel_coord(p.y, s)) * s.H + voxel_coord(p.x, s);
            }
            for_each_destination(key, [&](bool, unsigned long long lanes, bool leader) {
                if (leader) atomicAdd(a.hist + key, (float)__popcll(lanes));
            });
        }
        if (want_rgb && a.has_slf) pool_rows_combined(hit ? (long long)slf_index(a.slf, p) : -1, rgb, a.slf_acc, a.slf_count);
        if (want_rgb && a.tri_sum) pool_rows_combined(hit && h.id < a.n_tri ? (long long)h.id : -1, rgb, a.tri_sum, a.tri_count);
    }
    if (a.bounds) {      // (a.bounds is uniform: every lane of the workgroup is here)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, m));
            hi = fmaxf(hi, __shfl_xor(hi, m));
        }
        if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 1; w < kBlock / 64; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
            if (lo <= hi) {      // at least one hit in this workgroup
                atomic_min_float(a.bounds, lo);
                atomic_max_float(a.bounds + 1, hi);
            }
        }
    }
}

}  // namespace iris
