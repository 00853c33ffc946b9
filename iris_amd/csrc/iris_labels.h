// 5c-16: segmentation fusion (utils/fuse_segmentation.py of the reference) -- per-triangle label vote over a scene's views, and a view painted from a
// per-triangle table.
//
// The reference composes the vote from ray_intersect (five full-size outputs), a boolean-mask compaction (a host synchronisation) and scatter_add_ of int64
// ones, and the painting from ray_intersect, a gather and a masked fill.  Here each is one launch per view, one thread per pixel:
//     ray        view_ray (iris_batch.h): the ViewRays in the kernel arguments, a camera row or explicit origins / directions
//     hit        the trace_bvh4 instantiation pool_view_kernel and intersect_kernel get from with_trace: ray_intersect's closest hit, bit for bit
//     vote       hist[tri * n_labels + id] += 1 (uint32) for a hit whose pixel carries an id in [1, n_labels); column 0 is never written (nothing reads it)
//     argmax     per triangle row the column in [1, n_labels) with the highest count, the LOWER id among equal counts (numpy / torch-CPU argmax: first
//                occurrence), 0 when no column has a vote
//     view       out[i] = table[tri] on a hit, miss_value otherwise; float32 or the low byte as uint8
// Every result is an integer count or a copy: exact, independent of the order the atomics arrive in.
//
// Atomics.  Neighbouring pixels see the same triangle under the same segment, so the 64 lanes of a wave-instruction carry a handful of distinct
// (triangle, id) keys; the wave's equal keys are combined first (for_each_destination, iris_prebake.h) and the leader adds their count once.  The per-lane
// form stays behind iris_debug_set("pool_combine", 0) as the comparison arm (tools/bench_fuse_segmentation.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iris_batch.h"
#include "iris_device.h"
#include "iris_prebake.h"   // for_each_destination
#include "iris_trace.h"

namespace iris {

struct LabelViewArgs {
    ViewRays rays;
    int64_t n_tri;                // rows of hist / entries of table: a hit on a triangle beyond them counts as a miss
    // vote
    const void* ids; int ids_u8;  // the pixels' ids: float32 (truncated toward zero, as .long()) or uint8
    uint32_t* hist; int n_labels;
    int combine;                  // equal keys summed in the wave first (iris_debug_set("pool_combine"): the per-lane form for comparison)
    // view
    const int32_t* table; void* out; int out_u8; int miss_value;
};

// the id pixel i votes for, or -1: 0, negative, NaN, infinite and >= n_labels are dropped.  (The float is compared before it is converted: 1 <= f < 2^31
// holds exactly when its truncation is an int >= 1, and NaN fails every comparison.)
__device__ __forceinline__ int label_id(const LabelViewArgs& a, int64_t i) {
    int id;
    if (a.ids_u8) {
        id = ((const uint8_t*)a.ids)[i];
    } else {
        const float f = ((const float*)a.ids)[i];
        if (!(f >= 1.0f && f < 2147483648.0f)) return -1;
        id = (int)f;
    }
    return id >= 1 && id < a.n_labels ? id : -1;
}

template <int LAYOUT, bool JOINT>
__global__ __launch_bounds__(kBlock) void label_vote_kernel(SceneDev sc, LabelViewArgs a) {
    __shared__ uint32_t s_stack[kStackLds * kBlock];
    // (the loop's bound is the workgroup's, not the lane's: every lane stays for the wave-wide step below, a lane past the end with key -1)
    for (int64_t base = blockIdx.x * (int64_t)kBlock; base < a.rays.B; base += (int64_t)gridDim.x * kBlock) {
        const int64_t i = base + threadIdx.x;
        long long key = -1;
        if (i < a.rays.B) {
            const int id = label_id(a, i);
            const Ray r = view_ray(a.rays, i);
            const Hit h = trace_bvh4<LAYOUT, false, kStackLds, false, JOINT>(sc, r.o, r.d, s_stack + threadIdx.x);
            if (h.slot >= 0 && id >= 0 && h.id >= 0 && h.id < a.n_tri) key = (long long)h.id * a.n_labels + id;
        }
        if (!a.combine) {
            if (key >= 0) atomicAdd(a.hist + key, 1u);
            continue;
        }
        for_each_destination(key, [&](bool, unsigned long long lanes, bool leader) {
            if (leader) atomicAdd(a.hist + key, (uint32_t)__popcll(lanes));
        });
    }
}

// One wave per triangle row, the lanes striding over its columns; a wave takes kArgmaxRows neighbouring rows at a time so that as many independent loads
// are in flight (a 41-column row is one 164-byte load per wave: with one row at a time the kernel waits on latency, not on bytes).
// Order: higher count, then lower id; counts compare as unsigned (a row may hold more than 2^31 votes).
constexpr int kArgmaxRows = 4;
__global__ __launch_bounds__(256) void label_argmax_kernel(const uint32_t* __restrict__ hist, int64_t F, int n_labels, int32_t* __restrict__ tri_label) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = wave * kArgmaxRows; t < F; t += n_waves * kArgmaxRows) {      // (t is the wave's: the shuffles below run in uniform control flow)
        uint32_t best[kArgmaxRows]; int id[kArgmaxRows];
#pragma unroll
        for (int r = 0; r < kArgmaxRows; ++r) { best[r] = 0; id[r] = 0; }
        for (int c = 1 + lane; c < n_labels; c += 64) {   // ascending columns, strict comparison: the lower id of a lane's equal counts stays
            uint32_t v[kArgmaxRows];
#pragma unroll
            for (int r = 0; r < kArgmaxRows; ++r) v[r] = t + r < F ? hist[(t + r) * n_labels + c] : 0u;
#pragma unroll
            for (int r = 0; r < kArgmaxRows; ++r)
                if (v[r] > best[r]) { best[r] = v[r]; id[r] = c; }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
            for (int r = 0; r < kArgmaxRows; ++r) {
                const uint32_t ob = __shfl_xor(best[r], m); const int oi = __shfl_xor(id[r], m);
                if (ob > best[r] || (ob == best[r] && oi < id[r])) { best[r] = ob; id[r] = oi; }
            }
        }
#pragma unroll
        for (int r = 0; r < kArgmaxRows; ++r)
            if (lane == r && t + r < F) tri_label[t + r] = best[r] ? id[r] : 0;
    }
}

template <int LAYOUT, bool JOINT>
__global__ __launch_bounds__(kBlock) void label_view_kernel(SceneDev sc, LabelViewArgs a) {
    __shared__ uint32_t s_stack[kStackLds * kBlock];
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < a.rays.B; i += (int64_t)gridDim.x * kBlock) {
        const Ray r = view_ray(a.rays, i);
        const Hit h = trace_bvh4<LAYOUT, false, kStackLds, false, JOINT>(sc, r.o, r.d, s_stack + threadIdx.x);
        const int v = h.slot >= 0 && h.id >= 0 && h.id < a.n_tri ? a.table[h.id] : a.miss_value;
        if (a.out_u8) ((uint8_t*)a.out)[i] = (uint8_t)(v & 0xFF);      // numpy's astype(uint8) of an int: the low byte (-1 -> 255, 300 -> 44)
        else ((float*)a.out)[i] = (float)v;
    }
}

}  // namespace iris
