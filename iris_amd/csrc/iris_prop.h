// The BRDF trainer's roughness-metallic propagation regulariser (train_brdf_crf.py:212-290), forward and backward.
//
// Reference, semantic branch (:243-290): per segment, every pixel i draws K = 1024 partners j from its own segment (all members once each when the segment
// has fewer than K), weights them w = exp(-(|a_i-a_j|^2/sa^2)/2) exp(-(|p_i-p_j|^2/sp^2)/2), and is pulled towards the weighted means:
//     W_i = 1e-4 + sum w,  rbar_i = sum w r_j / W_i,  mbar_i likewise,  l_i = |rbar_i - r_i| + |mbar_i - m_i|,  loss = ls * sum over segments of mean l_i.
// It materialises the pair lists (8.4 M rows at a batch of 8192) and loops over segments on the host.  Part branch (:216-238): segment means of m and r
// weighted by (1 - r) + 1e-4 (detached), loss = lp * (mean |m - M_s| + mean |r - R_s|).
//
// Here everything works in SORTED space: `order` is torch.sort(segmentation, stable=True)'s permutation, position q of it holds pixel order[q], and a
// segment is a run [start, start + c) of positions whose members are in ascending pixel index (the order of the reference's torch.where).  A draw's local
// rank d therefore names position start + d: a dense index, and the records a pixel gathers are contiguous.  The number of segments is never needed:
// sum over segments of the mean of l = sum over pixels of l_i / c_i.
//   runs     one thread per position: lower / upper bound of its key in the sorted keys -> (start, c)
//   pack     (a.xyz, p.xyz, r, m) of pixel order[q] as one 32-B record at q (256 KB at N = 8192: L2 resident); p normalised here
//   forward  one wave per target position; lane l takes draws k = l, l + 64, ... in increasing k; xor-butterfly reduction: bitwise reproducible
//   backward one 1024-thread workgroup per chunk of kPropBwdTargets positions; per segment piece of the chunk the propagated part is summed in two LDS arrays
//            indexed by d (ds_add_f32), flushed with one contiguous global atomic per non-zero entry into a sorted-space buffer; a last kernel adds the
//            direct part and un-permutes with plain stores.  Segments above the LDS limit add straight into the sorted-space buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iris_device.h"

namespace iris {

constexpr uint32_t kPropStream = 0x50524F50u;   // Philox counter word 2 ("PROP"): the bakes use their lobe numbers 0..R there, so no counter is shared
constexpr int kPropBwdThreads = 1024;           // 16 waves: two workgroups fill a CU's 32 wave slots
constexpr int kPropBwdTargets = 32;             // target positions per backward workgroup: 256 workgroups at the trainer's batch of 8192
constexpr int kPropLdsMembers = 8192;           // largest segment summed in LDS: 2 x 4 B x 8192 = 64 KB, two workgroups per CU's 160 KB

struct PropRec { float4 ap, pm; };              // (a.x a.y a.z p.x) (p.y p.z r m)
struct PropArgs {
    const int2* runs;        // per position: (start, c) of its segment
    const int64_t* order;    // position -> pixel
    const PropRec* rec;      // per position
    const int64_t* draws;    // (N, K) local ranks by PIXEL, or NULL: Philox
    uint64_t seed;
    int n, K;
    float sa2, sp2;          // float32(sigma^2), as the reference's tensor / python-scalar division rounds it
};

__device__ __forceinline__ float prop_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // torch's abs backward: sign(0) = 0
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;        // every lane holds the same bits (a + b == b + a)
}

// Draw k of pixel `pix`: word (k / 64) % 4 of the Philox block (pix, 64 (k / 256) + k % 64).  A lane that walks k = l, l + 64, ... meets a new block
// every fourth draw and uses all four words of it; `g` remembers the block.
struct PropRng { uint32_t blk, w[4]; };
__device__ __forceinline__ uint32_t prop_word(PropRng& g, uint64_t seed, uint32_t pix, int k) {
    const uint32_t blk = (uint32_t)(((k >> 8) << 6) | (k & 63));
    if (g.blk != blk) {
        philox4x32(seed, ((uint64_t)pix << 32) | blk, kPropStream, g.w[0], g.w[1], g.w[2], g.w[3]);
        g.blk = blk;
    }
    const int j = (k >> 6) & 3;
    return j == 0 ? g.w[0] : j == 1 ? g.w[1] : j == 2 ? g.w[2] : g.w[3];
}
// local rank of draw k of a pixel whose segment has c members (k < min(c, K)); recorded ranks are clamped into the segment (the reference would raise)
__device__ __forceinline__ int prop_rank(const PropArgs& a, PropRng& g, int pix, int k, int c) {
    if (c < a.K) return k;
    if (a.draws) {
        const int64_t d = a.draws[(int64_t)pix * a.K + k];
        return (int)(d < 0 ? 0 : (d >= c ? c - 1 : d));
    }
    return (int)(prop_word(g, a.seed, (uint32_t)pix, k) % (uint32_t)c);
}
__device__ __forceinline__ float prop_weight(const PropRec& x, const PropRec& y, float sa2, float sp2) {
    const float ax = x.ap.x - y.ap.x, ay = x.ap.y - y.ap.y, az = x.ap.z - y.ap.z;
    const float px = x.ap.w - y.ap.w, py = x.pm.x - y.pm.x, pz = x.pm.y - y.pm.y;
    const float da = (ax * ax + ay * ay) + az * az, dp = (px * px + py * py) + pz * pz;
    return expf(-(da / sa2) / 2.0f) * expf(-(dp / sp2) / 2.0f);     // two exponentials, as :266-270
}

__global__ void prop_runs_kernel(const int64_t* __restrict__ keys, int n, int2* __restrict__ runs) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int64_t key = keys[p];
        int lo = 0, hi = p;                        // first position whose key is not below: in [0, p]
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
        int ulo = p + 1, uhi = n;                  // first position whose key is above: in [p + 1, n]
        while (ulo < uhi) { const int mid = (ulo + uhi) >> 1; if (keys[mid] <= key) ulo = mid + 1; else uhi = mid; }
        runs[p] = make_int2(lo, ulo - lo);
    }
}

__global__ void prop_draws_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, int n, int K, uint64_t seed, int64_t* __restrict__ draws) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < (int64_t)n * K; t += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(t / K), k = (int)(t - (int64_t)p * K);
        const int pix = (int)order[p];
        PropRng g; g.blk = 0xFFFFFFFFu;
        draws[(int64_t)pix * K + k] = (int64_t)(prop_word(g, seed, (uint32_t)pix, k) % (uint32_t)runs[p].y);
    }
}

// normalise: p = (x - vmin) / den * 2 - 1 (:244)
__global__ void prop_pack_kernel(const int64_t* __restrict__ order, const float* __restrict__ albedo, const float* __restrict__ positions,
                                 const float* __restrict__ roughness, const float* __restrict__ metallic, int n, int normalise, float vmin, float den,
                                 PropRec* __restrict__ rec) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int64_t i = order[p];
        f3 x = ld3(positions + i * 3);
        if (normalise) x = mk3((x.x - vmin) / den * 2.f - 1.f, (x.y - vmin) / den * 2.f - 1.f, (x.z - vmin) / den * 2.f - 1.f);
        PropRec r;
        r.ap = make_float4(albedo[i * 3], albedo[i * 3 + 1], albedo[i * 3 + 2], x.x);
        r.pm = make_float4(x.y, x.z, roughness[i], metallic[i]);
        rec[p] = r;
    }
}

// saved[p] = (W, sign(rbar - r), sign(mbar - m), 0); term[p] = l_p / c_p
__global__ __launch_bounds__(256) void prop_semantic_fwd_kernel(PropArgs a, float4* __restrict__ saved, float* __restrict__ term) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    for (int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < a.n; p += nwaves) {
        const int2 run = a.runs[p];
        const int pix = (int)a.order[p], c = run.y, cnt = c < a.K ? c : a.K;
        const PropRec me = a.rec[p];
        PropRng g; g.blk = 0xFFFFFFFFu;
        float sw = 0.f, sr = 0.f, sm = 0.f;
        for (int k = lane; k < cnt; k += 64) {
            const PropRec q = a.rec[run.x + prop_rank(a, g, pix, k, c)];
            const float w = prop_weight(me, q, a.sa2, a.sp2);
            sw += w; sr += q.pm.z * w; sm += q.pm.w * w;
        }
        sw = wave_sum(sw); sr = wave_sum(sr); sm = wave_sum(sm);
        if (lane == 0) {
            const float W = 1e-4f + sw;
            const float dr = sr / W - me.pm.z, dm = sm / W - me.pm.w;
            saved[p] = make_float4(W, prop_sign(dr), prop_sign(dm), 0.f);
            term[p] = (fabsf(dr) + fabsf(dm)) / (float)c;
        }
    }
}

// out[0] = scale * sum term[0..n): one workgroup, fixed order
__global__ __launch_bounds__(256) void prop_sum_kernel(const float* __restrict__ term, int n, float scale, float* __restrict__ out) {
    __shared__ float part[256];
    float s = 0.f;
    for (int t = threadIdx.x; t < n; t += 256) s += term[t];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = scale * part[0];
}

// The propagated part, in sorted space: gs[q] += sign_r(p) g_p w / W_p over the draws (p, q) (roughness), gs[n + q] likewise (metallic); g_p = ls gbar / c_p.
// gs is zero on entry.  lds_members: segments up to this size are summed in the 2 x lds_members floats of dynamic LDS first.
__global__ __launch_bounds__(kPropBwdThreads) void prop_semantic_bwd_kernel(PropArgs a, const float4* __restrict__ saved, const float* __restrict__ gbar, float ls,
                                                                           int targets, int lds_members, float* __restrict__ gs) {
    extern __shared__ float acc[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const float gl = ls * gbar[0];
    const int nchunks = (a.n + targets - 1) / targets;
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        int p = chunk * targets;
        const int end = min(a.n, p + targets);
        while (p < end) {                                   // the pieces of the segments this chunk overlaps (uniform over the workgroup)
            const int2 run = a.runs[p];
            const int c = run.y, pe = min(end, run.x + c), cnt = c < a.K ? c : a.K;
            const bool lds = c <= lds_members;
            if (lds) {
                for (int t = threadIdx.x; t < c; t += blockDim.x) { acc[t] = 0.f; acc[lds_members + t] = 0.f; }
                __syncthreads();
            }
            for (int q = p + wave; q < pe; q += nwaves) {
                const float4 s = saved[q];
                const float g = gl / (float)c;
                const float ar = s.y * g / s.x, am = s.z * g / s.x;
                if (ar == 0.f && am == 0.f) continue;
                const int pix = (int)a.order[q];
                const PropRec me = a.rec[q];
                PropRng rng; rng.blk = 0xFFFFFFFFu;
                for (int k = lane; k < cnt; k += 64) {
                    const int d = prop_rank(a, rng, pix, k, c);
                    const float w = prop_weight(me, a.rec[run.x + d], a.sa2, a.sp2);
                    if (lds) { atomicAdd(acc + d, ar * w); atomicAdd(acc + lds_members + d, am * w); }                         // ds_add_f32
                    else     { atomicAdd(gs + run.x + d, ar * w); atomicAdd(gs + a.n + run.x + d, am * w); }
                }
            }
            if (lds) {
                __syncthreads();
                for (int t = threadIdx.x; t < c; t += blockDim.x) {
                    const float vr = acc[t], vm = acc[lds_members + t];
                    if (vr != 0.f) atomicAdd(gs + run.x + t, vr);
                    if (vm != 0.f) atomicAdd(gs + a.n + run.x + t, vm);
                }
                __syncthreads();
            }
            p = pe;
        }
    }
}
// adds the direct part -sign g_p and un-permutes: every pixel is written exactly once
__global__ void prop_semantic_bwd_finish_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float4* __restrict__ saved,
                                                const float* __restrict__ gbar, float ls, const float* __restrict__ gs, int n,
                                                float* __restrict__ g_roughness, float* __restrict__ g_metallic) {
    const float gl = ls * gbar[0];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const float4 s = saved[p];
        const float g = gl / (float)runs[p].y;
        const int64_t i = order[p];
        g_roughness[i] = gs[p] - s.y * g;
        g_metallic[i] = gs[n + p] - s.z * g;
    }
}

// ---- part branch (:216-238) ----
// one wave per position, only a run's first position works: means[start] = (S, M, R, 0) of the segment, members summed lane-strided in position order
__global__ __launch_bounds__(256) void prop_part_means_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ roughness,
                                                              const float* __restrict__ metallic, int n, float4* __restrict__ means) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    for (int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n; p += nwaves) {
        const int2 run = runs[p];
        if (run.x != p) continue;
        float S = 0.f, sm = 0.f, sr = 0.f;
        for (int q = run.x + lane; q < run.x + run.y; q += 64) {
            const int64_t i = order[q];
            const float r = roughness[i], w = (1.f - r) + 1e-4f;
            S += w; sm += metallic[i] * w; sr += r * w;
        }
        S = wave_sum(S); sm = wave_sum(sm); sr = wave_sum(sr);
        if (lane == 0) means[p] = make_float4(S, sm / S, sr / S, 0.f);
    }
}
// signs[p] = (sign(m - M), sign(r - R)); term[p] = |m - M| + |r - R|
__global__ void prop_part_terms_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ roughness,
                                       const float* __restrict__ metallic, const float4* __restrict__ means, int n, float2* __restrict__ signs,
                                       float* __restrict__ term) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const float4 st = means[runs[p].x];
        const int64_t i = order[p];
        const float dm = metallic[i] - st.y, dr = roughness[i] - st.z;
        signs[p] = make_float2(prop_sign(dm), prop_sign(dr));
        term[p] = fabsf(dm) + fabsf(dr);
    }
}
// d/dm_k = lp gbar / n (sign_k - w_k / S sum over the segment of sign_i), r likewise (w detached).  One wave per position sums its segment's signs
// (small integers: exact, so the result is bitwise reproducible); simple rather than fast.
__global__ __launch_bounds__(256) void prop_part_bwd_kernel(const int2* __restrict__ runs, const int64_t* __restrict__ order, const float* __restrict__ roughness,
                                                            const float4* __restrict__ means, const float2* __restrict__ signs, const float* __restrict__ gbar,
                                                            float lp, int n, float* __restrict__ g_roughness, float* __restrict__ g_metallic) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    const float coef = lp * gbar[0] / (float)n;
    for (int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n; p += nwaves) {
        const int2 run = runs[p];
        float tm = 0.f, tr = 0.f;
        for (int q = run.x + lane; q < run.x + run.y; q += 64) { const float2 s = signs[q]; tm += s.x; tr += s.y; }
        tm = wave_sum(tm); tr = wave_sum(tr);
        if (lane == 0) {
            const int64_t i = order[p];
            const float S = means[run.x].x, w = (1.f - roughness[i]) + 1e-4f;
            const float2 s = signs[p];
            g_metallic[i] = coef * (s.x - w / S * tm);
            g_roughness[i] = coef * (s.y - w / S * tr);
        }
    }
}

}  // namespace iris
