// The material network of the reference's refine / emitter-training / BRDF-training stages: NGPBRDF.forward (model/brdf.py:213-260) =
// tiny-cuda-nn NetworkWithInputEncoding(3 -> HashGrid{32 levels x 2 features, 2^19 entries, base 16, x 1.3} -> FullyFusedMLP{64 x 2 hidden, ReLU} -> 5)
// + sigmoid, forward AND backward with respect to the parameters (train_brdf_crf.py:163-207 trains it; positions never need a gradient).
// tiny-cuda-nn is third party and CUDA only: what is implemented is its published algorithm (Mueller et al. 2022, section 3), restated
// for the tests in oracle/ngp_torch.py ("parity unpinned").
//
//   ngp_encode_kernel  one thread per (point, level), blockIdx.y = level: the blocks of a level are dispatched together, so the 8 x 4-B corner gathers
//                      of a wave go to ONE level's table (<= 2 MiB of half2 entries: it lives in an XCD's 4 MiB L2 while the level is being worked on).
//                      Features go to a [level][point] half2 plane: 256 contiguous bytes per wave-store.  Gather-bound (L2 / Infinity Cache lines).
//   ngp_mlp_kernel     the 64 -> 64 -> 64 -> 16 perceptron on the matrix cores: v_mfma_f32_32x32x16_f16, one wave per 32 points, the weights of all
//                      three layers resident in registers as A fragments, the activations handed from one layer's accumulators to the next layer's B
//                      operand WITHOUT leaving the registers (a 32x32 f32 accumulator tile has the point on the lane and the neuron in the register
//                      index; the next layer's weights are loaded in the matching permuted k order).  This IS a dense contraction (the bake path is not).
//
// Backward (straight-through: every rounding to half of the forward has derivative 1; nothing is saved by the forward, the backward re-encodes and recomputes):
//   ngp_mlp_bwd_kernel       same wave / tile shape as ngp_mlp_kernel, the forward recomputed by the same fragment code (ngp_forward_tile), then
//                            dz3 = g * s (1 - s) * loss_scale -> half; the data gradients dH2 = W3^T dz3, dH1 = W2^T dz2, dX = W1^T dz1 with the TRANSPOSED
//                            weights as A fragments in the permuted k order (accumulators feed the next MFMA from the registers; the fragments themselves
//                            are read from LDS, the registers go to the 160 accumulators of the weight gradient); the weight gradients
//                            dW = dz H^T contract over the POINTS: both operands go through a wave-private LDS tile [neuron][32 points] so that the point
//                            lies on k; f32 accumulators over the wave's whole tile loop, the 4 waves of a workgroup summed in LDS in wave order, one
//                            9216-float slab per workgroup.  dX goes to a [level][point] float2 plane (still carrying the loss scale).
//   ngp_wgrad_reduce_kernel  sums the slabs in slab order, * 1 / loss_scale, ADDS into grad_params[0 : 9216]: no float atomics, bitwise reproducible.
//   ngp_grid_bwd_kernel      one thread per (point, level) as the encode, the cell / weights / indices from the SAME helper (ngp_cell / ngp_corner_pair /
//                            ngp_corner_weight): wgt * dX / loss_scale into grad_params[9216 + 2 (offset + idx) + f] with f32 atomic adds (order-dependent).
//   ngp_params_cast_kernel   f32 master parameters on the device -> half weights + half2 tables (round to nearest even, as iris_ngp_create's host conversion).
#pragma once
#include "iris_device.h"

namespace iris {

constexpr int kNgpLevels = 32, kNgpWidth = 64, kNgpOutPad = 16, kNgpOut = 5;
constexpr int kNgpMlpParams = kNgpWidth * 64 + kNgpWidth * kNgpWidth + kNgpOutPad * kNgpWidth;   // 9216 halves: W1 (64 x 64), W2 (64 x 64), W3 (16 x 64), row-major (out x in)

struct NgpLevels {
    float scale[kNgpLevels];
    uint32_t res[kNgpLevels];
    uint32_t size[kNgpLevels];     // table entries of the level
    uint32_t offset[kNgpLevels];   // first entry of the level in the table
};
struct NgpArgs {
    NgpLevels lv;
    const uint32_t* grid;          // half2 entries (two features), all levels
    const _Float16* w;             // kNgpMlpParams halves
    const float* pos;              // (N, 3) world space
    uint32_t* feat;                // [level][n_chunk] half2
    float* albedo; float* rough; float* metal;   // (N,3), (N), (N)
    int64_t n0;                    // first point of this chunk
    int n;                         // points in this chunk
    int n_chunk;                   // plane stride of feat
    float vmin, den;               // voxel_min, float32(voxel_max - voxel_min)
};

typedef _Float16 iris_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 iris_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 iris_h2v __attribute__((ext_vector_type(2)));
typedef float iris_f16v __attribute__((ext_vector_type(16)));
typedef uint32_t ngp_u2a __attribute__((ext_vector_type(2), aligned(4)));     // two adjacent table entries, 4-byte aligned

// tiny-cuda-nn grid.h, kernel_grid, restated: position -> cell + weights, 8 corners, dense index while it fits the table, coherent prime hash otherwise.
// ONE helper for the encode and for the grid backward: the indices a gradient is scattered to are the indices the forward gathered from.
struct NgpCell {
    float w[3]; uint32_t cell[3];
    uint32_t stride1, stride2, size;
    bool hashed;
};
__device__ __forceinline__ void ngp_cell(const NgpArgs& a, int level, int i, NgpCell& q) {
    const float scale = a.lv.scale[level];
    const uint32_t res = a.lv.res[level], size = a.lv.size[level];
    const float* pp = a.pos + (a.n0 + i) * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        // model/brdf.py:252-254: (position - voxel_min) / (voxel_max - voxel_min), then * 2 - 1
        const float x = (pp[d] - a.vmin) / a.den * 2.0f - 1.0f;
        const float p = fmaf(scale, x, 0.5f);
        const float fl = floorf(p);
        q.w[d] = p - fl;
        q.cell[d] = (uint32_t)(int)fl;                // negative cells wrap, as in the library
    }
    // dense indexing covers as many dimensions as fit the table (wave-uniform: a property of the level)
    {
        uint64_t s = 1; int dims = 0;
        uint32_t st[3] = {0, 0, 0};
        for (int d = 0; d < 3 && s <= size; ++d) { st[d] = (uint32_t)s; s *= res; ++dims; }
        q.stride1 = st[1]; q.stride2 = st[2];
        q.hashed = (uint64_t)size < s;
        if (dims < 3 && !q.hashed) q.hashed = true;   // (cannot happen: the loop only stops early once the stride exceeds the table)
    }
    q.size = size;
}
// table indices of the two x-neighbours of corner pair c (c = 0, 2, 4, 6: bit 1 = y + 1, bit 2 = z + 1), the library's corner order (x fastest)
__device__ __forceinline__ void ngp_corner_pair(const NgpCell& q, int c, uint32_t& ia, uint32_t& ib) {
    uint32_t g1 = (c & 2) ? q.cell[1] + 1u : q.cell[1], g2 = (c & 4) ? q.cell[2] + 1u : q.cell[2];
    if (q.hashed) { const uint32_t k = (g1 * 2654435761u) ^ (g2 * 805459861u); ia = (q.cell[0] * 1u) ^ k; ib = ((q.cell[0] + 1u) * 1u) ^ k; }
    else { const uint32_t k = g1 * q.stride1 + g2 * q.stride2; ia = q.cell[0] + k; ib = q.cell[0] + 1u + k; }
    ia %= q.size; ib %= q.size;
}
// trilinear weight of corner c + xx (xx = 0 / 1: the x-neighbour)
__device__ __forceinline__ float ngp_corner_weight(const NgpCell& q, int c, int xx) {
    float wgt = 1.0f;
    wgt = xx ? wgt * q.w[0] : wgt * (1.0f - q.w[0]);
    wgt = (c & 2) ? wgt * q.w[1] : wgt * (1.0f - q.w[1]);
    wgt = (c & 4) ? wgt * q.w[2] : wgt * (1.0f - q.w[2]);
    return wgt;
}

__global__ __launch_bounds__(256) void ngp_encode_kernel(NgpArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int level = blockIdx.y;
    if (i >= a.n) return;
    const uint32_t* table = a.grid + a.lv.offset[level];
    NgpCell q;
    ngp_cell(a, level, i, q);
    _Float16 acc0 = (_Float16)0.f, acc1 = (_Float16)0.f;
    // The 8 corners in the library's order (x fastest), two x-neighbours at a time.  What bounds this kernel is the number of 64-B requests its gathers send
    // to the L2s (profiles/r4_ngp_pmc.json), and the two x-neighbours of a cell are adjacent table entries whenever the indexing lets them be -- always on a dense
    // level, for even x on a hashed one (x ^ K and (x + 1) ^ K differ in bit 0 only) --: one 8-byte load then fetches both.
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        uint32_t ia, ib;
        ngp_corner_pair(q, c, ia, ib);
        uint32_t ra, rb;
        // (the pair's base is an ODD entry about half the time on dense levels: the 8-byte load goes through a vector type declared 4-byte aligned -- gfx950
        //  global memory runs in unaligned-access mode, so it is still ONE global_load_dwordx2, and no C++ alignment rule is broken)
        if (ib == ia + 1u) { const ngp_u2a v = *reinterpret_cast<const ngp_u2a*>(table + ia); ra = v.x; rb = v.y; }
        else if (ia == ib + 1u) { const ngp_u2a v = *reinterpret_cast<const ngp_u2a*>(table + ib); ra = v.y; rb = v.x; }
        else { ra = table[ia]; rb = table[ib]; }
#pragma unroll
        for (int xx = 0; xx < 2; ++xx) {
            const float wgt = ngp_corner_weight(q, c, xx);
            const iris_h2v v = __builtin_bit_cast(iris_h2v, xx ? rb : ra);
            // result += (half)(weight * value): every term rounded to half, the sum a half add.  The product is rounded to f32 FIRST and then to half, as a
            // C compiler for any other target does it: behind the barrier hipcc cannot fold the multiplication into v_fma_mixlo_f16, which rounds the exact
            // product to half once -- measured different from the two-step rounding in 1.4e-4 of the features (tests/test_ngp.py compares bit for bit).
            float t0 = wgt * (float)v.x, t1 = wgt * (float)v.y;
            asm volatile("" : "+v"(t0), "+v"(t1));
            acc0 = (_Float16)((float)acc0 + (float)(_Float16)t0);
            acc1 = (_Float16)((float)acc1 + (float)(_Float16)t1);
        }
    }
    iris_h2v o; o.x = acc0; o.y = acc1;
    a.feat[(size_t)level * a.n_chunk + i] = __builtin_bit_cast(uint32_t, o);
}

__device__ __forceinline__ float ngp_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// The reference's output stage (model/brdf.py:255): tiny-cuda-nn hands back HALF, `.sigmoid()` is taken on that half tensor (torch: f32 arithmetic, ONE rounding
// to half) and only then `.float()` -- every albedo / metallic value, and the roughness before `* 0.98 + 0.02`, lies on the half grid.
__device__ __forceinline__ float ngp_out(float acc) { return (float)(_Float16)ngp_sigmoid((float)(_Float16)acc); }

// relu + f32 -> f16 of 8 accumulator registers: the B fragment of the next layer's k-step
__device__ __forceinline__ iris_h8 ngp_pack_relu(const iris_f16v& acc, int s) {
    iris_h8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float v = acc[8 * s + j]; r[j] = (_Float16)(v > 0.f ? v : 0.f); }
    return r;
}
// A fragment of a layer whose B operand is the previous layer's accumulator tile `b`, k-step s: element j is input neuron
// 32 b + 16 s + 8 (j >> 2) + 4 h + (j & 3)  (the row an accumulator register holds: row = (reg & 3) + 8 (reg >> 2) + 4 h)
__device__ __forceinline__ iris_h8 ngp_load_a_perm(const _Float16* W, int row, int b, int s, int h, bool valid) {
    iris_h8 r;
    const int k0 = 32 * b + 16 * s + 4 * h;
    const iris_h4 lo = valid ? *reinterpret_cast<const iris_h4*>(W + row * kNgpWidth + k0) : iris_h4{0, 0, 0, 0};
    const iris_h4 hi = valid ? *reinterpret_cast<const iris_h4*>(W + row * kNgpWidth + k0 + 8) : iris_h4{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[j] = lo[j]; r[4 + j] = hi[j]; }
    return r;
}

// The weights of the three layers as A fragments (the forward kernel and the backward's recomputation)
struct NgpWeights { iris_h8 a1[2][4], a2[2][2][2], a3[2][2]; };
__device__ __forceinline__ void ngp_load_weights(const _Float16* w, int r, int h, NgpWeights& W) {
    const _Float16* W1 = w;
    const _Float16* W2 = w + kNgpWidth * 64;
    const _Float16* W3 = W2 + kNgpWidth * kNgpWidth;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < 4; ++s) W.a1[b][s] = *reinterpret_cast<const iris_h8*>(W1 + (32 * b + r) * 64 + 16 * s + 8 * h);     // natural k order: k = 16 s + 8 h + j
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 2; ++s) W.a2[b2][b][s] = ngp_load_a_perm(W2, 32 * b2 + r, b, s, h, true);
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < 2; ++s) W.a3[b][s] = ngp_load_a_perm(W3, r, b, s, h, r < kNgpOutPad);                               // rows 16 .. 31 of the 32-row tile are zero
}
// The three layers of one 32-point tile: pre-activations of the two hidden layers and of the output layer in accumulator layout
// (row = neuron = (reg & 3) + 8 (reg >> 2) + 4 h [+ 32 b], column = point = lane & 31), the input features as the layer-1 B fragments.
__device__ __forceinline__ void ngp_forward_tile(const NgpArgs& a, const NgpWeights& W, int pt, bool pv, int h, iris_h8 (&xf)[4], iris_f16v (&acc1)[2], iris_f16v (&acc2)[2], iris_f16v& acc3) {
    // layer 1: B fragment of k-step s = features 16 s + 8 h .. + 7 of point pt = levels 8 s + 4 h .. + 3 (two features each)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc1[b][q] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        uint32_t f[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] = pv ? a.feat[(size_t)(8 * s + 4 * h + q) * a.n_chunk + pt] : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const iris_h2v v = __builtin_bit_cast(iris_h2v, f[q]); xf[s][2 * q] = v.x; xf[s][2 * q + 1] = v.y; }
#pragma unroll
        for (int b = 0; b < 2; ++b) acc1[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.a1[b][s], xf[s], acc1[b], 0, 0, 0);
    }
    // layer 2: relu(H1) straight from the accumulators
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc2[b][q] = 0.f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const iris_h8 bf = ngp_pack_relu(acc1[b], s);
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) acc2[b2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.a2[b2][b][s], bf, acc2[b2], 0, 0, 0);
        }
    // output layer (no activation)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc3[q] = 0.f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.a3[b][s], ngp_pack_relu(acc2[b], s), acc3, 0, 0, 0);
}

// One wave = 32 points per trip; 4 waves per workgroup, persistent over the chunk's 32-point tiles.
__global__ __launch_bounds__(256) void ngp_mlp_kernel(NgpArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    // weights as A fragments, resident for the life of the wave
    NgpWeights W;
    ngp_load_weights(a.w, r, h, W);

    const int n_tiles = (a.n + 31) >> 5;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (gridDim.x * 256) >> 6;
    for (int t = wave; t < n_tiles; t += n_waves) {
        const int pt = t * 32 + r;
        const bool pv = pt < a.n;
        iris_h8 xf[4];
        iris_f16v acc1[2], acc2[2], acc3;
        ngp_forward_tile(a, W, pt, pv, h, xf, acc1, acc2, acc3);
        // accumulator row = (reg & 3) + 8 (reg >> 2) + 4 h: lanes h = 0 hold outputs 0 .. 3 in registers 0 .. 3, lanes h = 1 output 4 in register 0
        if (pv) {
            const int64_t g = a.n0 + pt;
            if (h == 0) {
                // model/brdf.py:255-260: half -> sigmoid -> half -> float; albedo = [..., :3], roughness = [..., 3:4] * 0.98 + 0.02
                a.albedo[g * 3] = ngp_out(acc3[0]); a.albedo[g * 3 + 1] = ngp_out(acc3[1]); a.albedo[g * 3 + 2] = ngp_out(acc3[2]);
                a.rough[g] = ngp_out(acc3[3]) * 0.98f + 0.02f;          // (in f32, after .float(): model/brdf.py:258)
            } else {
                a.metal[g] = ngp_out(acc3[0]);
            }
        }
    }
}

// ======================================================================================================
// backward with respect to the parameters
// ======================================================================================================
struct NgpBwdArgs {
    NgpArgs f;                     // what the forward of this chunk was launched with (its output pointers unused)
    const float* g_albedo; const float* g_rough; const float* g_metal;      // cotangents (N,3), (N), (N)
    float2* dx;                    // [level][n_plane]: d loss / d feature (2 per level), still multiplied by loss_scale
    int n_plane;                   // plane stride of dx
    float* slabs;                  // [gridDim.x of ngp_mlp_bwd_kernel][kNgpMlpParams]: one weight-gradient partial sum per workgroup
    int n_slabs;
    float* grad;                   // grad_params (n_params f32), ADDED to
    float loss_scale, inv_scale;
};
constexpr int kNgpBwdMaxGroups = 256;                 // workgroups of ngp_mlp_bwd_kernel = slabs of the workspace (one per CU)
constexpr int kNgpLdsStride = 40;                     // halves per row of a staged [neuron][32 points] tile: 80 B, rows stay 16-byte aligned and spread over the banks
constexpr int kNgpStage = 64 * kNgpLdsStride;         // halves of one staged tile

// A fragment of a TRANSPOSED weight matrix whose B operand is an accumulator tile b (of dz), k-step s: row `col` of W^T, element j is
// W[32 b + 16 s + 8 (j >> 2) + 4 h + (j & 3)][col]  (the k order of ngp_load_a_perm)
__device__ __forceinline__ iris_h8 ngp_load_at_perm(const _Float16* W, int col, int b, int s, int h) {
    iris_h8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = W[(32 * b + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)) * kNgpWidth + col];
    return r;
}
// f32 -> f16 of 8 accumulator registers of a gradient tile, masked by the forward's pre-activations (> 0): the B fragment of the next data-gradient k-step
__device__ __forceinline__ iris_h8 ngp_pack_masked(const iris_f16v& d, const iris_f16v& pre, int s) {
    iris_h8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (_Float16)(pre[8 * s + j] > 0.f ? d[8 * s + j] : 0.f);
    return r;
}
// the lanes of a wave exchange a tile through LDS: LDS operations of one wave complete in order, the fence keeps the compiler from moving them
__device__ __forceinline__ void ngp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}
// 8 halves of an accumulator-layout fragment (element j = row base + (j & 3) + 8 (j >> 2) + 4 h) of point column r -> staged tile [row][point]
__device__ __forceinline__ void ngp_stage_frag(_Float16* tile, const iris_h8& v, int base, int r, int h) {
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[(base + (j & 3) + 8 * (j >> 2) + 4 * h) * kNgpLdsStride + r] = v[j];
}
// operand of a weight-gradient MFMA: row `row` of a staged tile, points 16 s + 8 h .. + 7 (the contraction runs over the points)
__device__ __forceinline__ iris_h8 ngp_stage_read(const _Float16* tile, int row, int s, int h) {
    return *reinterpret_cast<const iris_h8*>(tile + row * kNgpLdsStride + 16 * s + 8 * h);
}

__global__ __launch_bounds__(256) void ngp_mlp_bwd_kernel(NgpBwdArgs b) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[4 * 2 * kNgpStage];          // 40 KiB: two staged tiles per wave; the workgroup's slab sum (9216 f32) afterwards
    static_assert(sizeof(_Float16) * 4 * 2 * kNgpStage >= sizeof(float) * kNgpMlpParams, "the slab sum reuses the staging buffer");
    __shared__ iris_h8 tw[18][64];                                                     // 18 KiB
    const NgpArgs& a = b.f;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wid = threadIdx.x >> 6;
    _Float16* sz = lds + wid * 2 * kNgpStage;          // dz tile [neuron][point]
    _Float16* sh = sz + kNgpStage;                     // activation tile [neuron][point]
    const _Float16* W1 = a.w;
    const _Float16* W2 = a.w + kNgpWidth * 64;
    const _Float16* W3 = W2 + kNgpWidth * kNgpWidth;
    NgpWeights W;
    ngp_load_weights(a.w, r, h, W);
    // transposed weights as A fragments, in LDS (one 16-byte fragment per lane, shared by the 4 waves: 72 registers that the weight-gradient accumulators need):
    // fragment 0 .. 1 = W3^T (64 x 16, one k-step), 2 + 4 bo + 2 bi + s = W2^T, 10 + 4 bo + 2 bi + s = W1^T
    for (int f = wid; f < 18; f += 4) {
        const int g = f < 2 ? f : (f - 2) & 7, bo = f < 2 ? f : g >> 2, bi = (g >> 1) & 1, s = g & 1;
        tw[f][lane] = f < 2 ? ngp_load_at_perm(W3, 32 * bo + r, 0, 0, h)                       // k = output (j & 3) + 8 (j >> 2) + 4 h < 16
                            : ngp_load_at_perm(f < 10 ? W2 : W1, 32 * bo + r, bi, s, h);
    }
    __syncthreads();
    // weight-gradient accumulators, over the wave's whole tile loop: dw[row tile][column tile], row = dz neuron, column = input neuron
    iris_f16v dw1[2][2], dw2[2][2], dw3[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 16; ++q) dw3[i][q] = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) { dw1[i][j][q] = 0.f; dw2[i][j][q] = 0.f; }
    }

    const int n_tiles = (a.n + 31) >> 5;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (gridDim.x * 256) >> 6;
    for (int t = wave; t < n_tiles; t += n_waves) {
        const int pt = t * 32 + r;
        const bool pv = pt < a.n;
        iris_h8 xf[4];
        iris_f16v acc1[2], acc2[2], acc3;
        ngp_forward_tile(a, W, pt, pv, h, xf, acc1, acc2, acc3);           // (a point beyond the chunk has zero features: zero activations, zero gradients)

        // dz3 = g * s (1 - s) * loss_scale, s the forward's half-grid sigmoid; lanes h = 0: outputs 0 .. 3, lanes h = 1: output 4 (5 .. 7 padded: dz = 0)
        float gq[4] = {0.f, 0.f, 0.f, 0.f};
        if (pv) {
            const int64_t g = a.n0 + pt;
            if (h == 0) { gq[0] = b.g_albedo[g * 3]; gq[1] = b.g_albedo[g * 3 + 1]; gq[2] = b.g_albedo[g * 3 + 2]; gq[3] = b.g_rough[g] * 0.98f; }
            else gq[0] = b.g_metal[g];
        }
        iris_h8 z3;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float sg = ngp_out(acc3[q]);
            const float dz = gq[q] != 0.f ? gq[q] * (sg * (1.0f - sg)) * b.loss_scale : 0.f;
            z3[q] = (_Float16)dz; z3[4 + q] = (_Float16)0.f;               // elements 4 .. 7 are outputs 8 .. 15
        }

        // dW3 += dz3 H2^T  (rows 16 .. 31 of the tile do not exist: a zero A fragment)
        ngp_wave_sync();
        ngp_stage_frag(sz, z3, 0, r, h);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int s = 0; s < 2; ++s) ngp_stage_frag(sh, ngp_pack_relu(acc2[bi], s), 32 * bi + 16 * s, r, h);
        ngp_wave_sync();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            iris_h8 za = ngp_stage_read(sz, r & 15, s, h);
            if (r >= kNgpOutPad) za = iris_h8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) dw3[bi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(za, ngp_stage_read(sh, 32 * bi + r, s, h), dw3[bi], 0, 0, 0);
        }

        // dH2 = W3^T dz3, dz2 = dH2 where the forward's pre-activation is positive
        iris_f16v d2[2];
#pragma unroll
        for (int bo = 0; bo < 2; ++bo) {
#pragma unroll
            for (int q = 0; q < 16; ++q) d2[bo][q] = 0.f;
            d2[bo] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[bo][lane], z3, d2[bo], 0, 0, 0);
        }
        iris_h8 z2[2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int s = 0; s < 2; ++s) z2[bi][s] = ngp_pack_masked(d2[bi], acc2[bi], s);

        // dW2 += dz2 H1^T
        ngp_wave_sync();
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int s = 0; s < 2; ++s) { ngp_stage_frag(sz, z2[bi][s], 32 * bi + 16 * s, r, h); ngp_stage_frag(sh, ngp_pack_relu(acc1[bi], s), 32 * bi + 16 * s, r, h); }
        ngp_wave_sync();
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int bo = 0; bo < 2; ++bo) {
                const iris_h8 za = ngp_stage_read(sz, 32 * bo + r, s, h);
#pragma unroll
                for (int bi = 0; bi < 2; ++bi) dw2[bo][bi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(za, ngp_stage_read(sh, 32 * bi + r, s, h), dw2[bo][bi], 0, 0, 0);
            }

        // dH1 = W2^T dz2, dz1 masked by the first layer's pre-activations
        iris_f16v d1[2];
#pragma unroll
        for (int bo = 0; bo < 2; ++bo) {
#pragma unroll
            for (int q = 0; q < 16; ++q) d1[bo][q] = 0.f;
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int s = 0; s < 2; ++s) d1[bo] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[2 + 4 * bo + 2 * bi + s][lane], z2[bi][s], d1[bo], 0, 0, 0);
        }
        iris_h8 z1[2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int s = 0; s < 2; ++s) z1[bi][s] = ngp_pack_masked(d1[bi], acc1[bi], s);

        // dW1 += dz1 X^T  (X: the layer-1 B fragments hold features 16 s + 8 h + j of the lane's point)
        ngp_wave_sync();
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int s = 0; s < 2; ++s) ngp_stage_frag(sz, z1[bi][s], 32 * bi + 16 * s, r, h);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) sh[(16 * s + 8 * h + j) * kNgpLdsStride + r] = xf[s][j];
        ngp_wave_sync();
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int bo = 0; bo < 2; ++bo) {
                const iris_h8 za = ngp_stage_read(sz, 32 * bo + r, s, h);
#pragma unroll
                for (int bi = 0; bi < 2; ++bi) dw1[bo][bi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(za, ngp_stage_read(sh, 32 * bi + r, s, h), dw1[bo][bi], 0, 0, 0);
            }

        // dX = W1^T dz1 -> [level][point] planes: registers (q, q + 1), q even, are the two features of level (32 bo + (q & 3) + 8 (q >> 2) + 4 h) / 2
#pragma unroll
        for (int bo = 0; bo < 2; ++bo) {
            iris_f16v dx;
#pragma unroll
            for (int q = 0; q < 16; ++q) dx[q] = 0.f;
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int s = 0; s < 2; ++s) dx = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[10 + 4 * bo + 2 * bi + s][lane], z1[bi][s], dx, 0, 0, 0);
            if (pv) {
#pragma unroll
                for (int q = 0; q < 16; q += 2) {
                    const int level = (32 * bo + (q & 3) + 8 * (q >> 2) + 4 * h) >> 1;
                    b.dx[(size_t)level * b.n_plane + pt] = make_float2(dx[q], dx[q + 1]);
                }
            }
        }
    }

    // the workgroup's slab: its 4 waves summed in LDS in wave order (a fixed order: the slab is reproducible), then written out
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wid == w) {
#pragma unroll
            for (int bo = 0; bo < 2; ++bo)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
#pragma unroll
                    for (int bi = 0; bi < 2; ++bi) {
                        const int i1 = (32 * bo + row) * 64 + 32 * bi + r, i2 = kNgpWidth * 64 + i1;
                        red[i1] = (w ? red[i1] : 0.f) + dw1[bo][bi][q];
                        red[i2] = (w ? red[i2] : 0.f) + dw2[bo][bi][q];
                    }
                    if (q < 8) {                          // dw3[bo]: rows = outputs 0 .. 15 (registers 0 .. 7), columns 32 bo + r
                        const int i3 = 2 * kNgpWidth * 64 + row * 64 + 32 * bo + r;
                        red[i3] = (w ? red[i3] : 0.f) + dw3[bo][q];
                    }
                }
        }
        __syncthreads();
    }
    float* slab = b.slabs + (size_t)blockIdx.x * kNgpMlpParams;
    for (int i = threadIdx.x; i < kNgpMlpParams; i += 256) slab[i] = red[i];
}

// grad_params[i] += (slab 0 + slab 1 + ...)[i] / loss_scale, i < 9216: one thread per weight, slabs in order
__global__ __launch_bounds__(256) void ngp_wgrad_reduce_kernel(NgpBwdArgs b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kNgpMlpParams) return;
    float s = 0.f;
    for (int k = 0; k < b.n_slabs; ++k) s += b.slabs[(size_t)k * kNgpMlpParams + i];
    b.grad[i] += s * b.inv_scale;
}

// d loss / d table entry: the encode's 8 corners again, wgt * dX scattered with f32 atomic adds (there is no 8- or 16-byte f32 atomic to pair the two features
// or the two x-neighbours in; what adjacency buys is that their adds follow each other into the same 64-B line)
__global__ __launch_bounds__(256) void ngp_grid_bwd_kernel(NgpBwdArgs b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int level = blockIdx.y;
    if (i >= b.f.n) return;
    const float2 d = b.dx[(size_t)level * b.n_plane + i];
    if (d.x == 0.f && d.y == 0.f) return;                 // (a point without a cotangent adds exact zeros: skipped)
    const float gx = d.x * b.inv_scale, gy = d.y * b.inv_scale;
    NgpCell q;
    ngp_cell(b.f, level, i, q);
    float* table = b.grad + kNgpMlpParams + 2 * (size_t)b.f.lv.offset[level];
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        uint32_t ia, ib;
        ngp_corner_pair(q, c, ia, ib);
#pragma unroll
        for (int xx = 0; xx < 2; ++xx) {
            const float wgt = ngp_corner_weight(q, c, xx);
            float* e = table + 2 * (size_t)(xx ? ib : ia);
            unsafeAtomicAdd(e, wgt * gx);
            unsafeAtomicAdd(e + 1, wgt * gy);
        }
    }
}

// f32 master parameters -> the half weights and half2 tables the forward reads: round to nearest even, 8 parameters per thread (kNgpMlpParams % 8 == 0)
__global__ __launch_bounds__(256) void ngp_params_cast_kernel(const float4* __restrict__ params, int64_t n8, _Float16* __restrict__ w, _Float16* __restrict__ grid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const float4 lo = params[2 * i], hi = params[2 * i + 1];
    iris_h8 o;
    o[0] = (_Float16)lo.x; o[1] = (_Float16)lo.y; o[2] = (_Float16)lo.z; o[3] = (_Float16)lo.w;
    o[4] = (_Float16)hi.x; o[5] = (_Float16)hi.y; o[6] = (_Float16)hi.z; o[7] = (_Float16)hi.w;
    _Float16* dst = i * 8 < kNgpMlpParams ? w + i * 8 : grid + (i * 8 - kNgpMlpParams);
    *reinterpret_cast<iris_h8*>(dst) = o;
}

}  // namespace iris
