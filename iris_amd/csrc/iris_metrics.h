// Image-quality metrics on the device: SSIM and the squared error behind PSNR of two image stacks a, b (N, H, W, C) float32, C in {1, 3}, H, W >= 7
// (reference: render.py:236-239 -- skimage.metrics.peak_signal_noise_ratio / structural_similarity(data_range = R, channel_axis = -1)).
//
// skimage is not a dependency of this project; the contract is its defaults, restated.  Uniform 7 x 7 window, K1 = 0.01, K2 = 0.03, sample covariance:
//     cov_norm = 49 / 48,  C1 = (K1 R)^2,  C2 = (K2 R)^2
//     per channel and per window that lies fully inside the image (skimage crops a border of 3 before its mean: the filter's boundary mode never enters):
//     ux, uy window means;  vx, vy, vxy window (co)variances times cov_norm
//     S = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2))
//     mssim = mean over the channels of the mean of S over the (H - 6)(W - 6) windows
// skimage takes the variance as E[x^2] - E[x]^2 in the input's precision: on a bright, nearly flat float32 pair (a lit wall) the cancellation costs 2e-4 of S.
// Here the moments are taken of the window shifted by ITS OWN centre pixel (the rule iris_denoise.h states for its variance).  Operation order, every
// operation one correctly rounded float32 operation (the build has -ffp-contract=off), taps in the order row -3..3 outer, column -3..3 inner:
//     dx = x - x_c;  dy = y - y_c;  sx += dx;  sy += dy;  sxx += dx * dx;  syy += dy * dy;  sxy += dx * dy            (49 taps, the centre included)
//     mx = sx / 49;  my = sy / 49;  ux = x_c + mx;  uy = y_c + my
//     vx = cov_norm * (sxx / 49 - mx * mx);  vy = cov_norm * (syy / 49 - my * my);  vxy = cov_norm * (sxy / 49 - mx * my)
//     S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))                          (products left to right)
//     k1r = 0.01f * R;  C1 = k1r * k1r;  k2r = 0.03f * R;  C2 = k2r * k2r;  cov_norm = 49.f / 48.f                       (float32, on the host)
// A non-finite pixel makes every window that holds it NaN, and with them the image's sums (as in skimage).
//
//   tile kernel  one workgroup of 256 threads per tile of 64 x 16 pixels of one image.  An image row is W C contiguous floats, so everything is indexed by
//                ELEMENT e = x C + c along the row: the tile with its 3-pixel apron, 22 rows of 70 C floats of a and of b, is read with float4 loads at
//                16-byte-aligned addresses (whatever the row's alignment; the ragged ends of a row scalar) and stored to LDS unshifted (36 KB at C = 3:
//                four workgroups per CU).  A wave's 64 threads then own 64 consecutive elements of one tile row and read tap (i, j) at word
//                (row + i) * 70 C + e + j C: neighbouring lanes on neighbouring words, no bank conflict, every offset an immediate.  Slots outside the image
//                are neither written nor read: only windows fully inside the image are evaluated.
//   sums         per image and channel two doubles: sse = sum of ((double)a - (double)b)^2 over the pixels (each counted by the tile that OWNS it, not by
//                the aprons) and ssum = sum of (double)S over the windows (counted by the tile that owns the window's centre).  Every thread accumulates in
//                double over its elements in ascending order, the workgroup adds its threads in a fixed binary tree (stride 128, 64, ..., 1) and stores its
//                partial with plain stores into slab [image][tile][channel][2] of the workspace.
//   slab kernel  one workgroup per image: thread t adds slabs t, t + 256, ... in ascending order, the same tree adds the threads.  No atomics anywhere:
//                the sums are the same bits on every call for a given shape, with or without the optional map of S.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iris {

constexpr int kMetTileX = 64, kMetTileY = 16;      // pixels of a tile; 64 C elements per tile row = whole waves
constexpr int kMetThreads = 256;
constexpr int kMetApron = 3;                        // the 7 x 7 window

struct MetArgs {
    const float* a; const float* b;
    double* slabs;             // (N, tiles, C, 2)
    float* map;                // (N, H - 6, W - 6, C) or NULL
    int H, W, tiles_x, tiles_y;
    float c1, c2;
};

// red: (Q, kMetThreads) doubles in LDS, filled by every thread and synchronised; afterwards red[q * kMetThreads] holds the sum of row q
template <int Q>
__device__ __forceinline__ void met_tree(double* red) {
    const int t = threadIdx.x;
    for (int o = kMetThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int q = 0; q < Q; ++q) red[q * kMetThreads + t] += red[q * kMetThreads + t + o];
        }
        __syncthreads();
    }
}

template <int C>
__global__ __launch_bounds__(kMetThreads) void metrics_tile_kernel(MetArgs g) {
    constexpr int TE = kMetTileX * C;                               // elements of a tile row that this tile owns
    constexpr int LS = (kMetTileX + 2 * kMetApron) * C;             // LDS row stride = elements of a tile row with its apron
    constexpr int ROWS = kMetTileY + 2 * kMetApron;
    constexpr int NV = LS / 4 + 2;                                  // float4 slots that cover a row at any alignment: ceil((3 + LS) / 4)
    constexpr int Q = 2 * C;
    static_assert((3 + LS + 3) / 4 <= NV, "vector slots per row");
    static_assert(TE % 64 == 0, "a wave owns elements of one tile row");
    static_assert(2 * ROWS * LS * sizeof(float) >= (size_t)Q * kMetThreads * sizeof(double), "the reduction reuses the tile's LDS");
    __shared__ __align__(16) float lds[2 * ROWS * LS];
    float* const la = lds;
    float* const lb = lds + ROWS * LS;

    const int tid = threadIdx.x;
    const int tiles = g.tiles_x * g.tiles_y;
    const int n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int x0 = (tile % g.tiles_x) * kMetTileX, y0 = (tile / g.tiles_x) * kMetTileY;
    const int H = g.H, W = g.W;

    // ---- the tile and its apron -> LDS.  Row elements [es, ee) are wanted; LDS slot of row element q: q - (x0 - 3) C
    const int e_first = (x0 - kMetApron) * C;
    const int es = max(e_first, 0), ee = min(e_first + LS, W * C), len = ee - es;
    for (int u = tid; u < ROWS * NV; u += kMetThreads) {
        const int r = u / NV, k = u % NV;
        const int y = y0 - kMetApron + r;
        if (y < 0 || y >= H) continue;
        const int64_t first = (((int64_t)n * H + y) * W) * C + es;           // the row's first wanted float
#pragma unroll
        for (int img = 0; img < 2; ++img) {
            const float* p = (img ? g.b : g.a) + first;
            float* dst = (img ? lb : la) + r * LS + (es - e_first);
            const int j0 = 4 * k - (int)(((uintptr_t)p >> 2) & 3);              // p + j0 is 16-byte aligned
            if (j0 >= 0 && j0 + 4 <= len) {
                const float4 v = *reinterpret_cast<const float4*>(p + j0);
                dst[j0] = v.x; dst[j0 + 1] = v.y; dst[j0 + 2] = v.z; dst[j0 + 3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j0 + i >= 0 && j0 + i < len) dst[j0 + i] = p[j0 + i];
            }
        }
    }
    __syncthreads();

    // ---- every thread: its elements of the tile, in ascending order
    const float cov_norm = 49.f / 48.f;
    double acc[Q];                                   // [c * 2]: sse, [c * 2 + 1]: ssum
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
#pragma unroll 1
    for (int i = tid; i < kMetTileY * TE; i += kMetThreads) {
        const int ry = i / TE, e = i % TE;
        const int px = e / C, c = e - px * C;
        const int x = x0 + px, y = y0 + ry;
        if (x >= W || y >= H) continue;
        const float* pa = la + ry * LS + e;          // tap (i, j) of this element's window: pa[i * LS + j * C]
        const float* pb = lb + ry * LS + e;
        const float xc = pa[kMetApron * LS + kMetApron * C], yc = pb[kMetApron * LS + kMetApron * C];
        const double d = (double)xc - (double)yc;
        const double dd = d * d;
        const bool inside = x >= kMetApron && x < W - kMetApron && y >= kMetApron && y < H - kMetApron;
        float S = 0.f;
        if (inside) {
            float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
            for (int ti = 0; ti < 7; ++ti) {
#pragma unroll
                for (int tj = 0; tj < 7; ++tj) {
                    const float dx = pa[ti * LS + tj * C] - xc, dy = pb[ti * LS + tj * C] - yc;
                    sx += dx; sy += dy; sxx += dx * dx; syy += dy * dy; sxy += dx * dy;
                }
            }
            const float mx = sx / 49.f, my = sy / 49.f;
            const float ux = xc + mx, uy = yc + my;
            const float vx = cov_norm * (sxx / 49.f - mx * mx);
            const float vy = cov_norm * (syy / 49.f - my * my);
            const float vxy = cov_norm * (sxy / 49.f - mx * my);
            S = ((2.f * ux * uy + g.c1) * (2.f * vxy + g.c2)) / ((ux * ux + uy * uy + g.c1) * (vx + vy + g.c2));
            if (g.map) g.map[((((int64_t)n * (H - 6) + (y - kMetApron)) * (W - 6)) + (x - kMetApron)) * C + c] = S;
        }
#pragma unroll
        for (int cc = 0; cc < C; ++cc) {
            if (c == cc) {
                acc[cc * 2] += dd;
                if (inside) acc[cc * 2 + 1] += (double)S;
            }
        }
    }

    // ---- workgroup sum, fixed tree; the tile's LDS is free now
    __syncthreads();
    double* red = reinterpret_cast<double*>(lds);
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q * kMetThreads + tid] = acc[q];
    __syncthreads();
    met_tree<Q>(red);
    if (tid < Q) g.slabs[(int64_t)blockIdx.x * Q + tid] = red[tid * kMetThreads];
}

// sums (N, C, 2) from slabs (N, tiles, C, 2)
template <int C>
__global__ __launch_bounds__(kMetThreads) void metrics_slab_sum_kernel(const double* __restrict__ slabs, int tiles, double* __restrict__ sums) {
    constexpr int Q = 2 * C;
    __shared__ double red[Q * kMetThreads];
    const int tid = threadIdx.x;
    const double* mine = slabs + (int64_t)blockIdx.x * tiles * Q;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int t = tid; t < tiles; t += kMetThreads) {
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] += mine[(int64_t)t * Q + q];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q * kMetThreads + tid] = acc[q];
    __syncthreads();
    met_tree<Q>(red);
    if (tid < Q) sums[(int64_t)blockIdx.x * Q + tid] = red[tid * kMetThreads];
}

}  // namespace iris
