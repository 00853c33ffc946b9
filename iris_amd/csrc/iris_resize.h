// 8-bit image resize on the device: the scannetpp layout's --res_scale (photographs, albedo priors, segment ids), between the upload and pool_view / PixelSet.
// The contract is DESIGN.md 5c-15; tests/resize_ref.py restates it in numpy.
//
//   linear   OpenCV's cv2.resize(img, (Wt, Ht)) on uint8 (INTER_LINEAR, the 8-bit fixed-point C path of resize.cpp).  Per axis a table of source indices
//            and int16 weight pairs (resize_axis_table, HOST: float32 coordinate arithmetic, weights rounded half-even to 11 bits); horizontal pass in int32,
//            R = S[s] w0 + S[s+1] w1; vertical pass dst = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2.  R <= 255 * 2048 and b (R >> 4) <=
//            2048 * 32640 < 2^27: everything fits 32 bits.  When BOTH axes shrink by exactly 2 OpenCV takes its area path instead: (a + b + c + d + 2) >> 2.
//   nearest  PIL's Image.NEAREST (the reference's sample_nearest): dst[y][x] = S[yofs[y]][xofs[x]], the indices from the accumulated-addition scan.
//
// resize_kernel: an image's output is a block of Ht * Wt * C bytes with no padding between rows, so rows -- and, in a batch, blocks -- start at any
// alignment.  A lane owns one 4-byte-aligned dword of the block's byte range: it computes the four bytes (pixel and channel walked incrementally across row
// ends) and stores them as one dword; the first and last dword of a block, where the block covers them only in part, are written byte by byte and only
// inside the block, so a neighbouring image or tensor is never touched.  All-integer, no atomics, nothing order-dependent: bitwise reproducible.
#pragma once
#include <cmath>
#include <cstdint>

namespace iris {

constexpr int kResizeMaxImages = 16;  // images per launch (their pointers travel in the kernel arguments, as png_rows_kernel's)
constexpr int kResizeThreads = 256;
constexpr int kResizeMaxSide = 65535;
enum { kResizeLinear = 0, kResizeNearest = 1, kResizeHalf = 2 };          // kResizeHalf: the exact-2 path, chosen by iris_resize_u8 from the sizes

// One axis' table.  HOST arithmetic, compiled with -ffp-contract=off (the Makefile): a fused multiply-add on (d + 0.5) * scale - 0.5 changes f.
inline void resize_axis_table(int mode, int ns, int nd, int32_t* ofs, int16_t* coef) {
    if (mode == kResizeNearest) {
        const double a = (double)ns / (double)nd;
        double x = a * 0.5;
        for (int d = 0; d < nd; ++d) {
            const int s = (int)std::floor(x);
            ofs[d] = s < ns - 1 ? s : ns - 1;
            x += a;
        }
        return;
    }
    const double scale = 1.0 / ((double)nd / (double)ns);                 // OpenCV forms the inverse scale first: not ns / nd
    for (int d = 0; d < nd; ++d) {
        const double c = ((double)d + 0.5) * scale;
        float f = (float)(c - 0.5);
        int s = (int)std::floor(f);
        f = f - (float)s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= ns - 1) { s = ns - 1; f = 0.f; }
        const float g = 1.f - f;
        ofs[d] = s;
        coef[2 * d] = (int16_t)std::nearbyintf(g * 2048.f);               // round half to even (the default rounding mode)
        coef[2 * d + 1] = (int16_t)std::nearbyintf(f * 2048.f);
    }
}

struct ResizeArgs {
    const uint8_t* img[kResizeMaxImages];   // (Hs, Ws, C) uint8
    const int32_t *xofs, *yofs;             // (Wt), (Ht); unused by kResizeHalf
    const int16_t *xcoef, *ycoef;           // (Wt, 2), (Ht, 2); kResizeLinear only
    int Hs, Ws, Ht, Wt;
    int64_t block_bytes;                    // Ht * Wt * C
    uint8_t* out;                           // where image 0 of THIS launch starts: (M, block_bytes)
};

template <int C, int MODE>
__device__ __forceinline__ uint32_t resize_value(const ResizeArgs& a, const uint8_t* src, int y, int x, int c) {
    const int64_t row = (int64_t)a.Ws * C;
    if (MODE == kResizeHalf) {
        const uint8_t* p = src + (int64_t)(2 * y) * row + (int64_t)(2 * x) * C + c;
        return ((uint32_t)p[0] + p[C] + p[row] + p[row + C] + 2u) >> 2;
    }
    const int x0 = min(max(a.xofs[x], 0), a.Ws - 1), y0 = min(max(a.yofs[y], 0), a.Hs - 1);          // (the clamps cost nothing and keep a bad table in bounds)
    if (MODE == kResizeNearest) return src[(int64_t)y0 * row + (int64_t)x0 * C + c];
    const int x1 = min(x0 + 1, a.Ws - 1), y1 = min(y0 + 1, a.Hs - 1);
    const int w0 = a.xcoef[2 * x], w1 = a.xcoef[2 * x + 1], b0 = a.ycoef[2 * y], b1 = a.ycoef[2 * y + 1];
    const uint8_t *r0 = src + (int64_t)y0 * row + c, *r1 = src + (int64_t)y1 * row + c;
    const int R0 = (int)r0[(int64_t)x0 * C] * w0 + (int)r0[(int64_t)x1 * C] * w1;
    const int R1 = (int)r1[(int64_t)x0 * C] * w0 + (int)r1[(int64_t)x1 * C] * w1;
    return (uint32_t)((((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2) & 0xFFu;
}

// grid (the dwords that overlap the image's block, grid-stride; image)
template <int C, int MODE>
__global__ __launch_bounds__(kResizeThreads) void resize_kernel(ResizeArgs a) {
    const uint8_t* src = a.img[blockIdx.y];
    uint8_t* dst = a.out + (int64_t)blockIdx.y * a.block_bytes;                    // this image's block: any alignment
    const int64_t head = (int64_t)(reinterpret_cast<uintptr_t>(dst) & 3u);        // bytes of the first dword that lie in front of the block
    const int64_t n_dwords = (head + a.block_bytes + 3) >> 2;
    const int64_t row_bytes = (int64_t)a.Wt * C;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n_dwords; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t first = max(4 * j - head, (int64_t)0), last = min(4 * j - head + 4, a.block_bytes);   // this lane's bytes of the block: [first, last)
        int y = (int)(first / row_bytes);
        const int q = (int)(first - (int64_t)y * row_bytes);
        int x = q / C, c = q - x * C;
        const int n = (int)(last - first);
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                v[k] = resize_value<C, MODE>(a, src, y, x, c);
                if (++c == C) {
                    c = 0;
                    if (++x == a.Wt) { x = 0; ++y; }
                }
            }
        }
        if (n == 4) {                                                              // (first + head = 4 j: the address is 4-byte aligned)
            *reinterpret_cast<uint32_t*>(dst + first) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) dst[first + k] = (uint8_t)v[k];
        }
    }
}

}  // namespace iris
