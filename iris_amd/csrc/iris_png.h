// 8-bit PNG files on the device (render_video.py's eight files per frame): float maps -> PNG scanline bytes -> one zlib stream per image.
//
//   png_rows_kernel   one launch per group of equal-size images: per value v = x / d (IEEE division), NaN -> 0, clamp to [0,1], q = (uint8) trunc(v * 255) --
//                     the reference's (np.clip(image, 0, 1) * 255).astype(np.uint8) --, for a `magma` image q -> the 256 x 3 MAGMA table (cv2.applyColorMap
//                     + BGR2RGB), the crop to even height and width, and every row written as [1][Sub-filtered bytes] (PNG filter type 1, bpp = output
//                     channels): straight into the byte layout the deflate stage reads.  uint8 input takes the same path without the quantiser.
//   zip_segment_kernel (iris_deflate.h, unchanged): each image is ONE chunk, cut into kZipSeg-byte segments, one deflate block each.
//   png_chunk_kernel  one workgroup per image: block scans over its segments -> where each segment starts in the stream, the stream's size, its Adler-32
//   zip_offsets_kernel (iris_deflate.h, record_header = 0): where each image's stream starts
//   png_emit_kernel   one workgroup per SEGMENT copies it to its place (a 1080p image is ~380 segments: the copy is spread over that many workgroups);
//                     the first writes the zlib header, the last the Adler-32
// The stream is always the zlib stream: OpenEXR's "raw block when not shorter" rule, the un-predicting scan and the 8-byte record header do not apply.
// A segment is at most a stored block, kZipSeg + 5 bytes, so a stream is at most raw + 5 per segment + 6 (png_stream_bound).
#pragma once
#include "iris_deflate.h"

namespace iris {

constexpr int kPngMaxImages = 16;     // images per launch of png_rows_kernel (their pointers travel in the kernel arguments)
constexpr int kPngThreads = 256;

// OpenCV's COLORMAP_MAGMA as R,G,B: matplotlib's _magma_data (256 x 3, six decimals) * 255 rounded to nearest; no entry is within 5e-4 of a tie.
#define IRIS_PNG_MAGMA_RGB                                                                                                                                          \
    0, 0, 4, 1, 0, 5, 1, 1, 6, 1, 1, 8, 2, 1, 9, 2, 2, 11, 2, 2, 13, 3, 3, 15, 3, 3, 18, 4, 4, 20, 5, 4, 22, 6, 5, 24, 6, 5, 26, 7, 6, 28, 8, 7, 30, 9, 7, 32,     \
    10, 8, 34, 11, 9, 36, 12, 9, 38, 13, 10, 41, 14, 11, 43, 16, 11, 45, 17, 12, 47, 18, 13, 49, 19, 13, 52, 20, 14, 54, 21, 14, 56, 22, 15, 59, 24, 15, 61, 25, 16, 63, 26, 16, 66, 28, 16, 68, \
    29, 17, 71, 30, 17, 73, 32, 17, 75, 33, 17, 78, 34, 17, 80, 36, 18, 83, 37, 18, 85, 39, 18, 88, 41, 17, 90, 42, 17, 92, 44, 17, 95, 45, 17, 97, 47, 17, 99, 49, 17, 101, 51, 16, 103, 52, 16, 105, \
    54, 16, 107, 56, 16, 108, 57, 15, 110, 59, 15, 112, 61, 15, 113, 63, 15, 114, 64, 15, 116, 66, 15, 117, 68, 15, 118, 69, 16, 119, 71, 16, 120, 73, 16, 120, 74, 16, 121, 76, 17, 122, 78, 17, 123, 79, 18, 123, \
    81, 18, 124, 82, 19, 124, 84, 19, 125, 86, 20, 125, 87, 21, 126, 89, 21, 126, 90, 22, 126, 92, 22, 127, 93, 23, 127, 95, 24, 127, 96, 24, 128, 98, 25, 128, 100, 26, 128, 101, 26, 128, 103, 27, 128, 104, 28, 129, \
    106, 28, 129, 107, 29, 129, 109, 29, 129, 110, 30, 129, 112, 31, 129, 114, 31, 129, 115, 32, 129, 117, 33, 129, 118, 33, 129, 120, 34, 129, 121, 34, 130, 123, 35, 130, 124, 35, 130, 126, 36, 130, 128, 37, 130, 129, 37, 129, \
    131, 38, 129, 132, 38, 129, 134, 39, 129, 136, 39, 129, 137, 40, 129, 139, 41, 129, 140, 41, 129, 142, 42, 129, 144, 42, 129, 145, 43, 129, 147, 43, 128, 148, 44, 128, 150, 44, 128, 152, 45, 128, 153, 45, 128, 155, 46, 127, \
    156, 46, 127, 158, 47, 127, 160, 47, 127, 161, 48, 126, 163, 48, 126, 165, 49, 126, 166, 49, 125, 168, 50, 125, 170, 51, 125, 171, 51, 124, 173, 52, 124, 174, 52, 123, 176, 53, 123, 178, 53, 123, 179, 54, 122, 181, 54, 122, \
    183, 55, 121, 184, 55, 121, 186, 56, 120, 188, 57, 120, 189, 57, 119, 191, 58, 119, 192, 58, 118, 194, 59, 117, 196, 60, 117, 197, 60, 116, 199, 61, 115, 200, 62, 115, 202, 62, 114, 204, 63, 113, 205, 64, 113, 207, 64, 112, \
    208, 65, 111, 210, 66, 111, 211, 67, 110, 213, 68, 109, 214, 69, 108, 216, 69, 108, 217, 70, 107, 219, 71, 106, 220, 72, 105, 222, 73, 104, 223, 74, 104, 224, 76, 103, 226, 77, 102, 227, 78, 101, 228, 79, 100, 229, 80, 100, \
    231, 82, 99, 232, 83, 98, 233, 84, 98, 234, 86, 97, 235, 87, 96, 236, 88, 96, 237, 90, 95, 238, 91, 94, 239, 93, 94, 240, 95, 94, 241, 96, 93, 242, 98, 93, 242, 100, 92, 243, 101, 92, 244, 103, 92, 244, 105, 92, \
    245, 107, 92, 246, 108, 92, 246, 110, 92, 247, 112, 92, 247, 114, 92, 248, 116, 92, 248, 118, 92, 249, 120, 93, 249, 121, 93, 249, 123, 93, 250, 125, 94, 250, 127, 94, 250, 129, 95, 251, 131, 95, 251, 133, 96, 251, 135, 97, \
    252, 137, 97, 252, 138, 98, 252, 140, 99, 252, 142, 100, 252, 144, 101, 253, 146, 102, 253, 148, 103, 253, 150, 104, 253, 152, 105, 253, 154, 106, 253, 155, 107, 254, 157, 108, 254, 159, 109, 254, 161, 110, 254, 163, 111, 254, 165, 113, \
    254, 167, 114, 254, 169, 115, 254, 170, 116, 254, 172, 118, 254, 174, 119, 254, 176, 120, 254, 178, 122, 254, 180, 123, 254, 182, 124, 254, 183, 126, 254, 185, 127, 254, 187, 129, 254, 189, 130, 254, 191, 132, 254, 193, 133, 254, 194, 135, \
    254, 196, 136, 254, 198, 138, 254, 200, 140, 254, 202, 141, 254, 204, 143, 254, 205, 144, 254, 207, 146, 254, 209, 148, 254, 211, 149, 254, 213, 151, 254, 215, 153, 254, 216, 154, 253, 218, 156, 253, 220, 158, 253, 222, 160, 253, 224, 161, \
    253, 226, 163, 253, 227, 165, 253, 229, 167, 253, 231, 169, 253, 233, 170, 253, 235, 172, 252, 236, 174, 252, 238, 176, 252, 240, 178, 252, 242, 180, 252, 244, 182, 252, 246, 184, 252, 247, 185, 252, 249, 187, 252, 251, 189, 252, 253, 191
__constant__ uint8_t kPngMagma[768] = {IRIS_PNG_MAGMA_RGB};
static const uint8_t kPngMagmaHost[768] = {IRIS_PNG_MAGMA_RGB};     // the same bytes for iris_png_magma_table (the host arm and the tests read them)

struct PngRowsArgs {
    const void* img[kPngMaxImages];   // (H, W, C) float32 or uint8
    float div[kPngMaxImages];
    uint32_t magma;                   // bit m: image m goes through the colour map (C == 1)
    int M, H, W, H2, W2, cout;        // H2, W2: the even crop; cout: channels written (3 for a magma image)
    int64_t block_bytes;              // H2 * (1 + W2 * cout)
    uint8_t* rows;                    // (M, block_bytes)
};

__device__ __forceinline__ uint32_t png_quantize(float x, float d) {
    float v = x / d;                                      // IEEE division (-fno-fast-math): emission's / 10.0 as numpy divides
    v = v != v ? 0.f : v;
    v = fminf(fmaxf(v, 0.f), 1.f);
    return (uint32_t)(v * 255.0f);                        // truncation; v * 255 <= 255 exactly
}

template <int C, bool U8>
__device__ __forceinline__ void png_pixel(const void* src, int64_t i, float d, bool magma, uint32_t* q) {
    uint32_t v[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = U8 ? (uint32_t)static_cast<const uint8_t*>(src)[i * C + c] : png_quantize(static_cast<const float*>(src)[i * C + c], d);
    if (C == 1 && magma) {
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = kPngMagma[3 * v[0] + c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = v[c];
    }
}

// grid (pixels of the cropped image, grid-stride; image): one thread per output pixel writes its cout Sub-filtered bytes (its own value minus its left
// neighbour's, recomputed), the thread of column 0 also the row's filter-type byte
template <int C, bool U8>
__global__ __launch_bounds__(kPngThreads) void png_rows_kernel(PngRowsArgs a) {
    const int m = blockIdx.y;
    const void* src = a.img[m];
    const float d = a.div[m];
    const bool magma = (a.magma >> m) & 1u;
    const int cout = a.cout;
    const int64_t row_bytes = 1 + (int64_t)a.W2 * cout, n = (int64_t)a.H2 * a.W2;
    uint8_t* dst = a.rows + (int64_t)m * a.block_bytes;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = p / a.W2;
        const int x = (int)(p - y * a.W2);
        uint32_t q[3] = {0, 0, 0}, l[3] = {0, 0, 0};
        png_pixel<C, U8>(src, y * a.W + x, d, magma, q);
        if (x > 0) png_pixel<C, U8>(src, y * a.W + x - 1, d, magma, l);
        uint8_t* r = dst + y * row_bytes;
        if (x == 0) r[0] = 1;                             // filter type 1: Sub
        r += 1 + (int64_t)x * cout;
        for (int c = 0; c < cout; ++c) r[c] = (uint8_t)(q[c] - l[c]);
    }
}

__host__ __device__ inline int64_t png_stream_bound(int64_t block_bytes) {       // zlib header 2, per segment at most a stored block (5 + data), Adler-32 4
    return block_bytes + 5 * ((block_bytes + kZipSeg - 1) / kZipSeg) + 6;
}

// One workgroup per image (a chunk of a.sf segments, n_full = 1, no tail): seg_off, chunk_len, chunk_adler.  The Adler-32 of a concatenation:
// A = 1 + sum a_k, B = sum (len_k * A_before_k + b_k), all mod 65521 -- zip_chunk_kernel's recurrence as two prefix sums.
__global__ __launch_bounds__(kZipThreads) void png_chunk_kernel(ZipArgs a) {
    __shared__ uint32_t scan[kZipThreads];
    __shared__ uint32_t tot[3];
    const int t = threadIdx.x;
    const int64_t ci = blockIdx.x, base = ci * a.sf;
    uint32_t off = 2, A = 1, Bs = 0;
    for (int k0 = 0; k0 < a.sf; k0 += kZipThreads) {
        const int k = k0 + t;
        const bool in = k < a.sf;
        const uint32_t len = in ? a.seg_len[base + k] : 0u, sa = in ? a.seg_adler[2 * (base + k)] : 0u, sb = in ? a.seg_adler[2 * (base + k) + 1] : 0u;
        const uint32_t ls = in ? (uint32_t)min<int64_t>(kZipSeg, a.B - (int64_t)k * kZipSeg) : 0u;
        const uint32_t incl_len = zip_scan_add(len, scan);
        const uint32_t incl_a = zip_scan_add(sa, scan);                        // 256 values below 65521: no overflow
        const uint32_t a_before = (A + incl_a - sa) % kAdlerMod;
        const uint32_t term = in ? (uint32_t)(((uint64_t)ls * a_before + sb) % kAdlerMod) : 0u;
        const uint32_t incl_b = zip_scan_add(term, scan);
        if (in) a.seg_off[base + k] = off + incl_len - len;
        if (t == kZipThreads - 1) { tot[0] = incl_len; tot[1] = incl_a; tot[2] = incl_b; }
        __syncthreads();
        off += tot[0]; A = (A + tot[1]) % kAdlerMod; Bs = (Bs + tot[2]) % kAdlerMod;
        __syncthreads();
    }
    if (t == 0) { a.chunk_len[ci] = off + 4; a.chunk_adler[ci] = (Bs << 16) | A; }
}

// One workgroup per segment: its bytes at chunk_off + seg_off.
__global__ __launch_bounds__(kZipThreads) void png_emit_kernel(ZipArgs a) {
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x, ci = g / a.sf;
    const int s = (int)(g - ci * a.sf);
    uint8_t* dst = a.records + a.chunk_off[ci];
    if (s == 0 && t < 2) dst[t] = t == 0 ? 0x78 : 0x01;                        // 32 K window, no dictionary, check bits
    if (s == a.sf - 1 && t < 4) dst[a.chunk_len[ci] - 4 + t] = (uint8_t)(a.chunk_adler[ci] >> (24 - 8 * t));
    const uint32_t ls = a.seg_len[g];
    const uint8_t* sp = a.seg_data + g * kZipSegCap;
    uint8_t* dp = dst + a.seg_off[g];
    for (uint32_t i = t; i < ls; i += kZipThreads) dp[i] = sp[i];
}

}  // namespace iris
