// Baseline JPEG frames on the device (render_video.py --video mjpeg: the frames of the Motion-JPEG .avi files): float or uint8 maps -> the entropy-coded
// data of one JPEG file per image, back to back in one dense buffer.  The frame contract is DESIGN.md 5c-14 (tests/jpeg_ref.py states it in numpy): 8 bit,
// Y Cb Cr at 2x2 1x1 1x1, MCU 16 x 16 = six blocks Y00 Y01 Y10 Y11 Cb Cr, the Annex K tables, ONE restart interval per MCU row.  The headers depend on
// (width, height, quality) only and are the host's (utils/jpeg.py).
//
//   jpeg_transform_kernel  one WAVE per block of 64 coefficients, lane = (row, column): the PNG path's pixel (png_pixel: quantiser, MAGMA table; the even
//                          crop; the last column / row repeated up to the MCU grid) -> Y, or the 2 x 2 mean of Cb or Cr -> minus 128 -> rows then columns of
//                          the integer DCT through LDS -> quantised -> int16 at its zigzag position.  One launch per group of kPngMaxImages images.
//   jpeg_entropy_kernel    one LANE per block: the Huffman symbols of its 64 coefficients as a bit string in the block's workspace slot, and its length.
//                          The DC difference reads the DC of the previous block of the component inside the interval -- it is there since the transform:
//                          no scan.  A slot holds kJpegBlockBits bits, the longest string the tables can produce (below).
//   jpeg_assemble_kernel   one workgroup per restart interval: prefix sum of its blocks' lengths; then every 32-bit word of the interval is GATHERED from the
//                          slots that overlap it (binary search for the first one; no atomics, no cleared buffer), the last byte padded with 1-bits; FF bytes
//                          counted -> the interval's size with stuffing and its RSTm marker.  A 1080p interval is 720 blocks, up to 146 KiB before stuffing:
//                          more than LDS holds, so it is assembled in the global workspace.
//   zip_offsets_kernel     (iris_deflate.h, unchanged: an interval is a "chunk", an image a "map") where every interval and every image starts
//   jpeg_emit_kernel       one workgroup per interval: FF count per 16-byte span, block scan -> every byte at its stuffed position (FF -> FF 00), then RSTm
//                          (m = MCU row mod 8) except after the image's last interval.
// Arithmetic is integer throughout: no contraction or reassociation can change a byte, any order of an integer sum is the same sum.
//
// Worst case.  A block's string is longest when no coefficient is zero (a zero run replaces symbols by fewer bits: ZRL is 11 bits for 16 coefficients, EOB at
// most 4): the DC code plus its magnitude bits and 63 times the longest AC code plus its magnitude bits -- kJpegBlockBits, computed from the tables below
// (22 + 63 * 26 = 1660).  Magnitudes: the DC is sum / 8 of 64 samples in [-128, 127], so a difference has at most 11 bits; an AC coefficient is at most
// (1/4) * 128 * (sum_n |cos((2n + 1) k pi / 16)|)^2 <= 1024 * (1 - 1/256) at k = 4 and less elsewhere, 10 bits, and the fixed-point error is below 1.
// An interval is its blocks' bits rounded up to a byte, every byte possibly stuffed, plus a marker: jpeg_interval_bound.
#pragma once
#include "iris_png.h"

namespace iris {

constexpr int kJpegThreads = 256;

// ITU-T T.81 Annex K: K.1 and K.2 (natural order), K.3 - K.6 as (BITS, HUFFVAL)
#define IRIS_JPEG_QUANT_LUMA 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, \
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99
#define IRIS_JPEG_QUANT_CHROMA 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99
struct JpegSpec { uint8_t bits[16]; uint8_t vals[162]; int n; };
constexpr JpegSpec kJpegDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr JpegSpec kJpegDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr JpegSpec kJpegAcLuma = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
     0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
     0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
     0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}, 162};
constexpr JpegSpec kJpegAcChroma = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
     0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
     0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}, 162};

// symbol -> (code, length), Annex C: the codes of a length are consecutive; the first of a length is twice the one after the last of the length before
struct JpegHuff { uint16_t code[256]; uint8_t len[256]; };
constexpr JpegHuff jpeg_make_huff(const JpegSpec& s) {
    JpegHuff h{};
    int code = 0, i = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int k = 0; k < s.bits[length - 1]; ++k, ++i, ++code) { h.code[s.vals[i]] = (uint16_t)code; h.len[s.vals[i]] = (uint8_t)length; }
        code <<= 1;
    }
    return h;
}
constexpr int jpeg_longest(const JpegSpec& s) {          // the longest code plus the magnitude bits of its symbol (the low nibble)
    const JpegHuff h = jpeg_make_huff(s);
    int best = 0;
    for (int i = 0; i < s.n; ++i) { const int b = h.len[s.vals[i]] + (s.vals[i] & 15); best = b > best ? b : best; }
    return best;
}
constexpr int jpeg_max(int a, int b) { return a > b ? a : b; }
constexpr int kJpegBlockBits = jpeg_max(jpeg_longest(kJpegDcLuma), jpeg_longest(kJpegDcChroma)) + 63 * jpeg_max(jpeg_longest(kJpegAcLuma), jpeg_longest(kJpegAcChroma));
constexpr int kJpegSlotWords = (kJpegBlockBits + 31) / 32;
static_assert(kJpegBlockBits == 22 + 63 * 26 && kJpegSlotWords == 52, "Annex K: DC 11 + 11 bits, AC 16 + 10 bits");

// the 8-point transform: M[k][n] = +-C[j], C[j] = round(32768 cos(j pi / 16)); row 0 is C[4] (the 1/sqrt 2 of the DC term)
struct JpegDct { int16_t m[64]; };
constexpr JpegDct jpeg_make_dct() {
    const int C[9] = {0, 32138, 30274, 27246, 23170, 18205, 12540, 6393, 0};
    JpegDct d{};
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) {
            int a = (2 * n + 1) * k % 32, sign = 1;
            if (a > 16) a = 32 - a;
            if (a > 8) { a = 16 - a; sign = -1; }
            d.m[k * 8 + n] = (int16_t)(k == 0 ? C[4] : sign * C[a]);
        }
    return d;
}
// natural (row-major) index -> position in zigzag order
struct JpegZig { uint8_t pos[64]; uint8_t nat[64]; };
constexpr JpegZig jpeg_make_zigzag() {
    JpegZig z{};
    int k = 0;
    for (int s = 0; s < 15; ++s)
        for (int i = 0; i < 8; ++i) {
            const int r = s % 2 ? i : s - i, c = s - r;          // odd diagonals run down-left (rows ascending), even ones up-right
            if (r < 0 || r > 7 || c < 0 || c > 7) continue;
            z.pos[r * 8 + c] = (uint8_t)k; z.nat[k] = (uint8_t)(r * 8 + c); ++k;
        }
    return z;
}

constexpr JpegZig kJpegZigHost = jpeg_make_zigzag();
static const uint8_t kJpegQuantHost[2][64] = {{IRIS_JPEG_QUANT_LUMA}, {IRIS_JPEG_QUANT_CHROMA}};
__constant__ uint8_t kJpegQuant[2][64] = {{IRIS_JPEG_QUANT_LUMA}, {IRIS_JPEG_QUANT_CHROMA}};
__constant__ JpegZig kJpegZig = jpeg_make_zigzag();
__constant__ JpegDct kJpegDct = jpeg_make_dct();
__constant__ JpegHuff kJpegDc[2] = {jpeg_make_huff(kJpegDcLuma), jpeg_make_huff(kJpegDcChroma)};
__constant__ JpegHuff kJpegAc[2] = {jpeg_make_huff(kJpegAcLuma), jpeg_make_huff(kJpegAcChroma)};

__host__ __device__ inline int64_t jpeg_interval_words(int mcus) { return ((int64_t)mcus * 6 * kJpegBlockBits + 31) / 32; }      // before stuffing, 32-bit words
__host__ __device__ inline int64_t jpeg_interval_bound(int mcus) { return 2 * (((int64_t)mcus * 6 * kJpegBlockBits + 7) / 8) + 2; }

struct JpegTransformArgs {
    const void* img[kPngMaxImages];   // (H, W, C) float32 or uint8
    float div[kPngMaxImages];
    uint32_t magma;                   // bit m: image m goes through the colour map (C == 1)
    int M, H, W, H2, W2, mx, my;      // H2, W2: the even crop; mx, my: MCUs per row, MCU rows
    int scale;                        // the IJG scaling of the quality: 5000 / q below 50, 200 - 2 q from 50
    int16_t* coef;                    // (M, my, mx, 6, 64): quantised, zigzag order
};

struct JpegArgs {
    int mx, my;
    int64_t n_blocks, n_intervals;    // M * my * mx * 6, M * my
    const int16_t* coef;
    uint32_t* slots;                  // n_blocks x kJpegSlotWords: a block's bits, most significant bit first
    uint32_t* bit_len;                // n_blocks
    uint32_t* bit_off;                // n_blocks: where the block starts inside its interval
    uint32_t* cat;                    // n_intervals x jpeg_interval_words(mx): the interval before stuffing
    uint32_t* ivl_bytes;              // n_intervals: bytes before stuffing
    uint32_t* ivl_len;                // n_intervals: bytes in the stream (stuffed, with the marker)
    int64_t* ivl_off;                 // n_intervals: where it starts in `streams`
    uint8_t* streams;
};

__device__ __forceinline__ int jpeg_luma(const uint32_t* q) { return (int)((19595u * q[0] + 38470u * q[1] + 7471u * q[2] + 32768u) >> 16); }
__device__ __forceinline__ int jpeg_chroma(const uint32_t* q, bool red) {
    const int r = (int)q[0], g = (int)q[1], b = (int)q[2];
    return (red ? 32768 * r - 27439 * g - 5329 * b + 8388608 + 32767 : -11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
}

// grid (blocks of an image / 4, image): one wave per block, in stream order (MCU row, MCU, block of the MCU)
template <int C, bool U8>
__global__ __launch_bounds__(kJpegThreads) void jpeg_transform_kernel(JpegTransformArgs a) {
    __shared__ int tile[kJpegThreads / 64][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 3, c = lane & 7;
    const int m = blockIdx.y;
    const int64_t per_image = (int64_t)a.my * a.mx * 6, local = (int64_t)blockIdx.x * (kJpegThreads / 64) + w, blk = m * per_image + local;
    const bool active = local < per_image;                    // (whole waves: the barriers below are reached by every thread)
    const int64_t mcu = local / 6, row = mcu / a.mx;
    const int b = (int)(local - mcu * 6), mxi = (int)(mcu - row * a.mx), myi = (int)row;
    const void* src = a.img[m];
    const float d = a.div[m];
    const bool magma = (a.magma >> m) & 1u;
    auto pixel = [&](int y, int x, uint32_t* q) {
        png_pixel<C, U8>(src, (int64_t)min(y, a.H2 - 1) * a.W + min(x, a.W2 - 1), d, magma, q);
        if (C == 1 && !magma) q[1] = q[2] = q[0];
    };
    int v = 128;
    if (active) {
        uint32_t q[3];
        if (b < 4) {
            pixel(16 * myi + 8 * (b >> 1) + r, 16 * mxi + 8 * (b & 1) + c, q);
            v = jpeg_luma(q);
        } else {
            int sum = 2;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pixel(16 * myi + 2 * r + (k >> 1), 16 * mxi + 2 * c + (k & 1), q);
                sum += jpeg_chroma(q, b == 5);
            }
            v = sum >> 2;
        }
    }
    tile[w][0][lane] = v - 128;
    __syncthreads();
    int acc = 256;
#pragma unroll
    for (int n = 0; n < 8; ++n) acc += kJpegDct.m[c * 8 + n] * tile[w][0][r * 8 + n];        // rows: |sum| <= 8 * 32138 * 128 < 2^25
    tile[w][1][lane] = acc >> 9;                              // 128 times the 1-D transform, below 2^17
    __syncthreads();
    int64_t wide = 524288;
#pragma unroll
    for (int n = 0; n < 8; ++n) wide += (int64_t)kJpegDct.m[r * 8 + n] * tile[w][1][n * 8 + c];   // columns: below 2^35, one 32 x 32 -> 64 multiply-add each
    const int c8 = (int)(wide >> 20);                                                                 // eight times the coefficient
    const int e = min(max((kJpegQuant[b >= 4][lane] * a.scale + 50) / 100, 1), 255);
    const int mag = (abs(c8) + 4 * e) / (8 * e);                                               // half away from zero
    if (active) a.coef[blk * 64 + kJpegZig.pos[lane]] = (int16_t)(c8 < 0 ? -mag : mag);
}

// one lane per block: bits into the accumulator, full words out to the slot
__global__ __launch_bounds__(kJpegThreads) void jpeg_entropy_kernel(JpegArgs a) {
    const int64_t blk = (int64_t)blockIdx.x * kJpegThreads + threadIdx.x;
    if (blk >= a.n_blocks) return;
    const int64_t mcu = blk / 6;
    const int b = (int)(blk - mcu * 6), mxi = (int)(mcu % a.mx), tab = b >= 4;
    const int16_t* zz = a.coef + blk * 64;
    int pred = 0;                                             // the previous block of the component: the block before for Y01 Y10 Y11, else in the MCU before
    if (b >= 1 && b <= 3) pred = zz[-64];
    else if (mxi > 0) pred = zz[-64 * (b == 0 ? 3 : 6)];
    uint32_t* slot = a.slots + blk * kJpegSlotWords;
    uint64_t acc = 0;
    int held = 0, words = 0;
    auto put = [&](uint32_t bits, int n) {                    // n <= 26, held < 32
        acc = (acc << n) | bits;
        held += n;
        if (held >= 32) { held -= 32; slot[words++] = (uint32_t)(acc >> held); }
    };
    auto coded = [&](const JpegHuff& h, int run, int v) {     // the symbol (run, category of v) and the category's low bits of v (v - 1 for a negative v)
        const int size = v ? 32 - __clz(abs(v)) : 0, sym = run << 4 | size;
        put((uint32_t)h.code[sym] << size | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u)), h.len[sym] + size);
    };
    coded(kJpegDc[tab], 0, (int)zz[0] - pred);
    const JpegHuff& ac = kJpegAc[tab];
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) put(ac.code[0xF0], ac.len[0xF0]);
        coded(ac, run, v);
        run = 0;
    }
    if (run) put(ac.code[0], ac.len[0]);
    if (held) slot[words] = (uint32_t)(acc << (32 - held));
    a.bit_len[blk] = 32u * words + held;
}

__device__ __forceinline__ uint32_t jpeg_slot_bits(const uint32_t* slot, uint32_t at, uint32_t n) {      // n <= 32 bits of a slot from bit `at`, right-aligned
    const uint32_t w = at >> 5, sh = at & 31u;
    uint64_t v = (uint64_t)slot[w] << 32;
    if (sh + n > 32) v |= slot[w + 1];                        // (only then: the word after the string's last one is not the slot's)
    return (uint32_t)((v >> (64 - sh - n)) & ((1ull << n) - 1ull));
}

// one workgroup per interval
__global__ __launch_bounds__(kZipThreads) void jpeg_assemble_kernel(JpegArgs a) {
    __shared__ uint32_t scan[kZipThreads];
    __shared__ uint32_t tot, ff;
    const int t = threadIdx.x;
    const int64_t iv = blockIdx.x;
    const int nb = 6 * a.mx;
    const uint32_t* len = a.bit_len + iv * nb;
    const uint32_t* slots = a.slots + iv * nb * kJpegSlotWords;
    uint32_t* off = a.bit_off + iv * nb;
    uint32_t bits = 0;
    if (t == 0) ff = 0;
    for (int k0 = 0; k0 < nb; k0 += kZipThreads) {
        const int k = k0 + t;
        const uint32_t l = k < nb ? len[k] : 0u;
        const uint32_t incl = zip_scan_add(l, scan);
        if (k < nb) off[k] = bits + incl - l;
        if (t == kZipThreads - 1) tot = incl;
        __syncthreads();
        bits += tot;
        __syncthreads();                                      // (also: `off` is read below by other threads of this workgroup)
    }
    const uint32_t n_bytes = (bits + 7) / 8, n_words = (bits + 31) / 32;
    uint32_t* cat = a.cat + iv * jpeg_interval_words(a.mx);
    uint32_t n_ff = 0;
    for (uint32_t j = t; j < n_words; j += kZipThreads) {
        const uint32_t p = 32 * j;
        int lo = 0, hi = nb - 1;                              // the last block that starts at or before bit p (every block has at least 4 bits)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= p) lo = mid; else hi = mid - 1;
        }
        uint32_t word = 0, got = 0, at = p - off[lo];
        for (int i = lo; got < 32 && i < nb; ++i, at = 0) {
            const uint32_t take = min(len[i] - at, 32u - got);
            word |= jpeg_slot_bits(slots + (int64_t)i * kJpegSlotWords, at, take) << (32 - got - take);      // (take >= 1: the shift is below 32)
            got += take;
        }
        if (got < 32) word |= 0xFFFFFFFFu >> got;             // the padding: 1-bits to the byte boundary (the bytes after it are not read)
        cat[j] = word;
#pragma unroll
        for (int k = 0; k < 4; ++k) n_ff += (4 * j + k < n_bytes && ((word >> (24 - 8 * k)) & 0xFFu) == 0xFFu) ? 1u : 0u;
    }
    if (n_ff) atomicAdd(&ff, n_ff);
    __syncthreads();
    if (t == 0) {
        a.ivl_bytes[iv] = n_bytes;
        a.ivl_len[iv] = n_bytes + ff + (iv % a.my < a.my - 1 ? 2u : 0u);
    }
}

// one workgroup per interval: 16 bytes per thread and round
__global__ __launch_bounds__(kZipThreads) void jpeg_emit_kernel(JpegArgs a) {
    __shared__ uint32_t scan[kZipThreads];
    __shared__ uint32_t tot;
    const int t = threadIdx.x;
    const int64_t iv = blockIdx.x;
    const uint32_t n_bytes = a.ivl_bytes[iv];
    const uint32_t* cat = a.cat + iv * jpeg_interval_words(a.mx);
    uint8_t* dst = a.streams + a.ivl_off[iv];
    uint32_t base = 0;                                        // stuffing bytes in front of this round
    for (uint32_t b0 = 0; b0 < n_bytes; b0 += 16 * kZipThreads) {
        const uint32_t first = b0 + 16 * t;
        uint32_t w[4] = {0, 0, 0, 0}, n_ff = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (first + 4 * k < n_bytes) w[k] = cat[first / 4 + k];
#pragma unroll
        for (int k = 0; k < 16; ++k) n_ff += (first + k < n_bytes && ((w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu) == 0xFFu) ? 1u : 0u;
        const uint32_t incl = zip_scan_add(n_ff, scan);
        if (t == kZipThreads - 1) tot = incl;
        uint8_t* p = dst + first + base + incl - n_ff;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t byte = (w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu;
            if (first + k < n_bytes) {
                *p++ = (uint8_t)byte;
                if (byte == 0xFFu) *p++ = 0;
            }
        }
        __syncthreads();
        base += tot;
        __syncthreads();
    }
    const int myi = (int)(iv % a.my);
    if (t == 0 && myi < a.my - 1) { dst[n_bytes + base] = 0xFF; dst[n_bytes + base + 1] = (uint8_t)(0xD0 + (myi & 7)); }
}

}  // namespace iris
