// Device-side deflate of OpenEXR ZIP / ZIPS scanline blocks (the writer's last host stage: utils/exr.py _deflate_predicted).
//
// Input: the PREDICTED bytes of every scanline block of M maps (utils/exr.scanline_blocks_torch: planar B,G,R rows, even/odd byte reorder, delta
// predictor).  Output: every map's chunk records as the file stores them, back to back (int32 y, int32 size, data), and per-map byte offsets.
// A chunk's data is a zlib stream (RFC 1950) of the predicted bytes when that stream is shorter than the block, else the raw block bytes
// (un-predicted here) -- OpenEXR's rule; the reader tells the two apart by size.
//
// Encoder: each chunk is cut into segments of kZipSeg bytes, one workgroup per segment, each segment one deflate block (RFC 1951) with its own
// code: dynamic Huffman (BTYPE 2) over literals and matches at distance 1 only -- runs of one predicted byte, zlib's Z_RLE parse -- or a stored
// block when that is not larger.  A non-final segment is closed by an empty stored block (zlib's sync flush) so that every segment ends
// byte-aligned and the chunk is the concatenation of its segments; only the chunk's last segment sets BFINAL.
//   1. runs      : each thread owns 64 consecutive bytes; two block scans give the start of the run its first byte is in and the end of the run
//                  its last byte is in, so every thread parses its bytes alone (literal at a run start, then matches of 258, a last match >= 3 or
//                  the 1-2 left-over bytes as literals)
//   2. histogram : LDS atomics
//   3. lengths   : rank sort of the used symbols by the workgroup, then on one thread the in-place minimum-redundancy algorithm (Moffat &
//                  Katajainen 1995), limited to 15 bits (7 for the code-length code) by moving codes down the length counts; every code is
//                  complete; the distance code is a single 1-bit code (zlib accepts an incomplete set of one distance code)
//   4. codes     : canonical, bit-reversed (deflate sends Huffman codes MSB first into an LSB-first stream)
//   5. packing   : per-thread bit counts, a block scan, atomicOr into LDS words (disjoint bit ranges: the result does not depend on the order)
// Then, per chunk, segment sizes and Adler-32 partials are combined; one workgroup scans the record sizes of all maps; one workgroup per chunk
// writes its record (the segments by copy, or the raw block by an un-predicting scan).  No allocation: the caller passes the workspace.
// The segment and offsets kernels also serve the PNG writer (iris_png.h): one chunk per image, always the zlib stream, no record header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iris {

constexpr int kZipThreads = 256;
constexpr int kZipSeg = 16384;                          // bytes per segment: one deflate block (zlib's Z_RLE closes a block every ~16 K symbols too)
constexpr int kZipSpan = kZipSeg / kZipThreads;         // bytes per thread in the parse
constexpr int kZipSegCap = kZipSeg + 64;                // workspace bytes per segment: a segment is never larger than a stored block (kZipSeg + 5)
constexpr int kZipLitSyms = 286, kZipClSyms = 19;
constexpr uint32_t kAdlerMod = 65521;

struct ZipArgs {
    const uint8_t* full;      // (M, n_full, B) predicted bytes
    const uint8_t* tail;      // (M, T)
    int M, lines, sf, st;     // maps, scanlines per chunk, segments per full / tail chunk
    int64_t n_full, B, T;
    uint8_t* records;
    int64_t* map_offsets;     // M + 1
    uint8_t* seg_data;        // n_segs x kZipSegCap
    uint32_t* seg_len;        // n_segs
    uint32_t* seg_adler;      // n_segs x 2: sum of bytes, sum of (L_seg - i) * byte_i, both mod 65521
    uint32_t* chunk_len;      // data bytes of each chunk (== its block size: raw)
    uint32_t* chunk_adler;
    int64_t* chunk_off;
    uint32_t* seg_off;        // PNG mode (iris_png.h): where each segment starts inside its chunk's stream; NULL for EXR records
    int record_header;        // bytes in front of each chunk's data: 8 (int32 y, int32 size) for EXR records, 0 for a bare zlib stream
};

// chunks: the M * n_full full blocks map by map, then the M tails
__device__ __forceinline__ int64_t zip_n_chunks(const ZipArgs& a) { return (int64_t)a.M * a.n_full + (a.T > 0 ? a.M : 0); }
__device__ __forceinline__ const uint8_t* zip_chunk_src(const ZipArgs& a, int64_t ci, int64_t& L) {
    const int64_t nf = (int64_t)a.M * a.n_full;
    if (ci < nf) { L = a.B; return a.full + ci * a.B; }
    L = a.T; return a.tail + (ci - nf) * a.T;
}
__device__ __forceinline__ int64_t zip_seg_base(const ZipArgs& a, int64_t ci, int& nseg) {
    const int64_t nf = (int64_t)a.M * a.n_full;
    if (ci < nf) { nseg = a.sf; return ci * a.sf; }
    nseg = a.st; return nf * a.sf + (ci - nf) * a.st;
}

// deflate's length codes 257..285: base lengths and extra bits
__constant__ uint16_t kZipLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kZipLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint8_t kZipClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int zip_len_index(int len) {          // 3..258 -> 0..28 (258 has a code of its own)
    if (len == 258) return 28;
    int k = 27;
    while (kZipLenBase[k] > len) --k;
    return k;
}

// Hillis-Steele inclusive scans over the workgroup's 256 values (s: 256 words of LDS)
__device__ __forceinline__ uint32_t zip_scan_add(uint32_t v, uint32_t* s) {
    const int t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (int o = 1; o < kZipThreads; o <<= 1) {
        const uint32_t w = t >= o ? s[t - o] : 0u;
        __syncthreads(); s[t] += w; __syncthreads();
    }
    const uint32_t r = s[t]; __syncthreads();
    return r;
}
__device__ __forceinline__ int zip_scan_max(int v, int* s) {
    const int t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (int o = 1; o < kZipThreads; o <<= 1) {
        const int w = t >= o ? s[t - o] : -1;
        __syncthreads(); s[t] = max(s[t], w); __syncthreads();
    }
    const int r = s[t]; __syncthreads();
    return r;
}
__device__ __forceinline__ int zip_scan_min_rev(int v, int* s) {  // min over this thread and the ones after it
    const int t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (int o = 1; o < kZipThreads; o <<= 1) {
        const int w = t + o < kZipThreads ? s[t + o] : 0x7fffffff;
        __syncthreads(); s[t] = min(s[t], w); __syncthreads();
    }
    const int r = s[t]; __syncthreads();
    return r;
}

// The parse of the bytes [lo, hi) of a segment: p_in = start of the run d[lo] is in, e_after = end of the run d[hi - 1] is in when that run
// reaches hi.  lit(byte) / match(length) per token, in stream order.
template <class Lit, class Match>
__device__ __forceinline__ void zip_parse(const uint8_t* d, int lo, int hi, int p_in, int e_after, Lit&& lit, Match&& match) {
    int p = p_in, e = -1;
    for (int i = lo; i < hi; ++i) {
        const uint8_t c = d[i];
        if (i == 0 || c != d[i - 1]) { p = i; e = -1; }
        if (e < 0) {
            int k = i + 1;
            while (k < hi && d[k] == c) ++k;
            e = k < hi ? k : e_after;
        }
        const int k = i - p;
        if (k == 0) { lit(c); continue; }
        const int rest = e - p - 1, j = k - 1, q = rest / 258, r = rest - q * 258, piece = j / 258, off = j - piece * 258;
        if (piece < q) { if (off == 0) match(258); }
        else if (r >= 3) { if (off == 0) match(r); }
        else lit(c);
    }
}

__device__ __forceinline__ void zip_put(uint32_t* w, uint32_t pos, uint32_t v, int n) {   // n <= 31 bits of v at bit pos
    if (n == 0) return;
    const uint32_t s = pos & 31;
    atomicOr(&w[pos >> 5], v << s);
    if (s + n > 32) atomicOr(&w[(pos >> 5) + 1], v >> (32 - s));
}

struct ZipHuffScratch {
    uint32_t A[kZipLitSyms];   // sorted frequencies, then code lengths (Moffat & Katajainen, in place)
    uint16_t sym[kZipLitSyms];
    uint32_t blc[64];
    int nz;
};

// Code lengths (<= maxlen, complete) of the n symbols with frequencies f -> len.  Called by the whole workgroup.
__device__ void zip_huff_lengths(const uint32_t* f, int n, int maxlen, uint8_t* len, ZipHuffScratch& h) {
    const int t = threadIdx.x;
    if (t == 0) h.nz = 0;
    for (int s = t; s < n; s += kZipThreads) len[s] = 0;
    __syncthreads();
    for (int s = t; s < n; s += kZipThreads) {
        const uint32_t fs = f[s];
        if (!fs) continue;
        int rank = 0;
        for (int u = 0; u < n; ++u) {
            const uint32_t fu = f[u];
            rank += (fu != 0u) & ((fu < fs) | ((fu == fs) & (u < s)));
        }
        h.sym[rank] = (uint16_t)s; h.A[rank] = fs;
        atomicAdd(&h.nz, 1);
    }
    __syncthreads();
    if (t == 0) {
        const int nz = h.nz;
        uint32_t* A = h.A;
        if (nz == 1) {                                           // one used symbol: pair it with another one so that the code is complete
            const int s0 = h.sym[0];
            len[s0] = 1; len[s0 == 0 ? 1 : 0] = 1;
        } else if (nz >= 2) {
            A[0] += A[1];                                        // phase 1: internal node weights, parents in place
            int root = 0, leaf = 2;
            for (int next = 1; next < nz - 1; ++next) {
                if (leaf >= nz || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
                else A[next] = A[leaf++];
                if (leaf >= nz || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
                else A[next] += A[leaf++];
            }
            A[nz - 2] = 0;                                       // phase 2: internal node depths
            for (int next = nz - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
            int avbl = 1, used = 0, dpth = 0, root2 = nz - 2, next = nz - 1;     // phase 3: leaf depths
            while (avbl > 0) {
                while (root2 >= 0 && (int)A[root2] == dpth) { ++used; --root2; }
                while (avbl > used) { A[next--] = dpth; --avbl; }
                avbl = 2 * used; ++dpth; used = 0;
            }
            for (int i = 0; i < 64; ++i) h.blc[i] = 0;
            for (int i = 0; i < nz; ++i) h.blc[min((int)A[i], 63)]++;
            for (int i = maxlen + 1; i < 64; ++i) { h.blc[maxlen] += h.blc[i]; h.blc[i] = 0; }
            uint32_t total = 0;
            for (int i = 1; i <= maxlen; ++i) total += h.blc[i] << (maxlen - i);
            while (total > (1u << maxlen)) {                      // over-subscribed after the clamp: lengthen codes until the Kraft sum is 1
                h.blc[maxlen]--;
                for (int i = maxlen - 1; i > 0; --i)
                    if (h.blc[i]) { h.blc[i]--; h.blc[i + 1] += 2; break; }
                --total;
            }
            int j = 0;                                           // the rarest symbols get the longest codes
            for (int i = maxlen; i > 0; --i)
                for (uint32_t l = h.blc[i]; l > 0; --l) len[h.sym[j++]] = (uint8_t)i;
        }
    }
    __syncthreads();
}

__device__ void zip_canonical(const uint8_t* len, int n, uint16_t* code) {     // one thread
    uint32_t bl[16] = {0}, next[16];
    for (int s = 0; s < n; ++s) bl[len[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + bl[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < n; ++s)
        if (len[s]) code[s] = (uint16_t)(__brev(next[len[s]]++) >> (32 - len[s]));
}

// One workgroup per segment -> seg_data / seg_len / seg_adler.
__global__ __launch_bounds__(kZipThreads) void zip_segment_kernel(ZipArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t d[kZipSeg];
    __shared__ uint32_t out[kZipSegCap / 4];
    __shared__ uint32_t hist[kZipLitSyms];
    __shared__ uint8_t lens[kZipLitSyms];
    __shared__ uint16_t codes[kZipLitSyms];
    __shared__ uint32_t cl_freq[kZipClSyms];
    __shared__ uint8_t cl_len[kZipClSyms];
    __shared__ uint16_t cl_code[kZipClSyms];
    __shared__ uint8_t rle_sym[kZipLitSyms + 1];
    __shared__ uint8_t rle_extra[kZipLitSyms + 1];
    __shared__ uint32_t scan[kZipThreads];
    __shared__ ZipHuffScratch hs;
    __shared__ uint32_t s_hdr_bits, s_hlit, s_hclen, s_nrle, s_adler_a, s_adler_b, s_raw_only;

    const int t = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t nfs = (int64_t)a.M * a.n_full * a.sf;
    int64_t ci; int s;
    if (g < nfs) { ci = g / a.sf; s = (int)(g - ci * a.sf); }
    else { const int64_t r = g - nfs; ci = (int64_t)a.M * a.n_full + r / a.st; s = (int)(r % a.st); }
    int64_t L;
    const uint8_t* src = zip_chunk_src(a, ci, L) + (int64_t)s * kZipSeg;
    const int n = (int)min<int64_t>(kZipSeg, L - (int64_t)s * kZipSeg);
    const int nseg = ci < (int64_t)a.M * a.n_full ? a.sf : a.st;
    const bool final_seg = s == nseg - 1;

    if ((((uintptr_t)src) & 3) == 0) {
        const int nw = n >> 2;
        for (int i = t; i < nw; i += kZipThreads) reinterpret_cast<uint32_t*>(d)[i] = reinterpret_cast<const uint32_t*>(src)[i];
        for (int i = (nw << 2) + t; i < n; i += kZipThreads) d[i] = src[i];
    } else {
        for (int i = t; i < n; i += kZipThreads) d[i] = src[i];
    }
    for (int i = t; i < kZipLitSyms; i += kZipThreads) hist[i] = 0;
    if (t < kZipClSyms) cl_freq[t] = 0;
    if (t == 0) { s_adler_a = 0; s_adler_b = 0; }
    __syncthreads();

    // 1. runs
    const int lo = min(t * kZipSpan, n), hi = min(lo + kZipSpan, n);
    int last_start = -1, first_start = 0x7fffffff;
    uint32_t sa = 0, sb = 0;
    for (int i = lo; i < hi; ++i) {
        if (i == 0 || d[i] != d[i - 1]) { last_start = i; first_start = min(first_start, i); }
        sa += d[i]; sb += (uint32_t)(n - i) * d[i];
    }
    atomicAdd(&s_adler_a, sa % kAdlerMod); atomicAdd(&s_adler_b, sb % kAdlerMod);
    // p_in: the last run start before lo (exclusive maximum over the threads before); e_run: the first run start at or after hi (exclusive minimum
    // over the threads after), n when there is none -- the end of the run the span's last byte is in, when that run reaches hi
    const int max_incl = zip_scan_max(last_start, reinterpret_cast<int*>(scan));
    const int min_incl = zip_scan_min_rev(first_start, reinterpret_cast<int*>(scan));
    scan[t] = (uint32_t)max_incl; __syncthreads();
    const int p_in = t > 0 ? (int)scan[t - 1] : 0;
    __syncthreads();
    scan[t] = (uint32_t)min_incl; __syncthreads();
    const int e_run = min(t + 1 < kZipThreads ? (int)scan[t + 1] : n, n);
    __syncthreads();

    // 2. histogram
    zip_parse(d, lo, hi, p_in, e_run, [&](uint8_t c) { atomicAdd(&hist[c], 1u); },
              [&](int len) { atomicAdd(&hist[257 + zip_len_index(len)], 1u); });
    if (t == 0) hist[256] = 1;
    __syncthreads();

    // Early out: the entropy of the token histogram bounds the Huffman-coded size from below (header and extra bits not counted).  When that bound
    // is within 0.5 % of the stored block -- Monte-Carlo noise: the mantissa bytes are incompressible -- the segment is stored without building a
    // code; at most 0.5 % of such a segment is given up.  (Fixed-order reductions: the decision is deterministic.)
    {
        float e = 0.f; uint32_t ntok = 0;
        for (int sy = t; sy < kZipLitSyms; sy += kZipThreads) { const uint32_t f = hist[sy]; ntok += f; if (f) e += (float)f * __log2f((float)f); }
        for (int o = 32; o > 0; o >>= 1) { e += __shfl_down(e, o); ntok += __shfl_down(ntok, o); }
        if ((t & 63) == 0) { reinterpret_cast<float*>(scan)[t >> 6] = e; scan[4 + (t >> 6)] = ntok; }
        __syncthreads();
        if (t == 0) {
            const float* ef = reinterpret_cast<const float*>(scan);
            const float se = ((ef[0] + ef[1]) + ef[2]) + ef[3];
            const float nt = (float)(((scan[4] + scan[5]) + scan[6]) + scan[7]);
            s_raw_only = nt * __log2f(nt) - se >= 0.995f * 8.f * (float)n ? 1u : 0u;
        }
        __syncthreads();
    }
    uint8_t* dst = a.seg_data + g * kZipSegCap;
    const uint32_t stored_bytes = (uint32_t)n + 5;
    uint32_t dyn_bytes = 0xFFFFFFFFu, my_bits = 0, incl = 0, hdr = 0, end_bits = 0;
    if (!s_raw_only) {
    // 3. code lengths of the literal/length code
    zip_huff_lengths(hist, kZipLitSyms, 15, lens, hs);

    // the code-length sequence (HLIT literal/length lengths, then the one distance length), run-length coded as RFC 1951 3.2.7 defines it
    if (t == 0) {
        int hlit = kZipLitSyms;
        while (hlit > 257 && lens[hlit - 1] == 0) --hlit;
        const int total = hlit + 1;
        int nr = 0, i = 0;
        while (i < total) {
            const int v = i < hlit ? lens[i] : 1;
            int run = 1;
            while (i + run < total && (i + run < hlit ? lens[i + run] : 1) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = min(run, 138); rle_sym[nr] = 18; rle_extra[nr++] = (uint8_t)(r - 11); run -= r; }
                if (run >= 3) { rle_sym[nr] = 17; rle_extra[nr++] = (uint8_t)(run - 3); run = 0; }
            } else {
                rle_sym[nr] = (uint8_t)v; rle_extra[nr++] = 0; --run;
                while (run >= 3) { const int r = min(run, 6); rle_sym[nr] = 16; rle_extra[nr++] = (uint8_t)(r - 3); run -= r; }
            }
            while (run > 0) { rle_sym[nr] = (uint8_t)v; rle_extra[nr++] = 0; --run; }
        }
        for (int k = 0; k < nr; ++k) cl_freq[rle_sym[k]]++;
        s_nrle = nr; s_hlit = hlit;
    }
    __syncthreads();
    zip_huff_lengths(cl_freq, kZipClSyms, 7, cl_len, hs);
    if (t == 0) {
        int hclen = kZipClSyms;
        while (hclen > 4 && cl_len[kZipClOrder[hclen - 1]] == 0) --hclen;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (uint32_t k = 0; k < s_nrle; ++k) {
            const int sy = rle_sym[k];
            bits += cl_len[sy] + (sy == 16 ? 2 : sy == 17 ? 3 : sy == 18 ? 7 : 0);
        }
        s_hdr_bits = bits; s_hclen = hclen;
        zip_canonical(lens, kZipLitSyms, codes);
        zip_canonical(cl_len, kZipClSyms, cl_code);
    }
    __syncthreads();

    // 5. bit lengths, offsets, the choice between this block and a stored one
    zip_parse(d, lo, hi, p_in, e_run, [&](uint8_t c) { my_bits += lens[c]; },
              [&](int len) { const int k = zip_len_index(len); my_bits += lens[257 + k] + kZipLenExtra[k] + 1; });
    incl = zip_scan_add(my_bits, scan);
    scan[t] = incl; __syncthreads();
    const uint32_t all_bits = scan[kZipThreads - 1];
    __syncthreads();
    hdr = s_hdr_bits;
    end_bits = hdr + all_bits + lens[256];                                // through the end-of-block code
    dyn_bytes = final_seg ? (end_bits + 7) / 8 : (end_bits + 3 + 7) / 8 + 4;
    }

    if (dyn_bytes < stored_bytes) {
        const uint32_t nw = (dyn_bytes + 3) / 4;
        for (uint32_t i = t; i < nw; i += kZipThreads) out[i] = 0;
        __syncthreads();
        if (t == 0) {
            uint32_t pos = 0;
            zip_put(out, pos, (final_seg ? 1u : 0u) | (2u << 1), 3); pos += 3;
            zip_put(out, pos, s_hlit - 257, 5); pos += 5;
            zip_put(out, pos, 0, 5); pos += 5;                   // HDIST - 1: one distance code
            zip_put(out, pos, s_hclen - 4, 4); pos += 4;
            for (uint32_t k = 0; k < s_hclen; ++k) { zip_put(out, pos, cl_len[kZipClOrder[k]], 3); pos += 3; }
            for (uint32_t k = 0; k < s_nrle; ++k) {
                const int sy = rle_sym[k];
                zip_put(out, pos, cl_code[sy], cl_len[sy]); pos += cl_len[sy];
                const int xb = sy == 16 ? 2 : sy == 17 ? 3 : sy == 18 ? 7 : 0;
                zip_put(out, pos, rle_extra[k], xb); pos += xb;
            }
            zip_put(out, end_bits - lens[256], codes[256], lens[256]);
        }
        uint32_t pos = hdr + incl - my_bits;
        zip_parse(d, lo, hi, p_in, e_run, [&](uint8_t c) { zip_put(out, pos, codes[c], lens[c]); pos += lens[c]; },
                  [&](int len) {
                      const int k = zip_len_index(len), sy = 257 + k, nb = lens[sy] + kZipLenExtra[k];
                      zip_put(out, pos, codes[sy] | ((uint32_t)(len - kZipLenBase[k]) << lens[sy]), nb);
                      pos += nb + 1;                              // + the 1-bit distance code 0 (distance 1)
                  });
        __syncthreads();
        if (t == 0 && !final_seg) {                              // sync flush: empty stored block (3 zero bits), byte alignment, 00 00 FF FF
            const uint32_t b = (end_bits + 3 + 7) / 8;
            reinterpret_cast<uint8_t*>(out)[b + 2] = 0xFF; reinterpret_cast<uint8_t*>(out)[b + 3] = 0xFF;
        }
        __syncthreads();
        for (uint32_t i = t; i < nw; i += kZipThreads) reinterpret_cast<uint32_t*>(dst)[i] = out[i];
    } else {
        if (t == 0) {
            dst[0] = final_seg ? 1 : 0;                           // BFINAL, BTYPE 00, then byte alignment
            dst[1] = (uint8_t)(n & 0xFF); dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)(~n & 0xFF); dst[4] = (uint8_t)((~n >> 8) & 0xFF);
        }
        for (int i = t; i < n; i += kZipThreads) dst[5 + i] = d[i];
    }
    if (t == 0) {
        a.seg_len[g] = dyn_bytes < stored_bytes ? dyn_bytes : stored_bytes;
        a.seg_adler[2 * g] = s_adler_a % kAdlerMod; a.seg_adler[2 * g + 1] = s_adler_b % kAdlerMod;
    }
}

// Per chunk: stream size (zlib header + segments + Adler-32) against the block size, and the chunk's Adler-32.
__global__ void zip_chunk_kernel(ZipArgs a) {
    const int64_t nch = zip_n_chunks(a);
    for (int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ci < nch; ci += (int64_t)gridDim.x * blockDim.x) {
        int nseg;
        const int64_t base = zip_seg_base(a, ci, nseg);
        int64_t L;
        zip_chunk_src(a, ci, L);
        uint64_t bytes = 2 + 4;
        uint32_t A = 1, Bs = 0;
        int64_t rem = L;
        for (int k = 0; k < nseg; ++k) {
            const uint32_t ls = (uint32_t)min<int64_t>(kZipSeg, rem);
            rem -= ls;
            bytes += a.seg_len[base + k];
            Bs = (uint32_t)((Bs + (uint64_t)ls * A + a.seg_adler[2 * (base + k) + 1]) % kAdlerMod);
            A = (A + a.seg_adler[2 * (base + k)]) % kAdlerMod;
        }
        a.chunk_len[ci] = bytes < (uint64_t)L ? (uint32_t)bytes : (uint32_t)L;
        a.chunk_adler[ci] = (Bs << 16) | A;
    }
}

// One workgroup: exclusive scan of the record sizes in file order (map by map, chunk by chunk) -> chunk_off, map_offsets.
constexpr int kZipScanThreads = 1024;
__global__ __launch_bounds__(kZipScanThreads) void zip_offsets_kernel(ZipArgs a) {
    __shared__ uint64_t s[kZipScanThreads];
    const int t = threadIdx.x;
    const int64_t nc = a.n_full + (a.T > 0 ? 1 : 0), N = (int64_t)a.M * nc;
    const int64_t per = (N + kZipScanThreads - 1) / kZipScanThreads, k0 = min<int64_t>(N, t * per), k1 = min<int64_t>(N, k0 + per);
    auto chunk_of = [&](int64_t k) { const int64_t m = k / nc, c = k - m * nc; return c < a.n_full ? m * a.n_full + c : (int64_t)a.M * a.n_full + m; };
    uint64_t sum = 0;
    for (int64_t k = k0; k < k1; ++k) sum += a.record_header + a.chunk_len[chunk_of(k)];
    s[t] = sum; __syncthreads();
    for (int o = 1; o < kZipScanThreads; o <<= 1) {
        const uint64_t w = t >= o ? s[t - o] : 0;
        __syncthreads(); s[t] += w; __syncthreads();
    }
    uint64_t off = s[t] - sum;
    for (int64_t k = k0; k < k1; ++k) {
        const int64_t ci = chunk_of(k);
        if (k % nc == 0) a.map_offsets[k / nc] = (int64_t)off;
        a.chunk_off[ci] = (int64_t)off;
        off += a.record_header + a.chunk_len[ci];
    }
    if (t == kZipScanThreads - 1) a.map_offsets[a.M] = (int64_t)s[t];
}

// One workgroup per chunk: its record at chunk_off.
__global__ __launch_bounds__(kZipThreads) void zip_emit_kernel(ZipArgs a) {
    const int t = threadIdx.x;
    const int64_t ci = blockIdx.x;
    int64_t L;
    const uint8_t* src = zip_chunk_src(a, ci, L);
    const int64_t nf = (int64_t)a.M * a.n_full;
    const int32_t y = (int32_t)((ci < nf ? ci % a.n_full : a.n_full) * a.lines);
    const uint32_t len = a.chunk_len[ci];
    uint8_t* dst = a.records + a.chunk_off[ci];
    if (t < 8) {
        const uint32_t v = t < 4 ? (uint32_t)y : len;
        dst[t] = (uint8_t)(v >> (8 * (t & 3)));
    }
    dst += 8;
    if ((int64_t)len < L) {                                      // the zlib stream: 78 01 (32 K window, no dictionary), segments, Adler-32 big-endian
        if (t == 0) { dst[0] = 0x78; dst[1] = 0x01; }
        int nseg;
        const int64_t base = zip_seg_base(a, ci, nseg);
        uint32_t o = 2;
        for (int k = 0; k < nseg; ++k) {
            const uint32_t ls = a.seg_len[base + k];
            const uint8_t* sp = a.seg_data + (base + k) * kZipSegCap;
            for (uint32_t i = t; i < ls; i += kZipThreads) dst[o + i] = sp[i];
            o += ls;
        }
        if (t < 4) dst[o + t] = (uint8_t)(a.chunk_adler[ci] >> (24 - 8 * t));
        return;
    }
    // the raw block: undo the predictor (a prefix sum mod 256) and the even/odd reorder, in tiles of 4 bytes per thread (coalesced loads), a wave scan
    // and the wave totals of the tile in LDS (double-buffered: one barrier per tile)
    __shared__ uint32_t wsum[2][kZipThreads / 64];
    const int lane = t & 63, wid = t >> 6;
    const int64_t half = (L + 1) / 2;
    const bool aligned = (((uintptr_t)src) & 3) == 0;
    uint32_t carry = 0;
    for (int64_t base = 0, it = 0; base < L; base += 4 * kZipThreads, ++it) {
        const int64_t i0 = base + 4 * t;
        uint32_t e[4], s = 0;
        if (aligned && i0 + 4 <= L) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(src + i0);
            for (int k = 0; k < 4; ++k) e[k] = (w >> (8 * k)) & 0xFF;
        } else {
            for (int k = 0; k < 4; ++k) e[k] = i0 + k < L ? src[i0 + k] : 128u;
        }
        for (int k = 0; k < 4; ++k) { e[k] -= (i0 + k) ? 128u : 0u; s += e[k]; }       // (out-of-range bytes contribute 0)
        uint32_t v = s;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t w = __shfl_up(v, o); if (lane >= o) v += w; }
        if (lane == 63) wsum[it & 1][wid] = v;
        __syncthreads();
        uint32_t acc = carry + v - s, tot = 0;
        for (int w = 0; w < kZipThreads / 64; ++w) { const uint32_t x = wsum[it & 1][w]; tot += x; if (w < wid) acc += x; }
        carry += tot;
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k;
            if (i >= L) break;
            acc += e[k];
            dst[i < half ? 2 * i : 2 * (i - half) + 1] = (uint8_t)acc;
        }
    }
}

}  // namespace iris
