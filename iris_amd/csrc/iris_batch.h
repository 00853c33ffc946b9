// 5c-9: the trainers' pixel batch -- global pixel ids -> the rows the reference's loader slices from its host table.
//
// Reference: Inv*DatasetLDR(pixel=True) (utils/dataset/real_ldr.py:334-427, synthetic_ldr.py, scannetpp/dataset.py) keeps one float row per
// training pixel on the host -- rays_x | rays_d | dxdu | dydv | segmentation | rgb (16 floats), int_albedo (3), exposure (1), the shading
// cache (39) -- and __getitem__ slices a randperm of the rows.  Here the twelve ray floats are a function of the pixel's camera (24 floats per
// VIEW), images stay 8-bit, and one launch turns a list of ids into the batch: per element an 8-B id (coalesced), a 96-B camera row (V rows:
// resident in L2 / the vector cache), 3 + 3 + 4 scattered bytes of the 8-bit stores, and about 100 B of coalesced stores.
// One thread per element, no LDS traffic beyond the 1-KiB decode table, nothing shared between elements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iris_device.h"

namespace iris {

constexpr int kCamFloats = 24;       // K[9] | c2w[12] | focal | 2 pad: 96 B, six 16-B loads

struct PixelRay { f3 o, d, dxdu, dydv; };

// The rays of pixel (x, y): the ONE body of iris_raygen_real / iris_raygen_synthetic (raygen_kernel) and of pixel_batch_kernel, so that a batch row
// carries the bits the whole-view call writes.  (-ffp-contract=off: the operations below are the operations executed, wherever this is inlined.)
// ray_diff: d un-normalised, and dxdu / dydv are what the callers keep; else d normalised (dxdu / dydv are computed all the same: six products).
// (Returned by value and assigned once: an out-parameter filled in three branches stayed in private memory.)
__device__ __forceinline__ PixelRay raygen_pixel(const float* __restrict__ K, const float* __restrict__ c2w, float focal, int H, int W, int ray_diff,
                                                 int synthetic, int x, int y) {
    float dc0, dc1, ifx, ify;
    if (synthetic) {  // utils/dataset/synthetic_ldr.py:21-34
        const float hw = (float)((double)W / 2.0), hh = (float)((double)H / 2.0);
        dc0 = -(((float)x + 0.5f) - hw) / focal;
        dc1 = -(((float)y + 0.5f) - hh) / focal;
        ifx = ify = 1.0f / focal;
    } else {  // utils/dataset/real_ldr.py:49-61
        dc0 = ((float)x + 0.5f - K[2]) / K[0];
        dc1 = ((float)y + 0.5f - K[5]) / K[4];
        ifx = 1.0f / K[0]; ify = 1.0f / K[4];
    }
    const f3 d = mk3((dc0 * c2w[0] + dc1 * c2w[1]) + c2w[2], (dc0 * c2w[4] + dc1 * c2w[5]) + c2w[6], (dc0 * c2w[8] + dc1 * c2w[9]) + c2w[10]);
    float nrm = 1.f;          // ray_diff: d as it is
    if (!ray_diff) {
        nrm = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);  // synthetic: rays_d / torch.norm(rays_d); real: t_normalize, F.normalize's floor on the norm
        if (!synthetic) nrm = fmaxf(nrm, 1e-12f);
    }
    PixelRay r;
    r.o = mk3(c2w[3], c2w[7], c2w[11]);
    r.d = ray_diff ? d : mk3(d.x / nrm, d.y / nrm, d.z / nrm);
    r.dxdu = mk3(ifx * c2w[0], ifx * c2w[4], ifx * c2w[8]);
    r.dydv = mk3(ify * c2w[1], ify * c2w[5], ify * c2w[9]);
    return r;
}

// The rays of a per-view kernel (pool_view_kernel, label_vote_kernel, label_view_kernel), carried in its arguments: from_camera -> ray i is pixel
// (x, y) = (i % W, i / W) of an H x W view through raygen_pixel(camera), the rays of iris_raygen_real / iris_raygen_synthetic with ray_diff = 0; else
// o = rays_o[i * ray_stride], d = rays_d[i * ray_stride] (an (N,6) rays tensor is read in place).  The host fills it in view_rays_args (iris_hip.hip).
struct ViewRays {
    float camera[kCamFloats];
    int from_camera, H, W, synthetic;
    const float* rays_o; const float* rays_d; int64_t ray_stride;
    int64_t B;
};
struct Ray { f3 o, d; };
// ray i (i < v.B); by value and assigned once, as raygen_pixel's
__device__ __forceinline__ Ray view_ray(const ViewRays& v, int64_t i) {
    if (v.from_camera) {
        const int y = (int)(i / v.W), x = (int)(i - (int64_t)y * v.W);
        const PixelRay r = raygen_pixel(v.camera, v.camera + 9, v.camera[21], v.H, v.W, 0, v.synthetic, x, y);
        return Ray{r.o, r.d};
    }
    return Ray{ld3(v.rays_o + i * v.ray_stride), ld3(v.rays_d + i * v.ray_stride)};
}

struct PixelBatchArgs {
    const int64_t* ids; int64_t B;
    const float* cameras; int64_t V;
    int H, W, ray_diff, synthetic;
    const void* rgb; const void* albedo; int rgb_u8, albedo_u8;
    const int32_t* segmentation; const float* positions; const float* exposure;
    float* o_rays; float* o_rgbs; float* o_albedo; int64_t* o_segmentation; float* o_exposure; float* o_positions;
};

// three channels of pixel `id` of an (N,3) store: 8-bit through the decode table, float32 as stored
__device__ __forceinline__ f3 load_rgb(const void* __restrict__ store, int u8, int64_t id, const float* __restrict__ lut) {
    if (u8) {
        const uint8_t* p = (const uint8_t*)store + id * 3;
        return mk3(lut[p[0]], lut[p[1]], lut[p[2]]);
    }
    return ld3((const float*)store + id * 3);
}

__global__ __launch_bounds__(256) void pixel_batch_kernel(PixelBatchArgs a) {
    // u -> np.float32(u / 255.0): the float64 quotient rounded once (open_png, the albedo loader); u * (1.0f / 255.0f) rounds twice and differs in the last bit at 126 of the 256 levels
    __shared__ float lut[256];
    if (a.rgb_u8 || a.albedo_u8) {
        for (int u = threadIdx.x; u < 256; u += blockDim.x) lut[u] = (float)((double)u / 255.0);
        __syncthreads();
    }
    const int64_t hw = (int64_t)a.H * a.W, n_pixels = a.V * hw;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.B; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = a.ids[i];
        const bool ok = id >= 0 && id < n_pixels;          // (callers bound the ids on the host; an id outside the table reads nothing and gives a zero row)
        const int64_t view = ok ? id / hw : 0, pix = ok ? id - view * hw : 0;
        if (a.o_rays) {
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 row[3] = {z4, z4, z4};
            if (ok) {
                float cam[kCamFloats];
                const float4* c4 = reinterpret_cast<const float4*>(a.cameras + view * kCamFloats);
#pragma unroll
                for (int k = 0; k < kCamFloats / 4; ++k) {
                    const float4 v = c4[k];
                    cam[4 * k] = v.x; cam[4 * k + 1] = v.y; cam[4 * k + 2] = v.z; cam[4 * k + 3] = v.w;
                }
                const int y = (int)(pix / a.W), x = (int)(pix - (int64_t)y * a.W);
                const PixelRay r = raygen_pixel(cam, cam + 9, cam[21], a.H, a.W, a.ray_diff, a.synthetic, x, y);
                row[0] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
                row[1] = make_float4(r.d.y, r.d.z, 0.f, 0.f);
                if (a.ray_diff) {                             // (without it the whole-view call writes no differentials: the row carries zeros)
                    row[1].z = r.dxdu.x; row[1].w = r.dxdu.y;
                    row[2] = make_float4(r.dxdu.z, r.dydv.x, r.dydv.y, r.dydv.z);
                }
            }
            float4* o = reinterpret_cast<float4*>(a.o_rays + i * 12);      // 48-B rows of a 16-B aligned buffer
            o[0] = row[0]; o[1] = row[1]; o[2] = row[2];
        }
        if (a.o_rgbs) {
            f3 v = mk3(0.f, 0.f, 0.f);
            if (ok) v = load_rgb(a.rgb, a.rgb_u8, id, lut);
            st3(a.o_rgbs + i * 3, v);
        }
        if (a.o_albedo) {
            f3 v = mk3(0.f, 0.f, 0.f);
            if (ok) v = load_rgb(a.albedo, a.albedo_u8, id, lut);
            st3(a.o_albedo + i * 3, v);
        }
        if (a.o_segmentation) a.o_segmentation[i] = ok ? (int64_t)a.segmentation[id] : -1;
        if (a.o_exposure) a.o_exposure[i] = ok ? a.exposure[view] : 0.f;
        if (a.o_positions) {
            f3 v = mk3(0.f, 0.f, 0.f);
            if (ok) v = ld3(a.positions + id * 3);
            st3(a.o_positions + i * 3, v);
        }
    }
}

}  // namespace iris
