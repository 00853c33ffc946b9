// libiris_hip.so -- kernels and C ABI (include/iris_hip.h).  gfx950 / wave64 only.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/iris_hip.h"
#include "../../include/iris_hip_debug.h"
#include "bvh_build.h"
#include "iris_device.h"
#include "iris_trace.h"
#include "iris_bake.h"
#include "iris_pt.h"
#include "iris_relight.h"
#include "iris_cache.h"
#include "iris_denoise.h"
#include "iris_metrics.h"
#include "iris_matmetrics.h"
#include "iris_validate.h"
#include "iris_texture.h"
#include "iris_atlas.h"
#include "iris_ngp.h"
#include "iris_prop.h"
#include "iris_loss.h"
#include "iris_crf.h"
#include "iris_render.h"
#include "iris_deflate.h"
#include "iris_png.h"
#include "iris_jpeg.h"
#include "iris_resize.h"
#include "iris_batch.h"
#include "iris_optim.h"
#include "iris_prebake.h"
#include "iris_labels.h"
#include "iris_closest.h"
#include "iris_texmat.h"

using namespace iris;

// ======================================================================================================
// error plumbing
// ======================================================================================================
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(IRIS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define API_BEGIN try {
#define API_END                                                                   \
    }                                                                             \
    catch (const std::exception& ex) { return fail(IRIS_ERR_BUILD, ex.what()); }  \
    catch (...) { return fail(IRIS_ERR_BUILD, "unknown C++ exception"); }

extern "C" IRIS_API const char* iris_last_error(void) { return g_err.c_str(); }

// One device allocation / one event, owned: handles hold these, so that a constructor's early return and iris_*_destroy free the same things.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    hipError_t upload(const void* host, size_t bytes) { return hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }     // into the allocation
};
struct DevEvent {
    hipEvent_t ev = nullptr;
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept { std::swap(ev, o.ev); return *this; }
    ~DevEvent() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
};

// ---- diagnostics options (iris_hip_debug.h): process-wide, set by tests / experiments only; -1 = the built-in default
static long long g_opt_bvh_tri_cost_x100 = -1, g_opt_bvh_max_leaf = -1, g_opt_phase_min = -1, g_opt_tile_target_rays = -1, g_opt_tiles_per_block = -1, g_opt_pt_tile_min = -1, g_opt_bvh_presplit_x10 = -1, g_opt_joint_max_rays = -1, g_opt_prop_bwd_targets = -1, g_opt_prop_lds_members = -1, g_opt_pool_combine = -1;
extern "C" IRIS_API int iris_debug_set(const char* key, long long value) {
    if (!key) return fail(IRIS_ERR_ARG, "iris_debug_set: null key");
    const std::string k(key);
    if (k == "bvh_max_leaf") g_opt_bvh_max_leaf = value;
    else if (k == "bvh_tri_cost_x100") g_opt_bvh_tri_cost_x100 = value;
    else if (k == "bvh_presplit_x10") g_opt_bvh_presplit_x10 = value;
    else if (k == "phase_min") g_opt_phase_min = value;
    else if (k == "tile_target_rays") g_opt_tile_target_rays = value;
    else if (k == "tiles_per_block") g_opt_tiles_per_block = value;
    else if (k == "pt_tile_min") g_opt_pt_tile_min = value;
    else if (k == "joint_max_rays") g_opt_joint_max_rays = value;
    else if (k == "prop_bwd_targets") g_opt_prop_bwd_targets = value;
    else if (k == "prop_lds_members") g_opt_prop_lds_members = value;
    else if (k == "pool_combine") g_opt_pool_combine = value;
    else return fail(IRIS_ERR_ARG, "iris_debug_set: unknown option " + k);
    return IRIS_OK;
}
extern "C" IRIS_API const char* iris_version(void) { return "iris_hip 0.1 (gfx950)"; }
#ifndef IRIS_NO_FUSED_RECORDS
#define IRIS_NO_FUSED_RECORDS 0      // (A/B: 1 = the bake kernels keep the plain leaf records and gather the emitter ordinal from its own table)
#endif
#ifndef IRIS_BUILD_FLAGS
#define IRIS_BUILD_FLAGS "unknown"
#endif
extern "C" IRIS_API const char* iris_debug_build_flags(void) { return IRIS_BUILD_FLAGS; }
#ifndef IRIS_SOURCE_HASH
#define IRIS_SOURCE_HASH "unknown"
#endif
extern "C" IRIS_API const char* iris_debug_source_hash(void) { return IRIS_SOURCE_HASH; }

// ======================================================================================================
// handles
// ======================================================================================================
static std::atomic<uint64_t> g_scene_uid{1};
struct iris_scene {
    int device = 0;
    uint64_t uid = g_scene_uid.fetch_add(1);    // identity of this scene for caches keyed on it (a pointer can be reused after iris_scene_destroy)
    SceneDev dev{};
    DevBuf d_nodes, d_tris;
    iris_scene_info info{};
};
struct iris_slf {
    int device = 0;
    SlfDev dev{};
    DevBuf d_inds, d_rad;
    int64_t kv = 0;
    iris_slf(int device_, int64_t kv_) : device(device_), kv(kv_) {}
    void bind(int H, double voxel_min, double voxel_max) {      // once both buffers are allocated
        dev.inds = (const int32_t*)d_inds.p; dev.radiance = (const float4*)d_rad.p; dev.H = H;
        dev.vmin = (float)voxel_min;
        dev.den = (float)(voxel_max - voxel_min);
    }
};
struct iris_emitter {
    int device = 0;
    EmitDev dev{};
    DevBuf d_ord, d_rad, d_area;
    DevBuf d_verts;            // (K,3,3) emitter_vertices   (sample_emitter only)
    DevBuf d_cdf;              // (K) emitter_cdf
    DevBuf d_ord2tri;          // (K) triangle index per emitter ordinal
    EmitSampleDev sample{};
    bool can_sample = false;
    int64_t n_rad = 0, k = 0;
    // Fused leaf records (round 5): the scene's leaf-record table with this emitter's ordinal of every triangle in the record's free fourth plane, so that the shading pass of
    // the bake kernels reads it from the line it fetches anyway.  Built on first use per scene (iris_bake_view), kept for the handle's life (at most two scenes).
    struct Fused { uint64_t scene_uid; DevBuf d_tris; DevEvent ready; bool done; };
    mutable std::mutex fused_mu;
    mutable std::vector<Fused> fused;
    mutable std::vector<Fused> retired;      // tables pushed out by a third scene: a launch that was handed one may still be on its way -- freed with the handle, never earlier
};

// Launches of the one-ray-per-lane kernels (iris_intersect, the path-tracing stages below their tiling threshold) of at most this many rays run in LATENCY MODE
// (iris_trace.h trace_q8_joint: node and triangle loads of an iteration issued together): they do not fill the chip, and what they wait for is their longest wave's
// dependent round trips.  iris_debug_set("joint_max_rays") overrides (0 = never).  Results do not depend on it.
constexpr long long kJointMaxRays = 1 << 20;
static bool joint_launch(int64_t n_rays) { return n_rays <= (g_opt_joint_max_rays >= 0 ? g_opt_joint_max_rays : kJointMaxRays); }

// The template arguments of a traversal kernel as a value: a launcher picks them once and hands them to the generic lambda that holds the launch (and its one argument list).
template <int LAYOUT, bool JOINT = false> struct TraceTag { static constexpr int layout = LAYOUT; static constexpr bool joint = JOINT; };
template <class F> static void with_layout(const SceneDev& sc, F&& f) {
    if (sc.layout == kLayoutQ8) f(TraceTag<kLayoutQ8>{});
    else f(TraceTag<kLayoutF32>{});
}
// the one-ray-per-lane kernels: <Q8, joint> for a small launch, else the plain kernel of the layout (there is no joint F32 traversal)
template <class F> static void with_trace(const SceneDev& sc, int64_t n_rays, F&& f) {
    if (sc.layout == kLayoutQ8 && joint_launch(n_rays)) f(TraceTag<kLayoutQ8, true>{});
    else with_layout(sc, f);
}
// the bake kernels: <specular, instrumented, layout>
template <bool SPEC, bool STATS, int LAYOUT> struct BakeTag { static constexpr bool spec = SPEC, stats = STATS; static constexpr int layout = LAYOUT; };
template <class F> static void with_bake(bool spec, bool stats, const SceneDev& sc, F&& f) {
    const bool q8 = sc.layout == kLayoutQ8;
    if (stats) {
        if (spec) { if (q8) f(BakeTag<true, true, kLayoutQ8>{}); else f(BakeTag<true, true, kLayoutF32>{}); }
        else      { if (q8) f(BakeTag<false, true, kLayoutQ8>{}); else f(BakeTag<false, true, kLayoutF32>{}); }
    } else {
        if (spec) { if (q8) f(BakeTag<true, false, kLayoutQ8>{}); else f(BakeTag<true, false, kLayoutF32>{}); }
        else      { if (q8) f(BakeTag<false, false, kLayoutQ8>{}); else f(BakeTag<false, false, kLayoutF32>{}); }
    }
}

static int grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}
// A plain grid-stride launch: 256-thread blocks, at most max_blocks of them, and the launch's error.
template <class... P, class... A>
static int launch1d(void (*kernel)(P...), int64_t n, int max_blocks, iris_stream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, args...);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
static int num_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}
// the grid of a one-ray-per-lane traversal launch (with_trace) over n rays: kBlock-thread workgroups, at most six per compute unit
static dim3 trace_grid(int64_t n) { return dim3(grid_for(n, kBlock, num_cus() * 6)); }

// ------------------------------------------------------------------------------------------------------
extern "C" IRIS_API int iris_scene_create(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, int device, iris_scene** out) {
    return iris_debug_scene_create(verts, nv, faces, nf, device, IRIS_BVH_DEFAULT, out);
}
extern "C" IRIS_API int iris_debug_scene_create(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, int device, int layout,
                                       iris_scene** out) {
    API_BEGIN
    if (!out || nv < 0 || nf < 0 || (nf > 0 && (!verts || !faces))) return fail(IRIS_ERR_ARG, "iris_scene_create: bad arguments");
    if (nf >= (1 << 26) - 1) return fail(IRIS_ERR_ARG, "iris_scene_create: more than 2^26 triangles (32-bit byte offsets into the 64-B records)");
    for (int64_t i = 0; i < nf * 3; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return fail(IRIS_ERR_ARG, "iris_scene_create: face index out of range");
    if (layout == IRIS_BVH_DEFAULT) layout = IRIS_BVH4_Q8;
    if (layout != IRIS_BVH4_F32 && layout != IRIS_BVH4_Q8) return fail(IRIS_ERR_ARG, "iris_scene_create: unknown BVH layout");
    if (!buildable_extent(verts, faces, nf))
        return fail(IRIS_ERR_ARG, "iris_scene_create: the area of the mesh's bounding box is not finite in float32 (coordinates too far apart for the SAH build)");
    HIP_TRY(hipSetDevice(device));
    auto t0 = std::chrono::steady_clock::now();
    int max_leaf = 4;
    if (g_opt_bvh_max_leaf > 0) max_leaf = (int)std::min<long long>(7, g_opt_bvh_max_leaf);   // iris_debug_set("bvh_max_leaf")
    const float tri_cost = g_opt_bvh_tri_cost_x100 > 0 ? (float)g_opt_bvh_tri_cost_x100 * 0.01f : 0.7f;   // iris_debug_set("bvh_tri_cost_x100")
    const float presplit = g_opt_bvh_presplit_x10 >= 0 ? (float)g_opt_bvh_presplit_x10 * 0.1f : 8.f;       // iris_debug_set("bvh_presplit_x10"); 0 = off
    WideBvh bvh = build_wide_bvh(verts, nv, faces, nf, 4, max_leaf, 2e-5f, tri_cost, presplit);
    if (bvh.tri_order.size() >= (size_t)(1 << 26) - 1) return fail(IRIS_ERR_BUILD, "iris_scene_create: more than 2^26 leaf records");
    if (3 * bvh.depth + 4 > kStackLds + kStackSpill) return fail(IRIS_ERR_BUILD, "iris_scene_create: BVH too deep for the traversal stack");
    if (layout == IRIS_BVH4_Q8 && bvh.nodes.size() * kNodeBytes * 8 >= ((size_t)1 << 32)) return fail(IRIS_ERR_BUILD, "iris_scene_create: the eight octant copies of the node table exceed 4 GiB (32-bit byte offsets)");

    const std::vector<float> nodes = encode_nodes(bvh, layout == IRIS_BVH4_Q8 ? kLayoutQ8 : kLayoutF32);      // bvh_build.h: the tables as the kernels read them
    if (nodes.empty()) return fail(IRIS_ERR_BUILD, "iris_scene_create: node quantisation failed");
    const std::vector<float> tris = encode_leaf_records(bvh, verts, faces);
    const size_t nn = bvh.nodes.size(), nt = bvh.tri_order.size();
    auto s = std::make_unique<iris_scene>();
    s->device = device;
    if (s->d_nodes.alloc(nodes.size() * 4) != hipSuccess || s->d_tris.alloc(tris.size() * 4) != hipSuccess ||
        s->d_nodes.upload(nodes.data(), nodes.size() * 4) != hipSuccess || s->d_tris.upload(tris.data(), tris.size() * 4) != hipSuccess)
        return fail(IRIS_ERR_HIP, "iris_scene_create: device allocation / upload failed");
    s->dev.nodes = (const float4*)s->d_nodes.p;
    s->dev.tris = (const float4*)s->d_tris.p;
    s->dev.n_nodes = (int)nn;
    s->dev.n_tris = (int)nt;
    s->dev.layout = layout == IRIS_BVH4_Q8 ? kLayoutQ8 : kLayoutF32;
    s->dev.oct_stride = layout == IRIS_BVH4_Q8 ? (uint32_t)(nn * kNodeBytes) : 0u;
    s->dev.phase_min = kPhaseMin;
    if (g_opt_phase_min >= 0) s->dev.phase_min = (int)g_opt_phase_min;  // iris_debug_set("phase_min") (results do not depend on it)
    s->info.n_vertices = nv; s->info.n_triangles = nf; s->info.layout = layout; s->info.n_nodes = (int32_t)nn;
    s->info.node_bytes = (int)(layout == IRIS_BVH4_Q8 ? kNodeBytes : kNodeBytesF32); s->info.tri_bytes = (int)kLeafRecordBytes; s->info.depth = bvh.depth;
    s->info.sah_cost = bvh.sah_cost; s->info.n_leaf_records = (int32_t)nt;
    s->info.build_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
    *out = s.release();
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API void iris_scene_destroy(iris_scene* s) { delete s; }
extern "C" IRIS_API int iris_scene_get_info(const iris_scene* s, iris_scene_info* out) {
    if (!s || !out) return fail(IRIS_ERR_ARG, "iris_scene_get_info: null");
    *out = s->info;
    return IRIS_OK;
}

extern "C" IRIS_API int iris_slf_create(const int64_t* inds, int H, const float* radiance, int64_t kv, double voxel_min, double voxel_max,
                               int device, iris_slf** out) {
    API_BEGIN
    if (!out || !inds || H <= 0 || H > 1024 || kv < 0 || (kv > 0 && !radiance)) return fail(IRIS_ERR_ARG, "iris_slf_create: bad arguments");
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)H * H * H;
    std::vector<int32_t> i32(n);
    for (size_t i = 0; i < n; ++i) {
        int64_t v = inds[i];
        if (v < -1 || v >= kv) return fail(IRIS_ERR_ARG, "iris_slf_create: inds entry out of range");
        i32[i] = (int32_t)v;
    }
    std::vector<float> rad((size_t)std::max<int64_t>(kv, 1) * 4, 0.f);
    for (int64_t i = 0; i < kv; ++i) { rad[i * 4] = radiance[i * 3]; rad[i * 4 + 1] = radiance[i * 3 + 1]; rad[i * 4 + 2] = radiance[i * 3 + 2]; }
    auto s = std::make_unique<iris_slf>(device, kv);
    HIP_TRY(s->d_inds.alloc(n * 4));
    HIP_TRY(s->d_rad.alloc(rad.size() * 4));
    HIP_TRY(s->d_inds.upload(i32.data(), n * 4));
    HIP_TRY(s->d_rad.upload(rad.data(), rad.size() * 4));
    s->bind(H, voxel_min, voxel_max);
    *out = s.release();
    return IRIS_OK;
    API_END
}
// The same from DEVICE buffers (the pre-bake stages build the grid on the GPU: slf_bake.py:116-118 constructs VoxelSLF from the occupancy mask it has
// just counted there): no 8 H^3-byte round trip through the host.  One 4-byte read-back reports an out-of-range entry.
__global__ void slf_inds_narrow_kernel(const int64_t* __restrict__ src, int32_t* __restrict__ dst, int64_t n, int64_t kv, int* __restrict__ bad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = src[i];
        if (v < -1 || v >= kv) *bad = 1;
        dst[i] = (int32_t)v;
    }
}
__global__ void pad_rows_kernel(const float* __restrict__ src, float4* __restrict__ dst, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = make_float4(src[i * 3], src[i * 3 + 1], src[i * 3 + 2], 0.f);
}
extern "C" IRIS_API int iris_slf_create_dev(const int64_t* inds_dev, int H, const float* radiance_dev, int64_t kv, double voxel_min, double voxel_max,
                                   int device, iris_slf** out, iris_stream_t stream) {
    API_BEGIN
    if (!out || !inds_dev || H <= 0 || H > 1024 || kv < 0 || (kv > 0 && !radiance_dev)) return fail(IRIS_ERR_ARG, "iris_slf_create_dev: bad arguments");
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)H * H * H;
    auto s = std::make_unique<iris_slf>(device, kv);
    DevBuf d_bad;
    if (s->d_inds.alloc(n * 4) != hipSuccess || s->d_rad.alloc((size_t)std::max<int64_t>(kv, 1) * 16) != hipSuccess || d_bad.alloc(4) != hipSuccess)
        return fail(IRIS_ERR_HIP, "iris_slf_create_dev: out of device memory");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(d_bad.p, 0, 4, st);
    (void)hipMemsetAsync(s->d_rad.p, 0, (size_t)std::max<int64_t>(kv, 1) * 16, st);
    hipLaunchKernelGGL(slf_inds_narrow_kernel, dim3(grid_for((int64_t)n, 256, 8192)), dim3(256), 0, st, inds_dev, (int32_t*)s->d_inds.p, (int64_t)n, kv, (int*)d_bad.p);
    if (kv > 0) hipLaunchKernelGGL(pad_rows_kernel, dim3(grid_for(kv, 256, 1024)), dim3(256), 0, st, radiance_dev, (float4*)s->d_rad.p, kv);
    int bad = 0;
    if (hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(IRIS_ERR_HIP, "iris_slf_create_dev: HIP error");
    if (bad) return fail(IRIS_ERR_ARG, "iris_slf_create_dev: inds entry out of range");
    s->bind(H, voxel_min, voxel_max);
    *out = s.release();
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API void iris_slf_destroy(iris_slf* s) { delete s; }

// ======================================================================================================
// NGPBRDF (model/brdf.py:213-260): hash-grid encoding + MLP, forward and parameter gradient
// ======================================================================================================
struct iris_ngp {
    int device = 0;
    NgpLevels lv{};
    DevBuf d_grid;              // half2 entries
    DevBuf d_w;                 // kNgpMlpParams halves
    DevBuf d_feat;              // [32 levels][kChunk] half2: the encoded features of one chunk of points
    float vmin = 0.f, den = 1.f;
    uint64_t n_entries = 0;
    // d_feat is the handle's ONE scratch buffer: forwards and backwards of one handle are serialised on the device -- a call on another stream than the previous
    // call's first waits (on the device, not the host) for the event that call recorded behind its last kernel; a parameter refresh (iris_ngp_set_params_dev
    // rewrites d_w / d_grid) is ordered the same way.  Host threads are serialised by the mutex.
    mutable std::mutex mu;
    mutable DevEvent last_use;
    mutable hipStream_t last_stream = nullptr;
    mutable bool used = false;
};
constexpr int kNgpChunk = 1 << 20;       // points per encode / MLP launch pair: 128 MiB of features
static uint64_t ngp_levels(NgpLevels& lv) {
    // tiny-cuda-nn GridEncoding: scale = exp2(level * log2(per_level_scale)) * base - 1, resolution = ceil(scale) + 1, entries = min(round_up(res^3, 8), 2^19)
    // (the library evaluates this in float with the device's fast exp2f, whose last bits are not reproducible; here every transcendental is taken in double
    //  and rounded to float once, so that any host libm gives the same table: log2(1.3f) -> float, level * that in float, exp2 -> float, * 16 - 1 in float)
    const float log2_scale = (float)log2((double)1.3f);
    uint64_t off = 0;
    for (int l = 0; l < kNgpLevels; ++l) {
        const float scale = (float)exp2((double)((float)l * log2_scale)) * 16.f - 1.0f;
        const uint32_t res = (uint32_t)ceilf(scale) + 1u;
        uint64_t n = (uint64_t)res * res * res;
        n = std::min<uint64_t>(n, 0xFFFFFFFFull / 2);
        n = (n + 7) / 8 * 8;
        n = std::min<uint64_t>(n, 1ull << 19);
        lv.scale[l] = scale; lv.res[l] = res; lv.size[l] = (uint32_t)n; lv.offset[l] = (uint32_t)off;
        off += n;
    }
    return off;
}
static uint16_t f32_to_f16_bits(float f) { _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }     // round to nearest even, as torch's .half()
extern "C" IRIS_API int64_t iris_ngp_n_params(void) {
    NgpLevels lv;
    return (int64_t)kNgpMlpParams + (int64_t)ngp_levels(lv) * 2;
}
extern "C" IRIS_API int iris_ngp_create(const float* params, int64_t n_params, double voxel_min, double voxel_max, int device, iris_ngp** out) {
    API_BEGIN
    if (!out) return fail(IRIS_ERR_ARG, "iris_ngp_create: bad arguments");
    HIP_TRY(hipSetDevice(device));              // (before anything is allocated: an invalid device leaves nothing behind)
    auto g = std::make_unique<iris_ngp>();
    g->device = device;
    g->n_entries = ngp_levels(g->lv);
    if (n_params != (int64_t)kNgpMlpParams + (int64_t)g->n_entries * 2)
        return fail(IRIS_ERR_ARG, "iris_ngp_create: mlp.params has " + std::to_string(n_params) + " entries, the NGPBRDF configuration has " + std::to_string(iris_ngp_n_params()));
    std::vector<uint16_t> h(params ? (size_t)n_params : 0);
    for (int64_t i = 0; params && i < n_params; ++i) h[(size_t)i] = f32_to_f16_bits(params[i]);
    if (g->d_w.alloc((size_t)kNgpMlpParams * 2) != hipSuccess || g->d_grid.alloc((size_t)g->n_entries * 4) != hipSuccess ||
        g->d_feat.alloc((size_t)kNgpLevels * kNgpChunk * 4) != hipSuccess)
        return fail(IRIS_ERR_HIP, "iris_ngp_create: out of device memory");
    if (g->last_use.create() != hipSuccess) return fail(IRIS_ERR_HIP, "iris_ngp_create: hipEventCreate failed");
    if (!params) {            // all-zero parameters: the caller's live on the device and arrive through iris_ngp_set_params_dev
        if (hipMemset(g->d_w.p, 0, (size_t)kNgpMlpParams * 2) != hipSuccess || hipMemset(g->d_grid.p, 0, (size_t)g->n_entries * 4) != hipSuccess)
            return fail(IRIS_ERR_HIP, "iris_ngp_create: hipMemset failed");
    } else if (g->d_w.upload(h.data(), (size_t)kNgpMlpParams * 2) != hipSuccess || g->d_grid.upload(h.data() + kNgpMlpParams, (size_t)g->n_entries * 4) != hipSuccess)
        return fail(IRIS_ERR_HIP, "iris_ngp_create: upload failed");
    g->vmin = (float)voxel_min;
    g->den = (float)(voxel_max - voxel_min);           // (the difference of the two python floats, taken in double, enters the float32 tensor arithmetic as one scalar)
    *out = g.release();
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API int iris_ngp_forward(const iris_ngp* g, const float* position, int64_t N, float* albedo, float* roughness, float* metallic, iris_stream_t stream) {
    API_BEGIN
    if (!g || N < 0 || (N > 0 && (!position || !albedo || !roughness || !metallic))) return fail(IRIS_ERR_ARG, "iris_ngp_forward: bad arguments");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) return IRIS_OK;
    std::lock_guard<std::mutex> lock(g->mu);
    if (g->used && g->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, g->last_use.ev, 0));      // the previous forward of this handle still owns d_feat
    NgpArgs a{};
    a.lv = g->lv; a.grid = (const uint32_t*)g->d_grid.p; a.w = (const _Float16*)g->d_w.p; a.pos = position; a.feat = (uint32_t*)g->d_feat.p;
    a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.n_chunk = kNgpChunk; a.vmin = g->vmin; a.den = g->den;
    for (int64_t n0 = 0; n0 < N; n0 += kNgpChunk) {          // (stream-ordered: the feature planes of a chunk are consumed before the next chunk's encode overwrites them)
        a.n0 = n0; a.n = (int)std::min<int64_t>(kNgpChunk, N - n0);
        hipLaunchKernelGGL(ngp_encode_kernel, dim3((a.n + 255) / 256, kNgpLevels), dim3(256), 0, st, a);
        const int tiles = (a.n + 31) / 32;
        hipLaunchKernelGGL(ngp_mlp_kernel, dim3(std::min(std::max((tiles + 3) / 4, 1), 2048)), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->last_use.ev, st));
    g->last_stream = st; g->used = true;
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API int iris_ngp_set_params_dev(iris_ngp* g, const float* params_dev, int64_t n_params, iris_stream_t stream) {
    API_BEGIN
    if (!g || !params_dev) return fail(IRIS_ERR_ARG, "iris_ngp_set_params_dev: bad arguments");
    if (n_params != (int64_t)kNgpMlpParams + (int64_t)g->n_entries * 2)
        return fail(IRIS_ERR_ARG, "iris_ngp_set_params_dev: mlp.params has " + std::to_string(n_params) + " entries, the NGPBRDF configuration has " + std::to_string(iris_ngp_n_params()));
    if ((uintptr_t)params_dev % 16) return fail(IRIS_ERR_ARG, "iris_ngp_set_params_dev: params_dev must be 16-byte aligned");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g->mu);
    if (g->used && g->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, g->last_use.ev, 0));      // a forward in flight on another stream still reads the old parameters
    const int64_t n8 = n_params / 8;
    hipLaunchKernelGGL(ngp_params_cast_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const float4*)params_dev, n8, (_Float16*)g->d_w.p, (_Float16*)g->d_grid.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->last_use.ev, st));
    g->last_stream = st; g->used = true;
    return IRIS_OK;
    API_END
}
// ---- the optimizer step (iris_optim.h): torch.optim.Adam's arithmetic, the scalars formed in double and rounded to float once
static int adam_scalars(const char* who, int64_t n, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, AdamScalars& s) {
    const std::string w(who);
    if (n < 0) return fail(IRIS_ERR_ARG, w + ": n must not be negative");
    if (step < 1) return fail(IRIS_ERR_ARG, w + ": step counts from 1 (got " + std::to_string(step) + ")");
    if (!std::isfinite(lr) || !(lr > 0.0)) return fail(IRIS_ERR_ARG, w + ": lr must be positive and finite");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(IRIS_ERR_ARG, w + ": eps must be positive and finite");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(IRIS_ERR_ARG, w + ": the betas must lie in [0, 1)");
    if (!std::isfinite(weight_decay) || !(weight_decay >= 0.0)) return fail(IRIS_ERR_ARG, w + ": weight_decay must be finite and not negative");
    s.w1 = (float)(1.0 - beta1);
    s.w2 = (float)(1.0 - beta2);
    s.beta2 = (float)beta2;
    s.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)step)));
    s.bc2 = (float)std::sqrt(1.0 - std::pow(beta2, (double)step));
    s.eps = (float)eps;
    s.wd = (float)weight_decay;
    return IRIS_OK;
}
extern "C" IRIS_API int iris_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step, double lr, double beta1,
                                       double beta2, double eps, double weight_decay, iris_stream_t stream) {
    API_BEGIN
    AdamScalars s{};
    if (int rc = adam_scalars("iris_adam_step", n, step, lr, beta1, beta2, eps, weight_decay, s)) return rc;
    if (n == 0) return IRIS_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(IRIS_ERR_ARG, "iris_adam_step: null pointer");
    const uintptr_t bits = (uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
    if (bits % 4) return fail(IRIS_ERR_ARG, "iris_adam_step: the buffers must be 4-byte aligned");
    const int64_t n4 = bits % 16 ? 0 : n / 4;            // the 16-byte body; the scalar kernel takes the rest (everything when a buffer is not 16-byte aligned)
    if (n4 > 0)
        if (int rc = launch1d(adam_vec4_kernel, n4, 2048, stream, (float4*)param, (const float4*)grad, (float4*)exp_avg, (float4*)exp_avg_sq, n4, s)) return rc;
    if (n4 * 4 < n)
        if (int rc = launch1d(adam_scalar_kernel, n - n4 * 4, 2048, stream, param, grad, exp_avg, exp_avg_sq, n4 * 4, n, s)) return rc;
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API int iris_ngp_adam_step(iris_ngp* g, float* params_dev, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_params, int64_t step,
                                           double lr, double beta1, double beta2, double eps, double weight_decay, iris_stream_t stream) {
    API_BEGIN
    if (!g || !params_dev || !grad || !exp_avg || !exp_avg_sq) return fail(IRIS_ERR_ARG, "iris_ngp_adam_step: bad arguments");
    if (n_params != (int64_t)kNgpMlpParams + (int64_t)g->n_entries * 2)
        return fail(IRIS_ERR_ARG, "iris_ngp_adam_step: mlp.params has " + std::to_string(n_params) + " entries, the NGPBRDF configuration has " + std::to_string(iris_ngp_n_params()));
    AdamScalars s{};
    if (int rc = adam_scalars("iris_ngp_adam_step", n_params, step, lr, beta1, beta2, eps, weight_decay, s)) return rc;
    if (((uintptr_t)params_dev | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16)
        return fail(IRIS_ERR_ARG, "iris_ngp_adam_step: params_dev, grad, exp_avg and exp_avg_sq must be 16-byte aligned");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g->mu);
    if (g->used && g->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, g->last_use.ev, 0));      // a forward in flight on another stream still reads the old half copy
    const int64_t n8 = n_params / 8;
    if (int rc = launch1d(ngp_adam_kernel, n8, 2048, stream, (float4*)params_dev, (const float4*)grad, (float4*)exp_avg, (float4*)exp_avg_sq, n8, s,
                          (_Float16*)g->d_w.p, (_Float16*)g->d_grid.p)) return rc;
    HIP_TRY(hipEventRecord(g->last_use.ev, st));
    g->last_stream = st; g->used = true;
    return IRIS_OK;
    API_END
}
static int64_t ngp_bwd_plane(int64_t N) { return std::min<int64_t>((std::max<int64_t>(N, 1) + 63) / 64 * 64, kNgpChunk); }
extern "C" IRIS_API uint64_t iris_ngp_backward_workspace_bytes(int64_t N) {
    // dX planes [32 levels][min(N, chunk)] float2 + one weight-gradient slab per workgroup of ngp_mlp_bwd_kernel
    return (uint64_t)kNgpLevels * (uint64_t)ngp_bwd_plane(N) * 8 + (uint64_t)kNgpBwdMaxGroups * kNgpMlpParams * 4;
}
extern "C" IRIS_API int iris_ngp_backward(const iris_ngp* g, const float* position, int64_t N, const float* g_albedo, const float* g_roughness, const float* g_metallic,
                                          float loss_scale, float* grad_params, void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    API_BEGIN
    if (!g || N < 0 || (N > 0 && (!position || !g_albedo || !g_roughness || !g_metallic || !grad_params || !workspace))) return fail(IRIS_ERR_ARG, "iris_ngp_backward: bad arguments");
    if (!(loss_scale > 0.f) || !std::isfinite(loss_scale)) return fail(IRIS_ERR_ARG, "iris_ngp_backward: loss_scale must be positive and finite");
    if (N == 0) return IRIS_OK;
    if (workspace_bytes < iris_ngp_backward_workspace_bytes(N))
        return fail(IRIS_ERR_ARG, "iris_ngp_backward: workspace has " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(N) + " points need " + std::to_string(iris_ngp_backward_workspace_bytes(N)));
    if ((uintptr_t)workspace % 16) return fail(IRIS_ERR_ARG, "iris_ngp_backward: workspace must be 16-byte aligned");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g->mu);
    if (g->used && g->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, g->last_use.ev, 0));      // the previous call of this handle still owns d_feat
    NgpBwdArgs b{};
    NgpArgs& a = b.f;
    a.lv = g->lv; a.grid = (const uint32_t*)g->d_grid.p; a.w = (const _Float16*)g->d_w.p; a.pos = position; a.feat = (uint32_t*)g->d_feat.p;
    a.n_chunk = kNgpChunk; a.vmin = g->vmin; a.den = g->den;
    b.g_albedo = g_albedo; b.g_rough = g_roughness; b.g_metal = g_metallic;
    b.n_plane = (int)ngp_bwd_plane(N);
    b.dx = (float2*)workspace;
    b.slabs = (float*)((char*)workspace + (size_t)kNgpLevels * b.n_plane * 8);
    b.grad = grad_params; b.loss_scale = loss_scale; b.inv_scale = 1.0f / loss_scale;
    for (int64_t n0 = 0; n0 < N; n0 += kNgpChunk) {          // (stream-ordered, as the forward: a chunk's planes and slabs are consumed before the next chunk overwrites them)
        a.n0 = n0; a.n = (int)std::min<int64_t>(kNgpChunk, N - n0);
        const int tiles = (a.n + 31) / 32;
        b.n_slabs = std::min(std::max((tiles + 3) / 4, 1), kNgpBwdMaxGroups);
        hipLaunchKernelGGL(ngp_encode_kernel, dim3((a.n + 255) / 256, kNgpLevels), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ngp_mlp_bwd_kernel, dim3(b.n_slabs), dim3(256), 0, st, b);
        hipLaunchKernelGGL(ngp_wgrad_reduce_kernel, dim3(kNgpMlpParams / 256), dim3(256), 0, st, b);
        hipLaunchKernelGGL(ngp_grid_bwd_kernel, dim3((a.n + 255) / 256, kNgpLevels), dim3(256), 0, st, b);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->last_use.ev, st));
    g->last_stream = st; g->used = true;
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API int iris_debug_ngp_encode(const iris_ngp* g, const float* position, int64_t N, uint32_t* feat, iris_stream_t stream) {
    API_BEGIN
    if (!g || N < 0 || N > kNgpChunk || (N > 0 && (!position || !feat))) return fail(IRIS_ERR_ARG, "iris_debug_ngp_encode: bad arguments");
    if (N == 0) return IRIS_OK;
    HIP_TRY(hipSetDevice(g->device));
    NgpArgs a{};
    a.lv = g->lv; a.grid = (const uint32_t*)g->d_grid.p; a.w = (const _Float16*)g->d_w.p; a.pos = position; a.feat = feat;
    a.n_chunk = (int)N; a.vmin = g->vmin; a.den = g->den; a.n0 = 0; a.n = (int)N;
    hipLaunchKernelGGL(ngp_encode_kernel, dim3((a.n + 255) / 256, kNgpLevels), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API void iris_ngp_destroy(iris_ngp* g) { delete g; }

extern "C" IRIS_API int iris_emitter_create(const uint8_t* is_emitter, int64_t nf, const float* radiance, int64_t n_rad, const float* area,
                                   int64_t k, const float* verts, const float* cdf, int device, iris_emitter** out) {
    API_BEGIN
    if (!out || nf < 0 || k < 0 || n_rad < 0 || (nf > 0 && !is_emitter)) return fail(IRIS_ERR_ARG, "iris_emitter_create: bad arguments");
    HIP_TRY(hipSetDevice(device));
    std::vector<int32_t> ord((size_t)std::max<int64_t>(nf, 1), -1);
    int64_t c = 0;
    for (int64_t i = 0; i < nf; ++i) ord[(size_t)i] = is_emitter[i] ? (int32_t)c++ : -1;
    if (c != k) return fail(IRIS_ERR_ARG, "iris_emitter_create: is_emitter.sum() != len(emitter_area)");
    if (c > n_rad) return fail(IRIS_ERR_ARG, "iris_emitter_create: radiance has fewer rows than emitters");
    std::vector<float> rad((size_t)std::max<int64_t>(n_rad, 1) * 4, 0.f);
    for (int64_t i = 0; i < n_rad; ++i) { rad[i * 4] = radiance[i * 3]; rad[i * 4 + 1] = radiance[i * 3 + 1]; rad[i * 4 + 2] = radiance[i * 3 + 2]; }
    auto e = std::make_unique<iris_emitter>();
    e->device = device; e->n_rad = n_rad; e->k = k;
    HIP_TRY(e->d_ord.alloc(ord.size() * 4));
    HIP_TRY(e->d_rad.alloc(rad.size() * 4));
    HIP_TRY(e->d_area.alloc((size_t)std::max<int64_t>(k, 1) * 4));
    HIP_TRY(e->d_ord.upload(ord.data(), ord.size() * 4));
    HIP_TRY(e->d_rad.upload(rad.data(), rad.size() * 4));
    if (k > 0) HIP_TRY(e->d_area.upload(area, (size_t)k * 4));
    e->dev.emit_ord = (const int32_t*)e->d_ord.p; e->dev.radiance = (const float4*)e->d_rad.p; e->dev.area = (const float*)e->d_area.p;
    e->dev.nf = nf;
    float kf = (float)k; if (kf < 1e-12f) kf = 1e-12f;  // NF.normalize(ones(k), p=1)
    e->dev.emitter_pdf = 1.0f / kf;
    if (verts && cdf && k > 0) {                          // tables of sample_emitter (model/emitter.py:224-255)
        std::vector<int32_t> o2t((size_t)k);
        for (int64_t i = 0; i < nf; ++i) if (ord[(size_t)i] >= 0) o2t[(size_t)ord[(size_t)i]] = (int32_t)i;
        HIP_TRY(e->d_verts.alloc((size_t)k * 36));
        HIP_TRY(e->d_cdf.alloc((size_t)k * 4));
        HIP_TRY(e->d_ord2tri.alloc((size_t)k * 4));
        HIP_TRY(e->d_verts.upload(verts, (size_t)k * 36));
        HIP_TRY(e->d_cdf.upload(cdf, (size_t)k * 4));
        HIP_TRY(e->d_ord2tri.upload(o2t.data(), (size_t)k * 4));
        e->sample.cdf = (const float*)e->d_cdf.p; e->sample.verts = (const float*)e->d_verts.p; e->sample.area = (const float*)e->d_area.p;
        e->sample.ord2tri = (const int32_t*)e->d_ord2tri.p; e->sample.k = k; e->sample.emitter_pdf = e->dev.emitter_pdf;
        e->can_sample = true;
    }
    *out = e.release();
    return IRIS_OK;
    API_END
}
extern "C" IRIS_API void iris_emitter_destroy(iris_emitter* e) { delete e; }      // (the fused and the retired tables go with it)

extern "C" IRIS_API int iris_slf_set_radiance(iris_slf* s, const float* radiance_dev, int64_t kv, iris_stream_t stream) {
    if (!s || kv != s->kv || (kv > 0 && !radiance_dev)) return fail(IRIS_ERR_ARG, "iris_slf_set_radiance: bad arguments");
    if (kv == 0) return IRIS_OK;
    return launch1d(pad_rows_kernel, kv, 1024, stream, radiance_dev, (float4*)s->d_rad.p, kv);
}
extern "C" IRIS_API int iris_emitter_set_radiance(iris_emitter* e, const float* radiance_dev, int64_t n_rad, iris_stream_t stream) {
    if (!e || !radiance_dev || n_rad != e->n_rad) return fail(IRIS_ERR_ARG, "iris_emitter_set_radiance: bad arguments");
    return launch1d(pad_rows_kernel, n_rad, 1024, stream, radiance_dev, (float4*)e->d_rad.p, n_rad);
}

// ======================================================================================================
// a1 ray generation
// ======================================================================================================
struct RaygenArgs { float K[9]; float c2w[12]; float focal; int H, W, ray_diff, synthetic; };

__global__ void raygen_kernel(RaygenArgs a, float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ dxdu,
                              float* __restrict__ dydv) {
    const int64_t n = (int64_t)a.H * a.W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
        const PixelRay r = raygen_pixel(a.K, a.c2w, a.focal, a.H, a.W, a.ray_diff, a.synthetic, x, y);      // iris_batch.h: shared with pixel_batch_kernel
        st3(rays_o + i * 3, r.o);
        st3(rays_d + i * 3, r.d);
        if (a.ray_diff) {
            st3(dxdu + i * 3, r.dxdu);
            st3(dydv + i * 3, r.dydv);
        }
    }
}
static int raygen_launch(RaygenArgs a, float* o, float* d, float* dx, float* dy, iris_stream_t stream) {
    if (a.H <= 0 || a.W <= 0 || !o || !d || (a.ray_diff && (!dx || !dy))) return fail(IRIS_ERR_ARG, "iris_raygen: bad arguments");
    return launch1d(raygen_kernel, (int64_t)a.H * a.W, 4096, stream, a, o, d, dx, dy);
}
extern "C" IRIS_API int iris_raygen_real(const float K[9], const float c2w[12], int H, int W, int ray_diff, float* rays_o, float* rays_d,
                                float* dxdu, float* dydv, iris_stream_t stream) {
    if (!K || !c2w) return fail(IRIS_ERR_ARG, "iris_raygen_real: null K/c2w");
    RaygenArgs a{};
    std::memcpy(a.K, K, 36); std::memcpy(a.c2w, c2w, 48);
    a.H = H; a.W = W; a.ray_diff = ray_diff; a.synthetic = 0; a.focal = 1.f;
    return raygen_launch(a, rays_o, rays_d, dxdu, dydv, stream);
}
extern "C" IRIS_API int iris_raygen_synthetic(float focal, const float c2w[12], int H, int W, int ray_diff, float* rays_o, float* rays_d,
                                     float* dxdu, float* dydv, iris_stream_t stream) {
    if (!c2w) return fail(IRIS_ERR_ARG, "iris_raygen_synthetic: null c2w");
    RaygenArgs a{};
    std::memcpy(a.c2w, c2w, 48);
    a.H = H; a.W = W; a.ray_diff = ray_diff; a.synthetic = 1; a.focal = focal;
    return raygen_launch(a, rays_o, rays_d, dxdu, dydv, stream);
}

// 5c-9: the trainers' pixel batch (iris_batch.h)
extern "C" IRIS_API int iris_pixel_batch(const int64_t* ids, int64_t B, const float* cameras, int64_t V, int H, int W, int ray_diff, int synthetic,
                                const void* rgb, int rgb_is_u8, const void* int_albedo, int int_albedo_is_u8, const int32_t* segmentation,
                                const float* positions, const float* exposure, float* out_rays, float* out_rgbs, float* out_int_albedo,
                                int64_t* out_segmentation, float* out_exposure, float* out_positions, iris_stream_t stream) {
    if (B < 0 || V <= 0 || H <= 0 || W <= 0 || !cameras) return fail(IRIS_ERR_ARG, "iris_pixel_batch: bad arguments");
    if ((out_rgbs && !rgb) || (out_int_albedo && !int_albedo) || (out_segmentation && !segmentation) || (out_exposure && !exposure) ||
        (out_positions && !positions))
        return fail(IRIS_ERR_ARG, "iris_pixel_batch: an output was asked for whose store is NULL");
    if (B == 0) return IRIS_OK;
    if (!ids) return fail(IRIS_ERR_ARG, "iris_pixel_batch: null ids");
    PixelBatchArgs a{};
    a.ids = ids; a.B = B; a.cameras = cameras; a.V = V;
    a.H = H; a.W = W; a.ray_diff = ray_diff != 0; a.synthetic = synthetic != 0;
    a.rgb = rgb; a.albedo = int_albedo; a.rgb_u8 = rgb_is_u8 != 0; a.albedo_u8 = int_albedo_is_u8 != 0;
    a.segmentation = segmentation; a.positions = positions; a.exposure = exposure;
    a.o_rays = out_rays; a.o_rgbs = out_rgbs; a.o_albedo = out_int_albedo; a.o_segmentation = out_segmentation; a.o_exposure = out_exposure;
    a.o_positions = out_positions;
    return launch1d(pixel_batch_kernel, B, 4096, stream, a);
}

// ======================================================================================================
// a2 ray_intersect
// ======================================================================================================
template <int LAYOUT, bool JOINT = false>
__global__ __launch_bounds__(kBlock) void intersect_kernel(SceneDev sc, const float* __restrict__ xs, const float* __restrict__ ds,
                                                           int64_t B, float* __restrict__ pos, float* __restrict__ nrm,
                                                           float* __restrict__ uv, int64_t* __restrict__ idx, uint8_t* __restrict__ valid) {
    __shared__ uint32_t s_stack[kStackLds * kBlock];
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < B; i += (int64_t)gridDim.x * kBlock) {
        f3 o = ld3(xs + i * 3), d = ld3(ds + i * 3);
        Hit h = trace_bvh4<LAYOUT, false, kStackLds, false, JOINT>(sc, o, d, s_stack + threadIdx.x);
        if (h.slot >= 0) {
            f3 p0, p1, p2;
            hit_vertices(sc, h, p0, p1, p2);
            if (pos) st3(pos + i * 3, hit_position(h, p0, p1, p2));
            if (nrm) {
                f3 n = t_normalize(hit_normal(p0, p1, p2));                    // NF.normalize(ret.n)
                if (t_dot(n, mk3(-d.x, -d.y, -d.z)) < 0.f) n = mk3(-n.x, -n.y, -n.z);  // double_sided(-ds, normals)
                st3(nrm + i * 3, n);
            }
            if (uv) { uv[i * 2] = h.u; uv[i * 2 + 1] = h.v; }
            if (idx) idx[i] = h.id;
            if (valid) valid[i] = 1;
        } else {
            if (pos) st3(pos + i * 3, mk3(0.f, 0.f, 0.f));
            if (nrm) st3(nrm + i * 3, mk3(0.f, 0.f, 0.f));
            if (uv) { uv[i * 2] = 0.f; uv[i * 2 + 1] = 0.f; }
            if (idx) idx[i] = -1;
            if (valid) valid[i] = 0;
        }
    }
}
extern "C" IRIS_API int iris_intersect(const iris_scene* s, const float* xs, const float* ds, int64_t B, float* pos, float* nrm, float* uv,
                              int64_t* idx, uint8_t* valid, iris_stream_t stream) {
    if (!s || B < 0 || (B > 0 && (!xs || !ds))) return fail(IRIS_ERR_ARG, "iris_intersect: bad arguments");
    if (B == 0) return IRIS_OK;
    with_trace(s->dev, B, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((intersect_kernel<T::layout, T::joint>), trace_grid(B), dim3(kBlock), 0, (hipStream_t)stream, s->dev, xs, ds, B,
                           pos, nrm, uv, idx, valid);
    });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// a3/a4 samplers, a5 lookups, a10 lerp (unfused entry points of the call surface)
// ======================================================================================================
__global__ void sample_diffuse_kernel(const float* __restrict__ u2, const float* __restrict__ normal, int64_t B, float* __restrict__ wi,
                                      float* __restrict__ pdf, float* __restrict__ weight) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        f3 n = ld3(normal + i * 3), t, b;
        normal_space(n, t, b);
        f3 d = diffuse_sampler(u2[i * 2], u2[i * 2 + 1], n, t, b);
        st3(wi + i * 3, d);
        if (pdf) pdf[i] = relu(t_dot(n, d)) / kPi;
        if (weight) st3(weight + i * 3, mk3(1.f, 1.f, 1.f));
    }
}
extern "C" IRIS_API int iris_sample_diffuse(const float* u2, const float* normal, int64_t B, float* wi, float* pdf, float* weight,
                                   iris_stream_t stream) {
    if (B < 0 || (B > 0 && (!u2 || !normal || !wi))) return fail(IRIS_ERR_ARG, "iris_sample_diffuse: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(sample_diffuse_kernel, B, 8192, stream, u2, normal, B, wi, pdf, weight);
}

__global__ void sample_specular_kernel(const float* __restrict__ u2, const float* __restrict__ wo, const float* __restrict__ normal,
                                       float rough_all, const float* __restrict__ rough_each, int64_t B, float* __restrict__ wi, float* __restrict__ pdf,
                                       float* __restrict__ w0, float* __restrict__ w1) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        f3 n = ld3(normal + i * 3), o = ld3(wo + i * 3), t, b;
        const float rough = rough_each ? rough_each[i] : rough_all;
        normal_space(n, t, b);
        f3 d = specular_sampler(u2[i * 2], u2[i * 2 + 1], rough, o, n, t, b);
        SpecW w = specular_weights(d, o, n, rough, pdf != nullptr);
        st3(wi + i * 3, d);
        if (pdf) pdf[i] = w.pdf;
        if (w0) w0[i] = w.g0;
        if (w1) w1[i] = w.g1;
    }
}
extern "C" IRIS_API int iris_sample_specular(const float* u2, const float* wo, const float* normal, float roughness, int64_t B, float* wi,
                                    float* pdf, float* w0, float* w1, iris_stream_t stream) {
    if (B < 0 || (B > 0 && (!u2 || !wo || !normal || !wi))) return fail(IRIS_ERR_ARG, "iris_sample_specular: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(sample_specular_kernel, B, 8192, stream, u2, wo, normal, roughness,
                       (const float*)nullptr, B, wi, pdf, w0, w1);
}
extern "C" IRIS_API int iris_sample_specular_v(const float* u2, const float* wo, const float* normal, const float* roughness, int64_t B, float* wi,
                                      float* pdf, float* w0, float* w1, iris_stream_t stream) {
    if (B < 0 || (B > 0 && (!u2 || !wo || !normal || !roughness || !wi))) return fail(IRIS_ERR_ARG, "iris_sample_specular_v: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(sample_specular_kernel, B, 8192, stream, u2, wo, normal, 0.f, roughness, B,
                       wi, pdf, w0, w1);
}

__global__ void slf_lookup_kernel(SlfDev s, const float* __restrict__ x, int64_t B, int64_t* __restrict__ idx, float* __restrict__ rgb) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        f3 p = ld3(x + i * 3);
        int j = slf_index(s, p);
        if (idx) idx[i] = j;
        if (rgb) {
            f3 r = mk3(0.f, 0.f, 0.f);
            if (j >= 0) { float4 q = s.radiance[j]; r = mk3(q.x, q.y, q.z); }
            st3(rgb + i * 3, r);
        }
    }
}
extern "C" IRIS_API int iris_slf_lookup(const iris_slf* s, const float* x, int64_t B, int64_t* idx, float* rgb, iris_stream_t stream) {
    if (!s || B < 0 || (B > 0 && !x)) return fail(IRIS_ERR_ARG, "iris_slf_lookup: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(slf_lookup_kernel, B, 8192, stream, s->dev, x, B, idx, rgb);
}

__global__ void eval_emitter_kernel(EmitDev e, SlfDev s, const float* __restrict__ pos, const int64_t* __restrict__ tri,
                                    const float* __restrict__ rough, float trace_rough, int64_t B, float* __restrict__ Le,
                                    float* __restrict__ emit_pdf, uint8_t* __restrict__ valid_next) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        float pdf; bool vn;
        f3 l = eval_emitter1(e, s, ld3(pos + i * 3), tri[i], rough != nullptr, rough ? rough[i] : 0.f, trace_rough, pdf, vn);
        st3(Le + i * 3, l);
        if (emit_pdf) emit_pdf[i] = pdf;
        if (valid_next) valid_next[i] = vn ? 1 : 0;
    }
}
extern "C" IRIS_API int iris_eval_emitter(const iris_emitter* e, const iris_slf* s, const float* position, const int64_t* triangle_idx,
                                 const float* roughness, float trace_roughness, int64_t B, float* Le, float* emit_pdf,
                                 uint8_t* valid_next, iris_stream_t stream) {
    // (no radiance cache is consulted without a roughness array, or with trace_roughness = +inf: the cache may be NULL then -- AreaEmitter has none)
    const bool slf_unreachable = !roughness || (std::isinf(trace_roughness) && trace_roughness > 0.f);
    if (!e || (!s && !slf_unreachable) || B < 0 || (B > 0 && (!position || !triangle_idx || !Le))) return fail(IRIS_ERR_ARG, "iris_eval_emitter: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(eval_emitter_kernel, B, 8192, stream, e->dev, s ? s->dev : SlfDev{}, position,
                       triangle_idx, roughness, trace_roughness, B, Le, emit_pdf, valid_next);
}

__global__ void lerp_specular_kernel(const float* __restrict__ spec, const float* __restrict__ rough, int64_t B, int R, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        float r = (rough[i] - 0.02f) / (float)(1.0 - 0.02) * (float)(R - 1);
        int r1 = min(max((int)ceilf(r), 0), R - 1), r0 = min(max((int)floorf(r), 0), R - 1);
        float w = r - floorf(r);
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = spec[(i * R + r0) * 3 + c] * (1.f - w) + spec[(i * R + r1) * 3 + c] * w;
    }
}
extern "C" IRIS_API int iris_lerp_specular(const float* specular, const float* roughness, int64_t B, int R, float* out, iris_stream_t stream) {
    if (B < 0 || R < 1 || (B > 0 && (!specular || !roughness || !out))) return fail(IRIS_ERR_ARG, "iris_lerp_specular: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(lerp_specular_kernel, B, 8192, stream, specular, roughness, B, R, out);
}

// ---- multi-GPU: the gathered stripes of a view back into image order (iris_amd/sharding.py; the reference is single-GPU, bake_shading.py:41).
// gathered[r][m][j] is map m of rank r at its j-th local pixel (the rank's rows -- stripe s of `stripe` rows belongs to rank s % world -- in
// ascending order, row-major); full[m][row * W + col].  Pure index arithmetic: no index tensors, one pass, reads and writes coalesced along a row.
__global__ void unstripe_maps_kernel(const float* __restrict__ gathered, int world, int M, int64_t n_max, int H, int W, int stripe, float* __restrict__ full) {
    const int64_t n_px = (int64_t)H * W, total = n_px * M * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / (n_px * 3), rem = i - m * n_px * 3, p = rem / 3;
        const int c = (int)(rem - p * 3);
        const int row = (int)(p / W), col = (int)(p - (int64_t)row * W);
        const int s = row / stripe, r = s % world;
        const int64_t j = ((int64_t)(s / world) * stripe + (row - s * stripe)) * W + col;
        full[i] = gathered[(((int64_t)r * M + m) * n_max + j) * 3 + c];
    }
}
extern "C" IRIS_API int iris_unstripe_maps(const float* gathered, int world, int n_maps, int64_t n_max, int H, int W, int stripe_rows, float* full, iris_stream_t stream) {
    if (world < 1 || n_maps < 0 || H < 0 || W < 0 || stripe_rows < 1 || n_max < 0) return fail(IRIS_ERR_ARG, "iris_unstripe_maps: bad arguments");
    // the largest share of a rank: rank 0 owns stripes 0, world, 2 world, ...
    const int n_stripes = (H + stripe_rows - 1) / stripe_rows;
    int64_t rows0 = 0;
    for (int s = 0; s < n_stripes; s += world) rows0 += std::min(stripe_rows, H - s * stripe_rows);
    if (n_max < rows0 * W) return fail(IRIS_ERR_ARG, "iris_unstripe_maps: n_max is smaller than the largest rank's pixel count");
    const int64_t total = (int64_t)H * W * n_maps * 3;
    if (total == 0) return IRIS_OK;
    if (!gathered || !full) return fail(IRIS_ERR_ARG, "iris_unstripe_maps: null pointer");
    return launch1d(unstripe_maps_kernel, total, 16384, stream, gathered, world, n_maps, n_max, H, W, stripe_rows, full);
}

// ---- the small helpers of utils/ops.py as calls of their own (inside the bake / path-tracing kernels the same device functions are fused)
__global__ void normal_space_kernel(const float* normal, int64_t B, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const f3 n = ld3(normal + i * 3);
        f3 t, b;
        normal_space(n, t, b);
        float* o = out + i * 9;                    // (B,3,3)[i][row][col], columns tangent, bitangent, normal
        o[0] = t.x; o[1] = b.x; o[2] = n.x; o[3] = t.y; o[4] = b.y; o[5] = n.y; o[6] = t.z; o[7] = b.z; o[8] = n.z;
    }
}
__global__ void double_sided_kernel(const float* V, float* N, int64_t B) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const f3 v = ld3(V + i * 3), n = ld3(N + i * 3);
        if (t_dot(n, v) < 0.f) st3(N + i * 3, mk3(-n.x, -n.y, -n.z));
    }
}
__global__ void angle2xyz_kernel(const float* theta, const float* phi, int64_t B, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const float st = sinf(theta[i]), ct = cosf(theta[i]), sp = sinf(phi[i]), cp = cosf(phi[i]);
        st3(out + i * 3, t_normalize(mk3(st * cp, st * sp, ct)));
    }
}
// op 0: D_GGX(a = cos_h, b = eta)   1: G1_GGX_Schlick(a = NoV, b = eta)   2: G_Smith(a = NoV, b = NoL, c = eta)
//    3: fresnelSchlick(a = VoH, b = F0)   4: fresnelSchlick_sep(a = VoH) -> out = 1 - x, out2 = x      (x = (1 - VoH)^5)
__global__ void ggx_terms_kernel(int op, const float* a, const float* b, const float* c, int64_t B, float* out, float* out2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = a[i];
        if (op == 0) out[i] = D_GGX(x, b[i]);
        else if (op == 1) out[i] = G1_GGX_Schlick(x, b[i]);
        else if (op == 2) out[i] = G1_GGX_Schlick(b[i], c[i]) * G1_GGX_Schlick(x, c[i]);
        else {
            const float y = 1.f - x, y2 = y * y, p5 = y2 * y2 * y;
            if (op == 3) out[i] = b[i] + (1.f - b[i]) * p5;
            else { out[i] = 1.f - p5; out2[i] = p5; }
        }
    }
}
extern "C" IRIS_API int iris_get_normal_space(const float* normal, int64_t B, float* out, iris_stream_t stream) {
    if (B < 0 || (B > 0 && (!normal || !out))) return fail(IRIS_ERR_ARG, "iris_get_normal_space: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(normal_space_kernel, B, 8192, stream, normal, B, out);
}
extern "C" IRIS_API int iris_double_sided(const float* V, float* N, int64_t B, iris_stream_t stream) {
    if (B < 0 || (B > 0 && (!V || !N))) return fail(IRIS_ERR_ARG, "iris_double_sided: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(double_sided_kernel, B, 8192, stream, V, N, B);
}
extern "C" IRIS_API int iris_angle2xyz(const float* theta, const float* phi, int64_t B, float* out, iris_stream_t stream) {
    if (B < 0 || (B > 0 && (!theta || !phi || !out))) return fail(IRIS_ERR_ARG, "iris_angle2xyz: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(angle2xyz_kernel, B, 8192, stream, theta, phi, B, out);
}
extern "C" IRIS_API int iris_ggx_terms(int op, const float* a, const float* b, const float* c, int64_t B, float* out, float* out2, iris_stream_t stream) {
    const bool need_b = op != 4, need_c = op == 2, need_2 = op == 4;
    if (op < 0 || op > 4 || B < 0 || (B > 0 && (!a || !out || (need_b && !b) || (need_c && !c) || (need_2 && !out2))))
        return fail(IRIS_ERR_ARG, "iris_ggx_terms: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(ggx_terms_kernel, B, 8192, stream, op, a, b, c, B, out, out2);
}

// ---- 8(f)-3: packed shading cache + shading combine (iris_cache.h)
extern "C" IRIS_API int iris_cache_row_floats(int R) { return (R < 1 || R > kMaxLevels) ? 0 : cache_row_floats(R); }
extern "C" IRIS_API int iris_cache_pack(const float* diffuse, const float* const* spec0, const float* const* spec1, int64_t n, int R, float* rows,
                                        iris_stream_t stream) {
    if (n < 0 || R < 1 || R > kMaxLevels || (n > 0 && (!diffuse || !spec0 || !spec1 || !rows))) return fail(IRIS_ERR_ARG, "iris_cache_pack: bad arguments");
    if (n == 0) return IRIS_OK;
    CacheMaps m{};
    m.diffuse = diffuse;
    for (int j = 0; j < R; ++j) {
        if (!spec0[j] || !spec1[j]) return fail(IRIS_ERR_ARG, "iris_cache_pack: null map");
        m.s0[j] = spec0[j]; m.s1[j] = spec1[j];
    }
    return launch1d(cache_pack_kernel, n * (cache_row_floats(R) / 4), 16384, stream, m, n, R, rows);
}
extern "C" IRIS_API int iris_cache_gather(const float* rows, const int64_t* idx, int64_t B, int R, float* out, iris_stream_t stream) {
    if (B < 0 || R < 1 || R > kMaxLevels || (B > 0 && (!rows || !out))) return fail(IRIS_ERR_ARG, "iris_cache_gather: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(cache_gather_kernel, B * (3 + 6 * R), 16384, stream, rows, idx, B, R, out);
}
extern "C" IRIS_API int iris_shade_cached_fwd(const float* rows, const int64_t* idx, const float* albedo, const float* metallic,
                                              const float* roughness, int64_t B, int R, float* L, iris_stream_t stream) {
    if (B < 0 || R < 1 || R > kMaxLevels || (B > 0 && (!rows || !albedo || !metallic || !roughness || !L)))
        return fail(IRIS_ERR_ARG, "iris_shade_cached_fwd: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(shade_cached_fwd_kernel, B, 16384, stream, rows, idx, albedo, metallic,
                       roughness, B, R, L);
}
extern "C" IRIS_API int iris_shade_cached_bwd(const float* rows, const int64_t* idx, const float* albedo, const float* metallic,
                                              const float* roughness, const float* gL, int64_t B, int R, float* g_albedo, float* g_metallic,
                                              float* g_roughness, iris_stream_t stream) {
    if (B < 0 || R < 1 || R > kMaxLevels || (B > 0 && (!rows || !albedo || !metallic || !roughness || !gL)))
        return fail(IRIS_ERR_ARG, "iris_shade_cached_bwd: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(shade_cached_bwd_kernel, B, 16384, stream, rows, idx, albedo, metallic,
                       roughness, gL, B, R, g_albedo, g_metallic, g_roughness);
}

// ---- the BRDF trainer's propagation regulariser (iris_prop.h; train_brdf_crf.py:212-290)
static bool prop_n_ok(int64_t N) { return N >= 0 && N < (int64_t(1) << 31) - 64; }       // positions and counts are 32-bit in the kernels
extern "C" IRIS_API int iris_prop_runs(const int64_t* sorted_seg, int64_t N, int32_t* runs, iris_stream_t stream) {
    if (!prop_n_ok(N) || (N > 0 && (!sorted_seg || !runs))) return fail(IRIS_ERR_ARG, "iris_prop_runs: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(prop_runs_kernel, N, 4096, stream, sorted_seg, (int)N, (int2*)runs);
}
extern "C" IRIS_API int iris_prop_draws(const int32_t* runs, const int64_t* order, int64_t N, int K, uint64_t seed, int64_t* draws, iris_stream_t stream) {
    if (!prop_n_ok(N) || K < 1 || (N > 0 && (!runs || !order || !draws))) return fail(IRIS_ERR_ARG, "iris_prop_draws: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(prop_draws_kernel, N * K, 16384, stream, (const int2*)runs, order, (int)N, K, seed, draws);
}
static bool prop_sigmas(double sigma_albedo, double sigma_pos, PropArgs& a) {
    a.sa2 = (float)(sigma_albedo * sigma_albedo);
    a.sp2 = (float)(sigma_pos * sigma_pos);
    return a.sa2 > 0.f && a.sp2 > 0.f && std::isfinite(a.sa2) && std::isfinite(a.sp2);
}
extern "C" IRIS_API int iris_prop_semantic_fwd(const int32_t* runs, const int64_t* order, const float* roughness, const float* metallic, const float* albedo,
                                               const float* positions, int64_t N, int K, const int64_t* draws, uint64_t seed, double sigma_albedo,
                                               double sigma_pos, int normalise, double voxel_min, double voxel_max, float ls, float* records, float* saved,
                                               float* terms, float* loss, iris_stream_t stream) {
    PropArgs a;
    if (!prop_n_ok(N) || K < 1 || !loss || !prop_sigmas(sigma_albedo, sigma_pos, a) ||
        (N > 0 && (!runs || !order || !roughness || !metallic || !albedo || !positions || !records || !saved || !terms)))
        return fail(IRIS_ERR_ARG, "iris_prop_semantic_fwd: bad arguments");
    if (((uintptr_t)records | (uintptr_t)saved) % 16) return fail(IRIS_ERR_ARG, "iris_prop_semantic_fwd: records and saved must be 16-byte aligned");
    if (N > 0) {
        int rc = launch1d(prop_pack_kernel, N, 4096, stream, order, albedo, positions, roughness, metallic, (int)N, normalise, (float)voxel_min,
                          (float)(voxel_max - voxel_min), (PropRec*)records);
        if (rc) return rc;
        a.runs = (const int2*)runs; a.order = order; a.rec = (const PropRec*)records; a.draws = draws; a.seed = seed; a.n = (int)N; a.K = K;
        rc = launch1d(prop_semantic_fwd_kernel, N * 64, 1 << 16, stream, a, (float4*)saved, terms);     // one wave per pixel
        if (rc) return rc;
    }
    hipLaunchKernelGGL(prop_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)terms, (int)N, ls, loss);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_prop_semantic_bwd(const int32_t* runs, const int64_t* order, const float* records, const float* saved, int64_t N, int K,
                                               const int64_t* draws, uint64_t seed, double sigma_albedo, double sigma_pos, float ls, const float* g_loss,
                                               float* g_sorted, float* g_roughness, float* g_metallic, iris_stream_t stream) {
    PropArgs a;
    if (!prop_n_ok(N) || K < 1 || !prop_sigmas(sigma_albedo, sigma_pos, a) ||
        (N > 0 && (!runs || !order || !records || !saved || !g_loss || !g_sorted || !g_roughness || !g_metallic)))
        return fail(IRIS_ERR_ARG, "iris_prop_semantic_bwd: bad arguments");
    if (((uintptr_t)records | (uintptr_t)saved) % 16) return fail(IRIS_ERR_ARG, "iris_prop_semantic_bwd: records and saved must be 16-byte aligned");
    if (N == 0) return IRIS_OK;
    a.runs = (const int2*)runs; a.order = order; a.rec = (const PropRec*)records; a.draws = draws; a.seed = seed; a.n = (int)N; a.K = K;
    const int targets = g_opt_prop_bwd_targets > 0 ? (int)std::min<long long>(g_opt_prop_bwd_targets, 1 << 20) : kPropBwdTargets;
    const int members = g_opt_prop_lds_members >= 0 ? (int)std::min<long long>(g_opt_prop_lds_members, kPropLdsMembers) : kPropLdsMembers;   // 64 KB at most
    HIP_TRY(hipMemsetAsync(g_sorted, 0, (size_t)N * 2 * sizeof(float), (hipStream_t)stream));
    const int64_t chunks = (N + targets - 1) / targets;
    hipLaunchKernelGGL(prop_semantic_bwd_kernel, dim3(grid_for(chunks, 1, 1 << 16)), dim3(kPropBwdThreads), (size_t)members * 2 * sizeof(float), (hipStream_t)stream,
                       a, (const float4*)saved, g_loss, ls, targets, members, g_sorted);
    HIP_TRY(hipGetLastError());
    return launch1d(prop_semantic_bwd_finish_kernel, N, 4096, stream, (const int2*)runs, order, (const float4*)saved, g_loss, ls, (const float*)g_sorted, (int)N,
                    g_roughness, g_metallic);
}
extern "C" IRIS_API int iris_prop_part_fwd(const int32_t* runs, const int64_t* order, const float* roughness, const float* metallic, int64_t N, float lp,
                                           float* seg_means, float* signs, float* terms, float* loss, iris_stream_t stream) {
    if (!prop_n_ok(N) || !loss || (N > 0 && (!runs || !order || !roughness || !metallic || !seg_means || !signs || !terms)))
        return fail(IRIS_ERR_ARG, "iris_prop_part_fwd: bad arguments");
    if ((uintptr_t)seg_means % 16 || (uintptr_t)signs % 8) return fail(IRIS_ERR_ARG, "iris_prop_part_fwd: seg_means must be 16-byte, signs 8-byte aligned");
    if (N > 0) {
        int rc = launch1d(prop_part_means_kernel, N * 64, 1 << 16, stream, (const int2*)runs, order, roughness, metallic, (int)N, (float4*)seg_means);
        if (rc) return rc;
        rc = launch1d(prop_part_terms_kernel, N, 4096, stream, (const int2*)runs, order, roughness, metallic, (const float4*)seg_means, (int)N, (float2*)signs, terms);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(prop_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)terms, (int)N, N > 0 ? lp / (float)N : 0.f, loss);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_prop_part_bwd(const int32_t* runs, const int64_t* order, const float* roughness, const float* seg_means, const float* signs,
                                           int64_t N, float lp, const float* g_loss, float* g_roughness, float* g_metallic, iris_stream_t stream) {
    if (!prop_n_ok(N) || (N > 0 && (!runs || !order || !roughness || !seg_means || !signs || !g_loss || !g_roughness || !g_metallic)))
        return fail(IRIS_ERR_ARG, "iris_prop_part_bwd: bad arguments");
    if ((uintptr_t)seg_means % 16 || (uintptr_t)signs % 8) return fail(IRIS_ERR_ARG, "iris_prop_part_bwd: seg_means must be 16-byte, signs 8-byte aligned");
    if (N == 0) return IRIS_OK;
    return launch1d(prop_part_bwd_kernel, N * 64, 1 << 16, stream, (const int2*)runs, order, roughness, (const float4*)seg_means, (const float2*)signs, g_loss, lp,
                    (int)N, g_roughness, g_metallic);
}

// ---- the trainers' albedo regulariser (iris_loss.h; train_brdf_crf.py:292-306, initialize.py:188-201)
static int loss_blocks(int64_t N) { return grid_for(N, kLossThreads, kLossMaxBlocks); }       // a function of N alone: the sums' grouping does not depend on the device
extern "C" IRIS_API int iris_loss_albedo_fwd(const int32_t* runs, const int64_t* order, const float* albedo, const float* prior, int64_t N, int fit_scale,
                                             float weight, float* seg_means, float* partials, float* k, float* loss, iris_stream_t stream) {
    if (!prop_n_ok(N) || !loss || !k || (N > 0 && (!runs || !order || !albedo || !prior || !seg_means || !partials)))
        return fail(IRIS_ERR_ARG, "iris_loss_albedo_fwd: bad arguments");
    if ((uintptr_t)seg_means % 16 || (uintptr_t)partials % 8) return fail(IRIS_ERR_ARG, "iris_loss_albedo_fwd: seg_means must be 16-byte, partials 8-byte aligned");
    const int blocks = N > 0 ? loss_blocks(N) : 0;
    float2* dots = (float2*)partials;                 // 2 x blocks floats, then the terms' blocks floats
    float* terms = partials + 2 * (size_t)blocks;
    if (N > 0) {
        int rc = launch1d(loss_seg_means_kernel, N * 64, 1 << 16, stream, (const int2*)runs, order, prior, (int)N, (float4*)seg_means);
        if (rc) return rc;
        if (fit_scale) {
            hipLaunchKernelGGL(loss_dots_kernel, dim3(blocks), dim3(kLossThreads), 0, (hipStream_t)stream, (const int2*)runs, order, albedo,
                               (const float4*)seg_means, (int)N, dots);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(loss_terms_kernel, dim3(blocks), dim3(kLossThreads), 0, (hipStream_t)stream, (const int2*)runs, order, albedo,
                           (const float4*)seg_means, fit_scale ? (const float2*)dots : (const float2*)nullptr, blocks, (int)N, terms, k);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(prop_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)terms, blocks, N > 0 ? (float)((double)weight / (3.0 * (double)N)) : 0.f, loss);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_loss_albedo_bwd(const int32_t* runs, const int64_t* order, const float* albedo, const float* seg_means, const float* k, int64_t N,
                                             float weight, const float* g_loss, float* g_albedo, iris_stream_t stream) {
    if (!prop_n_ok(N) || (N > 0 && (!runs || !order || !albedo || !seg_means || !k || !g_loss || !g_albedo)))
        return fail(IRIS_ERR_ARG, "iris_loss_albedo_bwd: bad arguments");
    if ((uintptr_t)seg_means % 16) return fail(IRIS_ERR_ARG, "iris_loss_albedo_bwd: seg_means must be 16-byte aligned");
    if (N == 0) return IRIS_OK;
    return launch1d(loss_albedo_bwd_kernel, N, 4096, stream, (const int2*)runs, order, albedo, (const float4*)seg_means, k, g_loss,
                    (float)(2.0 * (double)weight / (3.0 * (double)N)), (int)N, g_albedo);
}

// ---- the camera response model (iris_crf.h; crf/model_crf.py:32-122)
static bool crf_args(const float* grid, const float* table, int n, const float* exposure, int64_t n_exposure, float exposure_value, int64_t B, CrfArgs& a) {
    a.grid = grid; a.table = table; a.n = n; a.exposure = exposure; a.n_exposure = n_exposure; a.exposure_value = exposure_value; a.B = B;
    return n >= 2 && n <= kCrfMaxKnots && B >= 0 && grid && table && (!exposure || n_exposure == 1 || n_exposure == B);
}
static int crf_slabs(int64_t B) { return grid_for(B, kCrfThreads, kCrfSlabs); }       // a function of B alone: the sum's grouping does not depend on the device
template <bool INV>
static int crf_lookup(const char* who, const float* grid, const float* table, int n, const float* in, const float* exposure, int64_t n_exposure,
                      float exposure_value, int64_t B, float* out, iris_stream_t stream) {
    CrfArgs a;
    if (!crf_args(grid, table, n, exposure, n_exposure, exposure_value, B, a) || (B > 0 && (!in || !out)))
        return fail(IRIS_ERR_ARG, std::string(who) + ": bad arguments (2 <= n <= 1024, exposure holds 1 or B values)");
    if (B == 0) return IRIS_OK;
    hipLaunchKernelGGL(crf_lookup_kernel<INV>, dim3(grid_for(B, kCrfThreads, kCrfLookupBlocks)), dim3(kCrfThreads), (size_t)n * 4 * sizeof(float), (hipStream_t)stream,
                       a, in, out);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_crf_fwd(const float* grid, const float* table, int n, const float* hdr, const float* exposure, int64_t n_exposure, float exposure_value,
                                     int64_t B, float* ldr, iris_stream_t stream) {
    return crf_lookup<false>("iris_crf_fwd", grid, table, n, hdr, exposure, n_exposure, exposure_value, B, ldr, stream);
}
extern "C" IRIS_API int iris_crf_lookup_inv(const float* grid, const float* inv_table, int n, const float* ldr, const float* exposure, int64_t n_exposure,
                                            float exposure_value, int64_t B, float* hdr, iris_stream_t stream) {
    return crf_lookup<true>("iris_crf_lookup_inv", grid, inv_table, n, ldr, exposure, n_exposure, exposure_value, B, hdr, stream);
}
extern "C" IRIS_API uint64_t iris_crf_bwd_workspace_bytes(int64_t B, int n) {
    if (B < 0 || n < 2 || n > kCrfMaxKnots) return 0;
    return (uint64_t)crf_slabs(B) * 3 * (uint64_t)n * sizeof(float);
}
extern "C" IRIS_API int iris_crf_bwd(const float* grid, const float* table, int n, const float* hdr, const float* exposure, int64_t n_exposure, float exposure_value,
                                     int64_t B, const float* g_ldr, float* g_hdr, float* g_table, void* workspace, uint64_t workspace_bytes,
                                     iris_stream_t stream) {
    CrfArgs a;
    if (!crf_args(grid, table, n, exposure, n_exposure, exposure_value, B, a) || (B > 0 && (!hdr || !g_ldr)))
        return fail(IRIS_ERR_ARG, "iris_crf_bwd: bad arguments (2 <= n <= 1024, exposure holds 1 or B values)");
    if (g_table && (!workspace || workspace_bytes < iris_crf_bwd_workspace_bytes(B, n) || (uintptr_t)workspace % 4))
        return fail(IRIS_ERR_ARG, "iris_crf_bwd: g_table needs a workspace of " + std::to_string(iris_crf_bwd_workspace_bytes(B, n)) + " bytes");
    if (B == 0) {
        if (g_table) HIP_TRY(hipMemsetAsync(g_table, 0, (size_t)3 * n * sizeof(float), (hipStream_t)stream));
        return IRIS_OK;
    }
    if (!g_hdr && !g_table) return IRIS_OK;
    const int slabs = crf_slabs(B);
    hipLaunchKernelGGL(crf_bwd_kernel, dim3(slabs), dim3(kCrfThreads), (size_t)n * (g_table ? 7 : 4) * sizeof(float), (hipStream_t)stream, a, hdr, g_ldr, g_hdr,
                       g_table ? (float*)workspace : (float*)nullptr);
    HIP_TRY(hipGetLastError());
    if (!g_table) return IRIS_OK;
    return launch1d(crf_slab_sum_kernel, 3 * n, 16, stream, (const float*)workspace, slabs, 3 * n, g_table);
}
extern "C" IRIS_API int iris_crf_inv_table(const float* grid, const float* table, int n, float* inv_table, iris_stream_t stream) {
    if (n < 2 || n > kCrfMaxKnots || !grid || !table || !inv_table) return fail(IRIS_ERR_ARG, "iris_crf_inv_table: bad arguments (2 <= n <= 1024)");
    hipLaunchKernelGGL(crf_inv_table_kernel, dim3(3), dim3(kCrfMaxKnots), 0, (hipStream_t)stream, grid, table, n, inv_table);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ---- the photometric step loss of the emitter and initialisation stages (iris_loss.h; train_emitter.py:189-195, initialize.py:180-184)
extern "C" IRIS_API uint64_t iris_loss_photometric_workspace_bytes(int64_t B) {
    if (B < 1) return 0;
    return (uint64_t)loss_blocks(B) * sizeof(double);
}
extern "C" IRIS_API int iris_loss_photometric(const float* L_sum, int n_calls, const float* grid, const float* table, int n, const float* exposure,
                                              int64_t n_exposure, float exposure_value, const float* rgbs_gt, int64_t B, float* loss, float* psnr, float* dL_sum,
                                              void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    CrfArgs a;
    if (!crf_args(grid, table, n, exposure, n_exposure, exposure_value, B, a) || B < 1 || B > (int64_t)1 << 40 || n_calls < 1 || n_calls > 1 << 24 || !L_sum ||
        !rgbs_gt || !loss || !psnr || !dL_sum)
        return fail(IRIS_ERR_ARG, "iris_loss_photometric: bad arguments (B >= 1, 1 <= n_calls <= 2^24, 2 <= n <= 1024, exposure holds 1 or B values)");
    if (!workspace || workspace_bytes < iris_loss_photometric_workspace_bytes(B) || (uintptr_t)workspace % 8)
        return fail(IRIS_ERR_ARG, "iris_loss_photometric: needs an 8-byte aligned workspace of " + std::to_string(iris_loss_photometric_workspace_bytes(B)) + " bytes");
    const int blocks = loss_blocks(B);
    const double three_b = 3.0 * (double)B;
    hipLaunchKernelGGL(loss_photometric_kernel, dim3(blocks), dim3(kLossThreads), (size_t)n * 4 * sizeof(float), (hipStream_t)stream, a, L_sum, (float)n_calls, rgbs_gt,
                       (float)three_b, (double*)workspace, dL_sum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_photometric_finish_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, (const double*)workspace, blocks, three_b, loss, psnr);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ---- 8(f)-4: denoiser substitute (iris_denoise.h)
extern "C" IRIS_API uint64_t iris_denoise_workspace_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return (uint64_t)H * W * (2 + 2 * kDnMaxMaps) * sizeof(float4);
}
template <int M>
static void denoise_group(const DnParams& P, const DnMaps& mp, const float4* g0, const float4* g1, int iterations, hipStream_t st) {
    const dim3 grid((P.W + 15) / 16, (P.H + 15) / 16), block(256);
    hipLaunchKernelGGL((dn_variance_kernel<M>), grid, block, 0, st, P, mp, g0, g1);
    DnMaps cur = mp;
    for (int it = 0; it < iterations; ++it) {
        if (it == iterations - 1) hipLaunchKernelGGL((dn_atrous_kernel<M, true>), grid, block, 0, st, P, cur, g0, g1, 1 << it);
        else hipLaunchKernelGGL((dn_atrous_kernel<M, false>), grid, block, 0, st, P, cur, g0, g1, 1 << it);
        for (int m = 0; m < M; ++m) std::swap(cur.a[m], cur.b[m]);
    }
}
extern "C" IRIS_API int iris_denoise(const float* normal, const float* position, const uint8_t* valid, int H, int W, int n_maps,
                                     const float* const* in, float* const* out, int iterations, float sigma_l, float sigma_n, float sigma_p,
                                     void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    if (H < 1 || W < 1 || n_maps < 0 || iterations < 1 || iterations > 8 || !(sigma_l > 0.f) || !(sigma_n >= 0.f) || !(sigma_p > 0.f) ||
        (n_maps > 0 && (!in || !out)))
        return fail(IRIS_ERR_ARG, "iris_denoise: bad arguments");
    if (!workspace || workspace_bytes < iris_denoise_workspace_bytes(H, W))
        return fail(IRIS_ERR_ARG, "iris_denoise: workspace of iris_denoise_workspace_bytes() bytes required");
    if (n_maps == 0) return IRIS_OK;
    for (int m = 0; m < n_maps; ++m) if (!in[m] || !out[m]) return fail(IRIS_ERR_ARG, "iris_denoise: null map");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    float4* g0 = (float4*)workspace;
    float4* g1 = g0 + n;
    float4* bufs = g1 + n;
    hipLaunchKernelGGL(dn_guides_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, normal, position, valid, n, g0, g1);
    DnParams P{H, W, sigma_l, sigma_n, sigma_p};
    for (int m0 = 0; m0 < n_maps; m0 += kDnMaxMaps) {
        const int M = std::min(kDnMaxMaps, n_maps - m0);
        DnMaps mp{};
        for (int m = 0; m < M; ++m) { mp.in[m] = in[m0 + m]; mp.out[m] = out[m0 + m]; mp.a[m] = bufs + (int64_t)(2 * m) * n; mp.b[m] = bufs + (int64_t)(2 * m + 1) * n; }
        switch (M) {
            case 1: denoise_group<1>(P, mp, g0, g1, iterations, st); break;
            case 2: denoise_group<2>(P, mp, g0, g1, iterations, st); break;
            case 3: denoise_group<3>(P, mp, g0, g1, iterations, st); break;
            default: denoise_group<4>(P, mp, g0, g1, iterations, st); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ---- SSIM and the squared error behind PSNR (iris_metrics.h; render.py:236-239)
static bool metrics_shape(int N, int H, int W, int C, int& tiles_x, int& tiles_y) {
    if (N < 1 || H < 7 || W < 7 || (C != 1 && C != 3)) return false;
    tiles_x = (W + kMetTileX - 1) / kMetTileX;
    tiles_y = (H + kMetTileY - 1) / kMetTileY;
    return (int64_t)N * tiles_x * tiles_y <= INT32_MAX && (int64_t)W * C <= INT32_MAX - 4 * kMetTileX;       // the grid, and a row's element index, are ints
}
extern "C" IRIS_API uint64_t iris_image_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
    int tx, ty;
    if (!metrics_shape(N, H, W, C, tx, ty)) return 0;
    return (uint64_t)N * tx * ty * C * 2 * sizeof(double);
}
extern "C" IRIS_API int iris_image_metrics(const float* a, const float* b, int32_t N, int32_t H, int32_t W, int32_t C, float data_range, double* sums,
                                           float* ssim_map, void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    int tx, ty;
    if (!metrics_shape(N, H, W, C, tx, ty))
        return fail(IRIS_ERR_ARG, "iris_image_metrics: bad shape (N, H, W, C) = (" + std::to_string(N) + ", " + std::to_string(H) + ", " + std::to_string(W) + ", " +
                                      std::to_string(C) + "): N >= 1, H >= 7, W >= 7, C 1 or 3");
    if (!(data_range > 0.f) || !std::isfinite(data_range)) return fail(IRIS_ERR_ARG, "iris_image_metrics: data_range must be positive and finite");
    if (!a || !b || !sums || (uintptr_t)a % 4 || (uintptr_t)b % 4 || (uintptr_t)sums % 8 || (uintptr_t)ssim_map % 4)
        return fail(IRIS_ERR_ARG, "iris_image_metrics: null or misaligned a / b / sums / ssim_map");
    const uint64_t need = iris_image_metrics_workspace_bytes(N, H, W, C);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(IRIS_ERR_ARG, "iris_image_metrics: an 8-byte aligned workspace of " + std::to_string(need) + " bytes is required (got " +
                                      std::to_string(workspace_bytes) + ")");
    const float k1r = 0.01f * data_range, k2r = 0.03f * data_range;
    MetArgs g{a, b, (double*)workspace, ssim_map, H, W, tx, ty, k1r * k1r, k2r * k2r};
    const hipStream_t st = (hipStream_t)stream;
    const int tiles = tx * ty;
    if (C == 1) {
        hipLaunchKernelGGL(metrics_tile_kernel<1>, dim3(N * tiles), dim3(kMetThreads), 0, st, g);
        hipLaunchKernelGGL(metrics_slab_sum_kernel<1>, dim3(N), dim3(kMetThreads), 0, st, (const double*)workspace, tiles, sums);
    } else {
        hipLaunchKernelGGL(metrics_tile_kernel<3>, dim3(N * tiles), dim3(kMetThreads), 0, st, g);
        hipLaunchKernelGGL(metrics_slab_sum_kernel<3>, dim3(N), dim3(kMetThreads), 0, st, (const double*)workspace, tiles, sums);
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ---- material metrics (iris_matmetrics.h; utils/metric_brdf.py:32-92)
static bool matmetrics_shape(int N, int H, int W, int& chunks) {
    if (N < 1 || H < 1 || W < 1 || (int64_t)H * W > kMmMaxPixels) return false;
    chunks = (int)(((int64_t)H * W + kMmChunk - 1) / kMmChunk);
    return (int64_t)N * chunks <= INT32_MAX;                              // the grid
}
extern "C" IRIS_API uint64_t iris_material_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    int chunks;
    if (!matmetrics_shape(N, H, W, chunks)) return 0;
    return (uint64_t)N * chunks * kMmWords * sizeof(uint64_t);
}
extern "C" IRIS_API int iris_material_metrics(const iris_material_metrics_args* v, iris_stream_t stream) {
    if (!v) return fail(IRIS_ERR_ARG, "iris_material_metrics: null arguments");
    int chunks;
    if (!matmetrics_shape(v->N, v->H, v->W, chunks))
        return fail(IRIS_ERR_ARG, "iris_material_metrics: unsupported size (N, H, W) = (" + std::to_string(v->N) + ", " + std::to_string(v->H) + ", " +
                                      std::to_string(v->W) + "): N, H, W >= 1, H W <= 2^30, N ceil(H W / 512) < 2^31");
    const void* f32[] = {v->emit_gt, v->albedo_gt, v->kd_gt, v->rough_gt, v->emit, v->albedo_is_u8 ? nullptr : v->albedo, v->kd_is_u8 ? nullptr : v->kd,
                         v->rough_is_u8 ? nullptr : v->rough};
    if (!v->emit_gt || !v->albedo_gt || !v->kd_gt || !v->rough_gt || !v->emit || !v->albedo || !v->kd || !v->rough || !v->sums || (uintptr_t)v->sums % 8)
        return fail(IRIS_ERR_ARG, "iris_material_metrics: a null map, or null / misaligned sums");
    for (const void* p : f32)
        if ((uintptr_t)p % 4) return fail(IRIS_ERR_ARG, "iris_material_metrics: a float32 map is not 4-byte aligned");
    const uint64_t need = iris_material_metrics_workspace_bytes(v->N, v->H, v->W);
    if (!v->workspace || v->workspace_bytes < need || (uintptr_t)v->workspace % 8)
        return fail(IRIS_ERR_ARG, "iris_material_metrics: an 8-byte aligned workspace of " + std::to_string(need) + " bytes is required (got " +
                                      std::to_string(v->workspace_bytes) + ")");
    MmArgs g{v->emit_gt, v->albedo_gt, v->kd_gt, v->rough_gt, v->emit, v->albedo, v->kd, v->rough, v->albedo_is_u8 != 0, v->kd_is_u8 != 0, v->rough_is_u8 != 0,
             v->H * v->W, chunks, (uint64_t*)v->workspace};
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(matmetrics_chunk_kernel, dim3(v->N * chunks), dim3(kMmThreads), 0, st, g);
    hipLaunchKernelGGL(matmetrics_slab_sum_kernel, dim3(v->N), dim3(kMmThreads), 0, st, (const uint64_t*)v->workspace, chunks, v->sums);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ---- the trainers' validation (iris_validate.h; train_brdf_crf.py:331-499)
extern "C" IRIS_API uint64_t iris_val_kd_loss_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    int chunks;
    if (!matmetrics_shape(N, H, W, chunks)) return 0;
    return (uint64_t)N * chunks * sizeof(double);
}
extern "C" IRIS_API int iris_val_kd_loss(const iris_val_kd_loss_args* v, iris_stream_t stream) {
    if (!v) return fail(IRIS_ERR_ARG, "iris_val_kd_loss: null arguments");
    int chunks;
    if (!matmetrics_shape(v->N, v->H, v->W, chunks))
        return fail(IRIS_ERR_ARG, "iris_val_kd_loss: unsupported size (N, H, W) = (" + std::to_string(v->N) + ", " + std::to_string(v->H) + ", " +
                                      std::to_string(v->W) + "): N, H, W >= 1, H W <= 2^30, N ceil(H W / 512) < 2^31");
    if (!v->albedo || !v->metallic || !v->valid || !v->gt || !v->sums || (uintptr_t)v->sums % 8)
        return fail(IRIS_ERR_ARG, "iris_val_kd_loss: a null map, or null / misaligned sums");
    if (v->gt_is_u8 ? (!v->lut || v->emit) : (!v->emit || v->lut))
        return fail(IRIS_ERR_ARG, "iris_val_kd_loss: 8-bit ground truth takes lut and no emit, float32 ground truth emit and no lut");
    const void* f32[] = {v->albedo, v->metallic, v->gt_is_u8 ? nullptr : v->gt, v->emit, v->lut};
    for (const void* p : f32)
        if ((uintptr_t)p % 4) return fail(IRIS_ERR_ARG, "iris_val_kd_loss: a float32 map is not 4-byte aligned");
    const uint64_t need = iris_val_kd_loss_workspace_bytes(v->N, v->H, v->W);
    if (!v->workspace || v->workspace_bytes < need || (uintptr_t)v->workspace % 8)
        return fail(IRIS_ERR_ARG, "iris_val_kd_loss: an 8-byte aligned workspace of " + std::to_string(need) + " bytes is required (got " +
                                      std::to_string(v->workspace_bytes) + ")");
    ValLossArgs g{v->albedo, v->metallic, v->valid, v->gt, v->emit, v->lut, v->gt_is_u8 != 0, v->H * v->W, chunks, (double*)v->workspace};
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(val_loss_chunk_kernel, dim3(v->N * chunks), dim3(kMmThreads), 0, st, g);
    hipLaunchKernelGGL(val_loss_slab_sum_kernel, dim3(v->N), dim3(kMmThreads), 0, st, (const double*)v->workspace, chunks, v->sums);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// texture export: UV rasteriser, per-texel resolve, quantisation (iris_texture.h)
// ======================================================================================================
static_assert(kUvSub == 256, "uv_setup shifts by 8");
static const int64_t kUvMaxRes = 8192;
static bool uv_shape(int64_t n_vt, int64_t F, int H, int W) {
    return n_vt >= 0 && F >= 0 && F <= INT32_MAX && H >= 1 && W >= 1 && H <= kUvMaxRes && W <= kUvMaxRes;
}
static int64_t uv_blocks(int64_t n) { return (n + kUvThreads - 1) / kUvThreads; }
extern "C" IRIS_API uint64_t iris_uv_raster_workspace_bytes(int64_t F) {
    if (F < 0 || F > INT32_MAX) return 0;
    return (uint64_t)((16 + 12 * F + 15) / 16 * 16);       // header, then per triangle an int64 first item and an int32 face index
}
static int uv_raster(const char* who, const float* vt, int64_t n_vt, const int32_t* ft, int64_t F, int H, int W, int32_t* ids, void* workspace,
                     uint64_t workspace_bytes, int mode, iris_stream_t stream) {
    if (!uv_shape(n_vt, F, H, W))
        return fail(IRIS_ERR_ARG, std::string(who) + ": bad sizes (n_vt " + std::to_string(n_vt) + ", F " + std::to_string(F) + ", H " + std::to_string(H) + ", W " +
                                      std::to_string(W) + "): H and W in [1, 8192], F below 2^31");
    if (!ids || (uintptr_t)ids % 4 || (F > 0 && (!vt || !ft || (uintptr_t)vt % 4 || (uintptr_t)ft % 4)))
        return fail(IRIS_ERR_ARG, std::string(who) + ": null or misaligned vt / ft / ids");
    const uint64_t need = iris_uv_raster_workspace_bytes(F);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(IRIS_ERR_ARG, std::string(who) + ": an 8-byte aligned workspace of " + std::to_string(need) + " bytes is required (got " +
                                      std::to_string(workspace_bytes) + ")");
    if (mode < 0 || (mode > kUvModeAllLarge && mode < 64)) return fail(IRIS_ERR_ARG, std::string(who) + ": unknown mode " + std::to_string(mode));
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(ids, 0xFF, (size_t)H * W * sizeof(int32_t), st));          // -1: uncovered, and the largest value of the unsigned atomicMin
    if (F == 0) return IRIS_OK;
    // the queue's slot field holds 24 bits, its item field 40: F triangles of at most 2^16 items each (8192 rows x 128 segments / 16) fit when F < 2^24.
    // A larger mesh keeps every triangle with its lane (correct at any size; such a mesh has no room for large triangles anyway).
    static_assert(kUvMaxRes * ((kUvMaxRes + 63) / 64) / kUvChunkSegs <= (1 << (kUvItemBits - kUvSlotBits)), "items of one triangle");
    int64_t small_max = mode == kUvModeAuto ? kUvSmallMaxTexels : mode == kUvModeAllSmall ? INT64_MAX : mode == kUvModeAllLarge ? 0 : (int64_t)mode;
    if (F >= ((int64_t)1 << kUvSlotBits)) small_max = INT64_MAX;
    UvQueue q;
    q.head = (unsigned long long*)workspace;
    q.first = (int64_t*)((char*)workspace + 16);
    q.face = (int32_t*)((char*)workspace + 16 + 8 * F);
    q.capacity = F;
    HIP_TRY(hipMemsetAsync(workspace, 0, 16, st));
    hipLaunchKernelGGL(uv_class_kernel, dim3((unsigned)uv_blocks(F)), dim3(kUvThreads), 0, st, vt, n_vt, ft, F, H, W, (uint32_t*)ids, q, small_max);
    if (small_max != INT64_MAX)
        hipLaunchKernelGGL(uv_span_kernel, dim3(kUvSpanBlocks), dim3(kUvThreads), 0, st, vt, n_vt, ft, H, W, (uint32_t*)ids, q);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_uv_raster(const float* vt, int64_t n_vt, const int32_t* ft, int64_t F, int32_t H, int32_t W, int32_t* ids, void* workspace,
                                       uint64_t workspace_bytes, iris_stream_t stream) {
    return uv_raster("iris_uv_raster", vt, n_vt, ft, F, H, W, ids, workspace, workspace_bytes, kUvModeAuto, stream);
}
extern "C" IRIS_API int iris_debug_uv_raster(const float* vt, int64_t n_vt, const int32_t* ft, int64_t F, int32_t H, int32_t W, int32_t* ids, void* workspace,
                                             uint64_t workspace_bytes, int mode, iris_stream_t stream) {
    return uv_raster("iris_debug_uv_raster", vt, n_vt, ft, F, H, W, ids, workspace, workspace_bytes, mode, stream);
}
extern "C" IRIS_API int iris_uv_resolve(const float* vt, int64_t n_vt, const int32_t* ft, const float* v, int64_t n_v, const int32_t* f, int64_t F, int32_t H,
                                        int32_t W, const int32_t* ids, int64_t texel0, int64_t n, float* bary, float* xyz, iris_stream_t stream) {
    if (!uv_shape(n_vt, F, H, W) || n_v < 0 || texel0 < 0 || n < 0 || texel0 + n > (int64_t)H * W)
        return fail(IRIS_ERR_ARG, "iris_uv_resolve: bad sizes or a texel range outside the texture (texel0 " + std::to_string(texel0) + ", n " + std::to_string(n) + ")");
    if (n == 0) return IRIS_OK;
    if (!ids || !xyz || (uintptr_t)ids % 4 || (uintptr_t)xyz % 4 || (uintptr_t)bary % 4 ||
        (F > 0 && (!vt || !ft || !v || !f || (uintptr_t)vt % 4 || (uintptr_t)ft % 4 || (uintptr_t)v % 4 || (uintptr_t)f % 4)))
        return fail(IRIS_ERR_ARG, "iris_uv_resolve: null or misaligned pointer");
    hipLaunchKernelGGL(uv_resolve_kernel, dim3((unsigned)uv_blocks(n)), dim3(kUvThreads), 0, (hipStream_t)stream, vt, n_vt, ft, v, n_v, f, F, H, W, ids, texel0, n,
                       bary, xyz);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_texture_quantize(const float* albedo, const float* roughness, const float* metallic, const int32_t* ids, int64_t texel0, int64_t n,
                                              int64_t n_texels, uint8_t* albedo_img, uint8_t* rm_img, iris_stream_t stream) {
    if (texel0 < 0 || n < 0 || n_texels < 0 || n_texels > kUvMaxRes * kUvMaxRes || texel0 + n > n_texels)
        return fail(IRIS_ERR_ARG, "iris_texture_quantize: texel range [" + std::to_string(texel0) + ", +" + std::to_string(n) + ") outside the texture of " +
                                      std::to_string(n_texels) + " texels");
    if (n == 0) return IRIS_OK;
    if (!albedo || !roughness || !metallic || !ids || !albedo_img || !rm_img || (uintptr_t)albedo % 4 || (uintptr_t)roughness % 4 || (uintptr_t)metallic % 4 ||
        (uintptr_t)ids % 4 || (uintptr_t)albedo_img % 4 || (uintptr_t)rm_img % 4)
        return fail(IRIS_ERR_ARG, "iris_texture_quantize: null pointer, or one that is not 4-byte aligned (the images are stored in words)");
    const int64_t groups = (texel0 + n + 3) / 4 - texel0 / 4;
    hipLaunchKernelGGL(uv_quantize_kernel, dim3((unsigned)uv_blocks(groups)), dim3(kUvThreads), 0, (hipStream_t)stream, albedo, roughness, metallic, ids, texel0, n,
                       albedo_img, rm_img);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// texture export: the area-proportional atlas and the seam dilation (iris_atlas.h)
// ======================================================================================================
// -> KMAX (2^KMAX = R), or -1 unless R is a power of two in [4, 8192]
static int atlas_kmax(int R) {
    if (R < 4 || R > kUvMaxRes || (R & (R - 1))) return -1;
    int k = 0;
    while ((1 << k) < R) ++k;
    return k;
}
static_assert((1 << kAtlasKMaxLimit) == kUvMaxRes && kAtlasKMaxLimit + 3 == kAtlasHist, "classes 0 .. 13 and two clamp counters");
static const int64_t kAtlasMaxFaces = kUvMaxRes * kUvMaxRes / 16 * 2;          // two faces per 4 x 4 cell of the largest texture
extern "C" IRIS_API int iris_atlas_measure(const float* v, int64_t n_v, const int32_t* f, int64_t F, double* S, uint8_t* corner, iris_stream_t stream) {
    if (n_v < 0 || n_v > INT32_MAX || F < 0 || F > kAtlasMaxFaces)
        return fail(IRIS_ERR_ARG, "iris_atlas_measure: bad sizes (n_v " + std::to_string(n_v) + ", F " + std::to_string(F) + "): F at most 2^23");
    if (F == 0) return IRIS_OK;
    if (!f || !S || !corner || (n_v > 0 && !v) || (uintptr_t)v % 4 || (uintptr_t)f % 4 || (uintptr_t)S % 8)
        return fail(IRIS_ERR_ARG, "iris_atlas_measure: null or misaligned pointer");
    hipLaunchKernelGGL(atlas_measure_kernel, dim3((unsigned)((F + kAtlasThreads - 1) / kAtlasThreads)), dim3(kAtlasThreads), 0, (hipStream_t)stream, v, n_v, f, F, S,
                       corner);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API double iris_atlas_density(int32_t j) {
    if (j < kAtlasJMin || j > kAtlasJMax) return 0.0;
    return std::ldexp((j & 1) ? 1.4142135623730951 : 1.0, j >> 1);          // (>> of a negative int floors; the scaling is exact: no subnormals in this range)
}
extern "C" IRIS_API int iris_atlas_classes(const double* S, int64_t F, int32_t j, int32_t tex_res, uint8_t* k, int64_t* hist, iris_stream_t stream) {
    const int kmax = atlas_kmax(tex_res);
    if (kmax < 0 || F < 0 || F > kAtlasMaxFaces || j < kAtlasJMin || j > kAtlasJMax)
        return fail(IRIS_ERR_ARG, "iris_atlas_classes: bad sizes (F " + std::to_string(F) + ", j " + std::to_string(j) + ", tex_res " + std::to_string(tex_res) +
                                      "): tex_res a power of two in [4, 8192], j in [-800, 800], F at most 2^23");
    if (!hist || (uintptr_t)hist % 8 || (F > 0 && (!S || !k || (uintptr_t)S % 8))) return fail(IRIS_ERR_ARG, "iris_atlas_classes: null or misaligned pointer");
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(hist, 0, kAtlasHist * sizeof(int64_t), st));
    if (F == 0) return IRIS_OK;
    const int64_t blocks = std::min<int64_t>((F + kAtlasThreads - 1) / kAtlasThreads, kAtlasClassBlocks);
    hipLaunchKernelGGL(atlas_classes_kernel, dim3((unsigned)blocks), dim3(kAtlasThreads), 0, st, S, F, iris_atlas_density(j), kmax, k, (unsigned long long*)hist);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_atlas_place(const uint8_t* k, const uint8_t* corner, const int64_t* order, int64_t F, int32_t tex_res, const int64_t* hist_host,
                                         float* vt, iris_stream_t stream) {
    const int kmax = atlas_kmax(tex_res);
    if (kmax < 0 || F < 0 || F > kAtlasMaxFaces || !hist_host)
        return fail(IRIS_ERR_ARG, "iris_atlas_place: bad sizes (F " + std::to_string(F) + ", tex_res " + std::to_string(tex_res) + ") or no class histogram");
    AtlasTable t;
    int64_t faces = 0, texels = 0;
    for (int c = 0; c <= kAtlasKMaxLimit; ++c) {
        const int64_t n = hist_host[c];
        if (n < 0 || n > F || (n > 0 && (c < kAtlasKMin || c > kmax))) return fail(IRIS_ERR_ARG, "iris_atlas_place: the histogram names a class outside [2, KMAX]");
        t.start[c] = faces;                                     // the order is sorted by ascending class
        faces += n;
    }
    for (int c = kAtlasKMaxLimit; c >= 0; --c) {                // the layout goes from the largest class down
        t.base[c] = texels;
        texels += (hist_host[c] + 1) / 2 * ((int64_t)1 << (2 * c));
    }
    if (faces != F) return fail(IRIS_ERR_ARG, "iris_atlas_place: the histogram counts " + std::to_string(faces) + " faces, F is " + std::to_string(F));
    if (texels > (int64_t)tex_res * tex_res)
        return fail(IRIS_ERR_ARG, "iris_atlas_place: the classes need " + std::to_string(texels) + " texels, the texture has " + std::to_string((int64_t)tex_res * tex_res));
    if (F == 0) return IRIS_OK;
    if (!k || !corner || !order || !vt || (uintptr_t)order % 8 || (uintptr_t)vt % 4) return fail(IRIS_ERR_ARG, "iris_atlas_place: null or misaligned pointer");
    hipLaunchKernelGGL(atlas_place_kernel, dim3((unsigned)((F + kAtlasThreads - 1) / kAtlasThreads)), dim3(kAtlasThreads), 0, (hipStream_t)stream, k, corner, order, F,
                       (int)tex_res, kmax, t, vt);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_texture_dilate(const int32_t* ids, int32_t H, int32_t W, int32_t n, uint8_t* albedo_img, uint8_t* rm_img, iris_stream_t stream) {
    if (H < 1 || W < 1 || H > kUvMaxRes || W > kUvMaxRes || n < 0 || n > kDilateMax)
        return fail(IRIS_ERR_ARG, "iris_texture_dilate: bad sizes (H " + std::to_string(H) + ", W " + std::to_string(W) + ", n " + std::to_string(n) +
                                      "): H and W in [1, 8192], n in [0, 4]");
    if (!ids || !albedo_img || !rm_img || (uintptr_t)ids % 4 || albedo_img == rm_img) return fail(IRIS_ERR_ARG, "iris_texture_dilate: null, misaligned or shared pointer");
    if (n == 0) return IRIS_OK;
    const int64_t texels = (int64_t)H * W;
    hipLaunchKernelGGL(texture_dilate_kernel, dim3((unsigned)((texels + kAtlasThreads - 1) / kAtlasThreads)), dim3(kAtlasThreads), 0, (hipStream_t)stream, ids, (int)H,
                       (int)W, (int)n, albedo_img, rm_img);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// 5c-17: closest point on the mesh, the exported textures read back (iris_closest.h, iris_texmat.h)
// ======================================================================================================
static int closest_scene_check(const char* who, const iris_scene* s) {
    if (!s) return fail(IRIS_ERR_ARG, std::string(who) + ": null scene");
    if (s->dev.layout != kLayoutQ8) return fail(IRIS_ERR_ARG, std::string(who) + ": the distance query reads the quantised node table (IRIS_BVH4_Q8, the default layout)");
    return IRIS_OK;
}
extern "C" IRIS_API int iris_closest_point(const iris_scene* s, const float* xs, int64_t B, int64_t* tri, float* bary, float* pos, float* dist2, iris_stream_t stream) {
    if (int rc = closest_scene_check("iris_closest_point", s)) return rc;
    if (B < 0 || (B > 0 && !xs)) return fail(IRIS_ERR_ARG, "iris_closest_point: bad arguments");
    if (B == 0) return IRIS_OK;
    hipLaunchKernelGGL(closest_point_kernel, trace_grid(B), dim3(kBlock), 0, (hipStream_t)stream, s->dev, xs, B, tri, bary, pos, dist2);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
static int tex_args(const char* who, const int32_t* ft, int64_t F, const float* vt, int64_t n_vt, const uint8_t* albedo_img, const uint8_t* rm_img, int32_t H, int32_t W,
                    int64_t B, const float* albedo, const float* rough, const float* metal, TexDev& t) {
    if (H < 1 || W < 1 || H > kUvMaxRes || W > kUvMaxRes || F < 0 || n_vt < 0 || B < 0)
        return fail(IRIS_ERR_ARG, std::string(who) + ": bad sizes (H " + std::to_string(H) + ", W " + std::to_string(W) + ", F " + std::to_string(F) + ", n_vt " +
                                      std::to_string(n_vt) + ", B " + std::to_string(B) + "): H and W in [1, 8192]");
    if (!albedo_img || !rm_img || (F > 0 && (!ft || !vt)) || (B > 0 && (!albedo || !rough || !metal)) || (uintptr_t)ft % 4 || (uintptr_t)vt % 4)
        return fail(IRIS_ERR_ARG, std::string(who) + ": null or misaligned pointer");
    t.ft = ft; t.vt = vt; t.albedo = albedo_img; t.rm = rm_img; t.F = F; t.n_vt = n_vt; t.H = (int)H; t.W = (int)W;
    return IRIS_OK;
}
extern "C" IRIS_API int iris_texture_sample(const int64_t* tri, const float* bary, int64_t B, const int32_t* ft, int64_t F, const float* vt, int64_t n_vt,
                                            const uint8_t* albedo_img, const uint8_t* rm_img, int32_t H, int32_t W, float* albedo, float* rough, float* metal,
                                            iris_stream_t stream) {
    TexDev t;
    if (int rc = tex_args("iris_texture_sample", ft, F, vt, n_vt, albedo_img, rm_img, H, W, B, albedo, rough, metal, t)) return rc;
    if (B == 0) return IRIS_OK;
    if (!tri || !bary || (uintptr_t)tri % 8 || (uintptr_t)bary % 4) return fail(IRIS_ERR_ARG, "iris_texture_sample: null or misaligned pointer");
    return launch1d(texture_sample_kernel, B, 4096, stream, t, tri, bary, B, albedo, rough, metal);
}
extern "C" IRIS_API int iris_texture_material(const iris_scene* s, const float* xs, int64_t B, const int32_t* ft, int64_t F, const float* vt, int64_t n_vt,
                                              const uint8_t* albedo_img, const uint8_t* rm_img, int32_t H, int32_t W, float* albedo, float* rough, float* metal,
                                              iris_stream_t stream) {
    if (int rc = closest_scene_check("iris_texture_material", s)) return rc;
    TexDev t;
    if (int rc = tex_args("iris_texture_material", ft, F, vt, n_vt, albedo_img, rm_img, H, W, B, albedo, rough, metal, t)) return rc;
    if (B == 0) return IRIS_OK;
    if (!xs) return fail(IRIS_ERR_ARG, "iris_texture_material: null positions");
    hipLaunchKernelGGL(texture_material_kernel, trace_grid(B), dim3(kBlock), 0, (hipStream_t)stream, s->dev, t, xs, B, albedo, rough, metal);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
// 5c-20: the trainable texture's float texels (iris_texmat.h)
static int texels_args(const char* who, const int64_t* tri, const float* bary, int64_t B, const int32_t* ft, int64_t F, const float* vt, int64_t n_vt, const float* texels,
                       int32_t H, int32_t W, const float* albedo, const float* rough, const float* metal, TexelsDev& t) {
    if (H < 1 || W < 1 || H > kUvMaxRes || W > kUvMaxRes || F < 0 || n_vt < 0 || B < 0)
        return fail(IRIS_ERR_ARG, std::string(who) + ": bad sizes (H " + std::to_string(H) + ", W " + std::to_string(W) + ", F " + std::to_string(F) + ", n_vt " +
                                      std::to_string(n_vt) + ", B " + std::to_string(B) + "): H and W in [1, 8192]");
    if (!texels || (F > 0 && (!ft || !vt)) || (B > 0 && (!tri || !bary || !albedo || !rough || !metal)) || (uintptr_t)ft % 4 || (uintptr_t)vt % 4 || (uintptr_t)texels % 4 ||
        (uintptr_t)tri % 8 || (uintptr_t)bary % 4 || (uintptr_t)albedo % 4 || (uintptr_t)rough % 4 || (uintptr_t)metal % 4)
        return fail(IRIS_ERR_ARG, std::string(who) + ": null or misaligned pointer");
    t.ft = ft; t.vt = vt; t.texels = texels; t.F = F; t.n_vt = n_vt; t.H = (int)H; t.W = (int)W;
    return IRIS_OK;
}
extern "C" IRIS_API int iris_texture_sample_f32(const int64_t* tri, const float* bary, int64_t B, const int32_t* ft, int64_t F, const float* vt, int64_t n_vt,
                                                const float* texels, int32_t H, int32_t W, float* albedo, float* rough, float* metal, iris_stream_t stream) {
    TexelsDev t;
    if (int rc = texels_args("iris_texture_sample_f32", tri, bary, B, ft, F, vt, n_vt, texels, H, W, albedo, rough, metal, t)) return rc;
    if (B == 0) return IRIS_OK;
    return launch1d(texture_sample_f32_kernel, B, 4096, stream, t, tri, bary, B, albedo, rough, metal);
}
extern "C" IRIS_API int iris_texture_sample_f32_bwd(const int64_t* tri, const float* bary, int64_t B, const int32_t* ft, int64_t F, const float* vt, int64_t n_vt,
                                                    const float* texels, int32_t H, int32_t W, const float* g_albedo, const float* g_rough, const float* g_metal,
                                                    float* g_texels, iris_stream_t stream) {
    TexelsDev t;
    if (int rc = texels_args("iris_texture_sample_f32_bwd", tri, bary, B, ft, F, vt, n_vt, texels, H, W, g_albedo, g_rough, g_metal, t)) return rc;
    if (!g_texels || (uintptr_t)g_texels % 4 || g_texels == texels) return fail(IRIS_ERR_ARG, "iris_texture_sample_f32_bwd: g_texels is null, misaligned or the texels themselves");
    if (B == 0) return IRIS_OK;
    return launch1d(texture_sample_f32_bwd_kernel, B, 4096, stream, t, tri, bary, B, g_albedo, g_rough, g_metal, g_texels);
}

__global__ void philox_kernel(uint64_t seed, uint64_t idx0, uint32_t stream_id, int64_t n, float* __restrict__ u2) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float a, b;
        philox_u2(seed, idx0 + (uint64_t)i, stream_id, a, b);
        u2[i * 2] = a; u2[i * 2 + 1] = b;
    }
}
extern "C" IRIS_API int iris_philox_u2(uint64_t seed, uint64_t idx0, uint32_t stream_id, int64_t n, float* u2, iris_stream_t stream) {
    if (n < 0 || (n > 0 && !u2)) return fail(IRIS_ERR_ARG, "iris_philox_u2: bad arguments");
    if (n == 0) return IRIS_OK;
    return launch1d(philox_kernel, n, 8192, stream, seed, idx0, stream_id, n, u2);
}

// ======================================================================================================
// a3..a7 fused bake kernels (iris_bake.h)
// ======================================================================================================
// Pixels per tile.  ~5000-ray tiles are the optimum at 1080p x SPP 128 (with 32-B slots: 8192 rays: 324 ms per view, 6144: 322, 5120: 319,
// 4096: 308, 3072: 314, 2048: 326; with today's 24-B slots 4096: 6.99, 5120: 7.04, 6144: 6.98 Grays/s): larger tiles push the workgroups' slot
// slabs out of the 256 MB Infinity Cache, smaller ones pay more low-utilisation drains (one per wave and tile).  The LDS ray list is sized for
// exactly that (kTileRays = 5120), which is what lets 7 workgroups share a CU.  Round 3 (watertight leaf test, phase threshold 12): 3072-ray tiles
// 7.37, 3584: 7.42, 4096: 7.50, 4608: 7.45, 5120: 7.43 Grays/s -> the default target is 4096 (spp above it still get kTileRays).
// iris_debug_set("tile_target_rays") overrides.
constexpr int kTileTarget = 4096;
static int tile_pixels(int spp) {
    const int target = g_opt_tile_target_rays > 0 ? (int)std::min<long long>(kTileRays, std::max<long long>(64, g_opt_tile_target_rays)) : kTileTarget;
    return std::max(1, std::min(kTileRays, std::max(target, spp)) / spp);
}
#ifndef IRIS_TILE_GRID
#define IRIS_TILE_GRID IRIS_TILE_WAVES
#endif
static int bake_grid_blocks() { return num_cus() * IRIS_TILE_GRID; }  // resident 256-thread workgroups per CU (VGPR- and LDS-bound)
static uint64_t stack_ovf_bytes() {
    return (uint64_t)bake_grid_blocks() * (kStackCapacity - IRIS_TILE_STACK) * kBlock * sizeof(uint32_t);
}

extern "C" IRIS_API int iris_bake_tile_max_spp(void) { return kTileRays; }
extern "C" IRIS_API uint64_t iris_bake_workspace_bytes(int64_t P, int spp, int specular) {
    if (spp < 1 || spp > kTileRays || P < 0) return 0;  // v1 kernel only
    // [256 B counters][blocks x kTileRays x (16|32) B per-ray slots]
    // (packing the pixel tensors into 48-B records was measured 7 % SLOWER than reading pos/nrm/wo directly: not done)
    // + [blocks x (96 - LDS depth) x 256 dwords: traversal-stack entries beyond the LDS part]   (specular sizing also serves iris_bake_view)
    const uint64_t blocks = (uint64_t)bake_grid_blocks();
    return 256 + blocks * kTileRays * (specular ? 2 : 1) * sizeof(float4) + stack_ovf_bytes();
}

static const float4* fused_tris(const iris_scene* sc, const iris_emitter* em, hipStream_t st);
static int bake_launch(bool spec, const iris_scene* sc, const iris_emitter* em, const iris_slf* slf, const float* pos, const float* nrm,
                       const float* wo, float rough, int64_t P, int spp, const float* u2, uint64_t seed, uint32_t stream_id,
                       const int32_t* pix_id, float* out0, float* out1, int64_t* tri_next, int64_t* src_next, uint64_t* stats, int variant,
                       void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    if (!sc || !em || !slf || P < 0 || spp < 1 || (P > 0 && (!pos || !nrm || !out0 || (spec && (!wo || !out1)))))
        return fail(IRIS_ERR_ARG, "iris_bake: bad arguments");
    if (variant < IRIS_BAKE_AUTO || variant > IRIS_BAKE_TILE_SORTED) return fail(IRIS_ERR_ARG, "iris_bake: unknown kernel variant");
    if (em->dev.nf != sc->info.n_triangles)      // eval_emitter indexes is_emitter / emitter_idx by the hit triangle (model/emitter.py:196-203)
        return fail(IRIS_ERR_ARG, "iris_bake: the emitter tables were built for a mesh with a different number of triangles than the scene");
    if (P == 0) return IRIS_OK;
    BakeArgs a{};
    a.sc = sc->dev; a.em = em->dev; a.slf = slf->dev;
    a.pos = pos; a.nrm = nrm; a.wo = wo; a.u2 = u2; a.pix_id = pix_id;
    a.P = P; a.spp = spp; a.seed = seed; a.stream_id = stream_id; a.rough = rough;
    a.out0 = out0; a.out1 = out1; a.tri_next = tri_next; a.src_next = src_next; a.stats = (unsigned long long*)stats;
    const uint64_t need = iris_bake_workspace_bytes(P, spp, spec ? 1 : 0);
    bool tiled = variant != IRIS_BAKE_PIXEL_PER_WAVE && need > 0 && workspace && workspace_bytes >= need;
    if (variant == IRIS_BAKE_TILE_SORTED && !tiled)
        return fail(IRIS_ERR_ARG, "iris_bake: the tile-sorted kernel needs spp <= iris_bake_tile_max_spp() and a workspace of iris_bake_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    if (tiled) {
        const int blocks = bake_grid_blocks();
        int tile_px = tile_pixels(spp);                      // ~4096 rays per tile (at most what fits the LDS ray list) ...
        int tiles_per_block = 4;                             // ... but at least ~4 tiles per workgroup, so that the dynamic tile queue
        if (g_opt_tiles_per_block > 0) tiles_per_block = (int)g_opt_tiles_per_block;                  // balances (iris_debug_set("tiles_per_block"))
        const int64_t even = (P + (int64_t)blocks * tiles_per_block - 1) / ((int64_t)blocks * tiles_per_block);
        if (even < tile_px) tile_px = (int)std::max<int64_t>(even, std::min(tile_px, 16));   // not below 16 px: the sort needs rays
        if (tile_px < 1) tile_px = 1;
        a.tile_px = tile_px;
        a.tile_counter = (unsigned int*)workspace;
        a.scratch = (float4*)((char*)workspace + 256);
        a.stack_ovf = (uint32_t*)((char*)workspace + need - stack_ovf_bytes());
        HIP_TRY(hipMemsetAsync(workspace, 0, 256, st));
        if (const float4* ft = fused_tris(sc, em, st)) { a.sc.tris = ft; a.em.emit_ord = nullptr; }      // (tile kernels only: their shading pass reads the ordinal from the record)
        const int64_t n_tiles = (P + tile_px - 1) / tile_px;
        const int grid = (int)std::min<int64_t>(blocks, n_tiles);
        with_bake(spec, stats != nullptr, a.sc, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((bake_tile_kernel<T::spec, T::stats, T::layout>), dim3(grid), dim3(kBlock), 0, st, a);
        });
    } else {
        const int ppw = (spp < 64 && (spp & (spp - 1)) == 0) ? 64 / spp : 1;
        const int64_t n_groups = (P + ppw - 1) / ppw;
        const int grid = grid_for(n_groups * 64, kBlock, num_cus() * 6);
        with_bake(spec, stats != nullptr, a.sc, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((bake_kernel<T::spec, T::stats, T::layout>), dim3(grid), dim3(kBlock), 0, st, a);
        });
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
// All lobes of a view in one launch (see bake_view_kernel).  roughness[l] < 0 selects the diffuse lobe.
__global__ void fuse_ord_kernel(const float4* __restrict__ src, const int32_t* __restrict__ emit_ord, int64_t n_records, float4* __restrict__ dst) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_records; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 x = src[i * 4], y = src[i * 4 + 1], z = src[i * 4 + 2];
        const int id = __float_as_int(x.w);
        const int ord = id >= 0 ? emit_ord[id] : -1;              // (the degenerate record unused child slots point to carries id -1)
        dst[i * 4] = x; dst[i * 4 + 1] = y; dst[i * 4 + 2] = z; dst[i * 4 + 3] = make_float4(__int_as_float(ord), 0.f, 0.f, 0.f);
    }
}
// the scene's leaf records with the emitter's ordinals in the fourth plane; NULL when they cannot be had (memory): the caller then keeps the plain table + the ordinal gather
static const float4* fused_tris(const iris_scene* sc, const iris_emitter* em, hipStream_t st) {
    if (IRIS_NO_FUSED_RECORDS) return nullptr;
    std::lock_guard<std::mutex> lock(em->fused_mu);
    for (auto& f : em->fused) if (f.scene_uid == sc->uid) {
        // the table is filled by a kernel on the stream of the call that built it: a call on another stream waits for that kernel ON THE DEVICE (no host
        // synchronisation inside a bake call -- legal under stream capture) until the event has been seen complete once
        if (!f.done) {
            if (hipEventQuery(f.ready.ev) == hipSuccess) f.done = true;
            else { (void)hipGetLastError(); if (hipStreamWaitEvent(st, f.ready.ev, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; } }
        }
        return (const float4*)f.d_tris.p;
    }
    if (em->fused.size() >= 2) { em->retired.push_back(std::move(em->fused.front())); em->fused.erase(em->fused.begin()); }      // (a training loop uses one scene: the live set stays at two)
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(sc->device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }     // allocate where the scene lives, whatever the caller's current device
    DevBuf d; DevEvent ev;
    const int64_t n_rec = (int64_t)sc->dev.n_tris + 1;
    bool ok = d.alloc((size_t)n_rec * kLeafRecordBytes) == hipSuccess && ev.create() == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(fuse_ord_kernel, dim3(grid_for(n_rec, 256, 4096)), dim3(256), 0, st, sc->dev.tris, em->dev.emit_ord, n_rec, (float4*)d.p);
        ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev, st) == hipSuccess;
    }
    (void)hipSetDevice(prev);
    if (!ok) { (void)hipGetLastError(); return nullptr; }
    em->fused.push_back({sc->uid, std::move(d), std::move(ev), false});
    return (const float4*)em->fused.back().d_tris.p;            // (this call's own launch follows the fill on the same stream)
}
extern "C" IRIS_API int iris_bake_view(const iris_scene* sc, const iris_emitter* em, const iris_slf* slf, const float* pos, const float* nrm,
                              const float* wo, const int32_t* pix_id, int64_t P, int n_lobes, const float* roughness, const int32_t* spp,
                              const uint32_t* stream_ids, uint64_t seed, float* const* out0, float* const* out1, void* workspace,
                              uint64_t workspace_bytes, iris_stream_t stream) {
    if (!sc || !em || !slf || P < 0 || n_lobes < 1 || n_lobes > kMaxLobes || !roughness || !spp || !stream_ids || !out0 || !out1 ||
        (P > 0 && (!pos || !nrm || !wo)))
        return fail(IRIS_ERR_ARG, "iris_bake_view: bad arguments");
    if (em->dev.nf != sc->info.n_triangles)
        return fail(IRIS_ERR_ARG, "iris_bake_view: the emitter tables were built for a mesh with a different number of triangles than the scene");
    if (P == 0) return IRIS_OK;
    const uint64_t need = iris_bake_workspace_bytes(P, 1, 1);
    if (!workspace || workspace_bytes < need) return fail(IRIS_ERR_ARG, "iris_bake_view: workspace of iris_bake_workspace_bytes() bytes required");
    ViewArgs v{};
    v.base.sc = sc->dev; v.base.em = em->dev; v.base.slf = slf->dev;
    if (const float4* ft = fused_tris(sc, em, (hipStream_t)stream)) { v.base.sc.tris = ft; v.base.em.emit_ord = nullptr; }      // the shading pass reads the ordinal from the record
    v.base.pos = pos; v.base.nrm = nrm; v.base.wo = wo; v.base.pix_id = pix_id; v.base.P = P; v.base.seed = seed;
    v.base.tile_counter = (unsigned int*)workspace;
    v.base.scratch = (float4*)((char*)workspace + 256);
    v.base.stack_ovf = (uint32_t*)((char*)workspace + need - stack_ovf_bytes());
    v.n_lobes = n_lobes;
    const int blocks = bake_grid_blocks();
    long long t = 0;
    int tile_px_min = kTileRays;
    for (int l = 0; l < n_lobes; ++l) {
        if (spp[l] < 1 || spp[l] > kTileRays) return fail(IRIS_ERR_ARG, "iris_bake_view: spp must be in [1, iris_bake_tile_max_spp()]");
        if (!out0[l] || (roughness[l] >= 0.f && !out1[l])) return fail(IRIS_ERR_ARG, "iris_bake_view: null output");
        int tile_px = tile_pixels(spp[l]);
        const int64_t even = (P * n_lobes + (int64_t)blocks * 4 - 1) / ((int64_t)blocks * 4);   // >= ~4 tiles per workgroup over the whole view
        if (even < tile_px) tile_px = (int)std::max<int64_t>(even, std::min(tile_px, 16));
        if (tile_px < 1) tile_px = 1;
        v.lobe[l].rough = roughness[l]; v.lobe[l].spp = spp[l]; v.lobe[l].stream_id = stream_ids[l]; v.lobe[l].spec = roughness[l] >= 0.f ? 1 : 0;
        v.lobe[l].tile_px = tile_px; v.lobe[l].out0 = out0[l]; v.lobe[l].out1 = out1[l];
        tile_px_min = std::min(tile_px_min, tile_px);
        t += (P + tile_px - 1) / tile_px;
    }
    // the queue's virtual numbering (ViewArgs): spans of kTileChunk tiles of the lobe with the smallest tiles
    v.span_px = kTileChunk * tile_px_min;
    for (int l = 0; l < n_lobes; ++l) v.lobe[l].tiles_per_span = (v.span_px + v.lobe[l].tile_px - 1) / v.lobe[l].tile_px;
    const long long n_spans = (P + v.span_px - 1) / v.span_px;
    hipStream_t st = (hipStream_t)stream;
    v.n_tiles = ((n_spans + 7) / 8) * 8 * n_lobes * kTileChunk;
    HIP_TRY(hipMemsetAsync(workspace, 0, 256, st));
    const int grid = (int)std::min<long long>(blocks, t);
    with_layout(v.base.sc, [&](auto t) { hipLaunchKernelGGL(bake_view_kernel<decltype(t)::layout>, dim3(grid), dim3(kBlock), 0, st, v); });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_bake_diffuse(const iris_scene* sc, const iris_emitter* em, const iris_slf* slf, const float* pos, const float* nrm,
                                 int64_t P, int spp, const float* u2, uint64_t seed, uint32_t stream_id, const int32_t* pix_id,
                                 float* Ld, int64_t* tri_next, void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    return bake_launch(false, sc, em, slf, pos, nrm, nullptr, -1.f, P, spp, u2, seed, stream_id, pix_id, Ld, nullptr, tri_next, nullptr, nullptr,
                       IRIS_BAKE_AUTO, workspace, workspace_bytes, stream);
}
extern "C" IRIS_API int iris_bake_specular(const iris_scene* sc, const iris_emitter* em, const iris_slf* slf, const float* pos, const float* nrm,
                                  const float* wo, float roughness, int64_t P, int spp, const float* u2, uint64_t seed,
                                  uint32_t stream_id, const int32_t* pix_id, float* Ls0, float* Ls1, int64_t* tri_next,
                                  void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    return bake_launch(true, sc, em, slf, pos, nrm, wo, roughness, P, spp, u2, seed, stream_id, pix_id, Ls0, Ls1, tri_next, nullptr, nullptr,
                       IRIS_BAKE_AUTO, workspace, workspace_bytes, stream);
}
// diagnostics twins (iris_hip_debug.h): kernel variant, instrumented build, per-sample source rows
extern "C" IRIS_API int iris_debug_bake_diffuse(const iris_scene* sc, const iris_emitter* em, const iris_slf* slf, const float* pos, const float* nrm,
                                       int64_t P, int spp, const float* u2, uint64_t seed, uint32_t stream_id, const int32_t* pix_id,
                                       float* Ld, int64_t* tri_next, int64_t* src_next, uint64_t* stats, int variant, void* workspace,
                                       uint64_t workspace_bytes, iris_stream_t stream) {
    return bake_launch(false, sc, em, slf, pos, nrm, nullptr, -1.f, P, spp, u2, seed, stream_id, pix_id, Ld, nullptr, tri_next, src_next, stats, variant,
                       workspace, workspace_bytes, stream);
}
extern "C" IRIS_API int iris_debug_bake_specular(const iris_scene* sc, const iris_emitter* em, const iris_slf* slf, const float* pos, const float* nrm,
                                        const float* wo, float roughness, int64_t P, int spp, const float* u2, uint64_t seed,
                                        uint32_t stream_id, const int32_t* pix_id, float* Ls0, float* Ls1, int64_t* tri_next, int64_t* src_next,
                                        uint64_t* stats, int variant, void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    return bake_launch(true, sc, em, slf, pos, nrm, wo, roughness, P, spp, u2, seed, stream_id, pix_id, Ls0, Ls1, tri_next, src_next, stats, variant,
                       workspace, workspace_bytes, stream);
}

#ifdef IRIS_PHASE_TIMING
// diagnostic build only (tools/diag_phases.py): read / reset the per-phase cycle sums of the tile kernels
extern "C" IRIS_API int iris_debug_phase_cycles(unsigned long long* out8, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    if (out8) HIP_TRY(hipMemcpyFromSymbol(out8, HIP_SYMBOL(iris::g_phase_cycles), 64));
    if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(iris::g_phase_cycles), z, 64)); }
    return IRIS_OK;
}
#endif

// ======================================================================================================
// a9 (cfg 5): path_tracing_single building blocks and stages (iris_pt.h)
// ======================================================================================================
// Large batches go through the direction-sorted, persistent-lane tile kernel (iris_pt.h); small ones (cfg 5: 262 144 rays) keep the
// one-ray-per-thread kernels, which expose more parallelism.  iris_debug_set("pt_tile_min") overrides the switch-over (tests force the tile path).
static bool pt_tiling(int64_t N, int& tile_rays, int& grid) {
    const int64_t blocks = (int64_t)num_cus() * IRIS_PT_WAVES;
    int64_t min_n = 512 * blocks;
    if (g_opt_pt_tile_min >= 0) min_n = g_opt_pt_tile_min;
    if (N < min_n) return false;
    int64_t t = (N / (2 * blocks) + kBlock - 1) / kBlock * kBlock;          // >= 2 tiles per resident workgroup ...
    tile_rays = (int)std::min<int64_t>(kPtTileCap, std::max<int64_t>(kBlock, t));   // ... of 256 .. 4096 rays
    grid = (int)std::min<int64_t>(blocks, (N + tile_rays - 1) / tile_rays);
    return true;
}
extern "C" IRIS_API int iris_sample_emitter(const iris_emitter* e, const float* s1, const float* s2, const float* position, int64_t N, float* wi,
                                   float* pdf, int64_t* tri, iris_stream_t stream) {
    if (!e || !e->can_sample) return fail(IRIS_ERR_ARG, "iris_sample_emitter: emitter was created without vertices / cdf");
    if (N < 0 || (N > 0 && (!s1 || !s2 || !position || !wi || !pdf || !tri))) return fail(IRIS_ERR_ARG, "iris_sample_emitter: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(sample_emitter_kernel, N, 8192, stream, e->sample, s1, s2, position, N, wi, pdf, tri);
}
extern "C" IRIS_API int iris_eval_brdf(const float* wi, const float* wo, const float* normal, const float* albedo, const float* roughness,
                              const float* metallic, int64_t N, float* brdf, float* pdf, iris_stream_t stream) {
    if (N < 0 || (N > 0 && (!wi || !wo || !normal || !albedo || !roughness || !metallic || !brdf || !pdf))) return fail(IRIS_ERR_ARG, "iris_eval_brdf: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(eval_brdf_kernel, N, 8192, stream, wi, wo, normal, albedo, roughness, metallic, N, brdf, pdf);
}
extern "C" IRIS_API int iris_sample_brdf(const float* s1, const float* s2, const float* wo, const float* normal, const float* albedo,
                                const float* roughness, const float* metallic, int64_t N, float* wi, float* pdf, float* weight,
                                iris_stream_t stream) {
    if (N < 0 || (N > 0 && (!s1 || !s2 || !wo || !normal || !albedo || !roughness || !metallic || !wi || !pdf || !weight)))
        return fail(IRIS_ERR_ARG, "iris_sample_brdf: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(sample_brdf_kernel, N, 8192, stream, s1, s2, wo, normal, albedo, roughness, metallic, N, wi, pdf, weight);
}
extern "C" IRIS_API int iris_pt_jitter(const float* rays_d, const float* dxdu, const float* dydv, const float* dudv, int64_t B, int spp, float* wi,
                              iris_stream_t stream) {
    if (B < 0 || spp < 1 || (B > 0 && (!rays_d || !dxdu || !dydv || !dudv || !wi))) return fail(IRIS_ERR_ARG, "iris_pt_jitter: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(pt_jitter_kernel, B * spp, 8192, stream, rays_d, dxdu, dydv, dudv, B, spp, wi);
}
__global__ void pt_primary_emit_kernel(EmitDev e, const int64_t* __restrict__ tri, int64_t N, int32_t* __restrict__ e0, uint8_t* __restrict__ valid_next) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const bool vis = tri[i] != -1;
        const int ord = vis ? e.emit_ord[tri[i]] : -1;
        e0[i] = ord;
        valid_next[i] = (vis && ord < 0) ? 1 : 0;
    }
}
extern "C" IRIS_API int iris_pt_primary_emit(const iris_emitter* e, const int64_t* tri, int64_t N, int32_t* e0, uint8_t* valid_next, iris_stream_t stream) {
    if (!e || N < 0 || (N > 0 && (!tri || !e0 || !valid_next))) return fail(IRIS_ERR_ARG, "iris_pt_primary_emit: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(pt_primary_emit_kernel, N, 8192, stream, e->dev, tri, N, e0, valid_next);
}
// The head of path_tracing_single's un-compacted mode as ONE launch (round 5): :338-340 jitter -> :343 ray_intersect(rays_o.repeat_interleave(spp), wi) -> :344 the primary hit's
// emitter ordinal -> which paths continue (path_of) -> wo = -wi.  The same arithmetic as iris_pt_jitter + iris_intersect + iris_pt_primary_emit and the torch glue between them
// (repeat_interleave, where, neg): six launches of a 0.5 ms call.
template <int LAYOUT, bool JOINT>
__global__ __launch_bounds__(kBlock) void pt_primary_kernel(SceneDev sc, EmitDev em, const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ dxdu,
                                                            const float* __restrict__ dydv, const float* __restrict__ dudv, float jitter_offset, int64_t B, int spp, float* __restrict__ wi_out,
                                                            float* __restrict__ wo_out, float* __restrict__ pos, float* __restrict__ nrm, int32_t* __restrict__ e0,
                                                            uint8_t* __restrict__ valid_next, int32_t* __restrict__ path_of) {
    __shared__ uint32_t s_stack[kStackLds * kBlock];
    const int64_t n = B * spp;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = i / spp;
        const f3 d = pt_jitter_dir(ld3(rays_d + b * 3), ld3(dxdu + b * 3), ld3(dydv + b * 3), dudv[i], dudv[n + i], jitter_offset);   // pt_jitter_kernel (0.5), render.py:180 (0)
        const f3 o = ld3(rays_o + b * 3);
        st3(wi_out + i * 3, d); st3(wo_out + i * 3, mk3(-d.x, -d.y, -d.z));
        const Hit h = trace_bvh4<LAYOUT, false, kStackLds, false, JOINT>(sc, o, d, s_stack + threadIdx.x);
        int ord = -1;
        if (h.slot >= 0) {                                                         // intersect_kernel's outputs
            f3 p0, p1, p2;
            hit_vertices(sc, h, p0, p1, p2);
            st3(pos + i * 3, hit_position(h, p0, p1, p2));
            f3 nn = t_normalize(hit_normal(p0, p1, p2));
            if (t_dot(nn, mk3(-d.x, -d.y, -d.z)) < 0.f) nn = mk3(-nn.x, -nn.y, -nn.z);
            st3(nrm + i * 3, nn);
            ord = em.emit_ord[h.id];                                               // pt_primary_emit_kernel
        } else {
            st3(pos + i * 3, mk3(0.f, 0.f, 0.f)); st3(nrm + i * 3, mk3(0.f, 0.f, 0.f));
        }
        const bool cont = h.slot >= 0 && ord < 0;
        e0[i] = ord; valid_next[i] = cont ? 1 : 0;
        if (path_of) path_of[i] = cont ? (int32_t)i : -1;                          // (iris_render_primary has no use for it)
    }
}
static int pt_primary_launch(const iris_scene* sc, const iris_emitter* e, const float* rays_o, const float* rays_d, const float* dxdu, const float* dydv, const float* dudv,
                             float jitter_offset, int64_t B, int spp, float* wi, float* wo, float* pos, float* nrm, int32_t* e0, uint8_t* valid_next, int32_t* path_of,
                             iris_stream_t stream) {
    const int64_t N = B * spp;
    const dim3 grid = trace_grid(N);
    with_trace(sc->dev, N, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pt_primary_kernel<T::layout, T::joint>), grid, dim3(kBlock), 0, (hipStream_t)stream, sc->dev, e->dev, rays_o, rays_d, dxdu, dydv, dudv, jitter_offset, B, spp, wi, wo, pos, nrm, e0, valid_next, path_of);
    });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_pt_primary(const iris_scene* sc, const iris_emitter* e, const float* rays_o, const float* rays_d, const float* dxdu, const float* dydv,
                               const float* dudv, int64_t B, int spp, float* wi, float* wo, float* pos, float* nrm, int32_t* e0, uint8_t* valid_next, int32_t* path_of,
                               iris_stream_t stream) {
    if (!sc || !e || B < 0 || spp < 1 || (B > 0 && (!rays_o || !rays_d || !dxdu || !dydv || !dudv || !wi || !wo || !pos || !nrm || !e0 || !valid_next || !path_of)))
        return fail(IRIS_ERR_ARG, "iris_pt_primary: bad arguments");
    if (B == 0) return IRIS_OK;
    if (B * spp >= ((int64_t)1 << 31)) return fail(IRIS_ERR_ARG, "iris_pt_primary: more than 2^31 paths in one call (path_of is int32)");
    if (e->dev.nf != sc->info.n_triangles) return fail(IRIS_ERR_ARG, "iris_pt_primary: the emitter tables are for a mesh of another size than the scene's");
    return pt_primary_launch(sc, e, rays_o, rays_d, dxdu, dydv, dudv, 0.5f, B, spp, wi, wo, pos, nrm, e0, valid_next, path_of, stream);
}
// render.py:179-184 + the primary hit's emitter ordinal: iris_pt_primary's kernel with render.py's jitter (du, dv in [0,1), no -0.5) and without path_of
extern "C" IRIS_API int iris_render_primary(const iris_scene* sc, const iris_emitter* e, const float* rays_o, const float* rays_d, const float* dxdu, const float* dydv,
                                   const float* dudv, int64_t B, int spp, float* wi, float* wo, float* pos, float* nrm, int32_t* e0, uint8_t* valid_next,
                                   iris_stream_t stream) {
    if (!sc || !e || B < 0 || spp < 1 || (B > 0 && (!rays_o || !rays_d || !dxdu || !dydv || !dudv || !wi || !wo || !pos || !nrm || !e0 || !valid_next)))
        return fail(IRIS_ERR_ARG, "iris_render_primary: bad arguments");
    if (B == 0) return IRIS_OK;
    if (B > (((int64_t)1 << 40) / spp)) return fail(IRIS_ERR_ARG, "iris_render_primary: more than 2^40 samples in one call");
    if (e->dev.nf != sc->info.n_triangles) return fail(IRIS_ERR_ARG, "iris_render_primary: the emitter tables are for a mesh of another size than the scene's");
    return pt_primary_launch(sc, e, rays_o, rays_d, dxdu, dydv, dudv, 0.0f, B, spp, wi, wo, pos, nrm, e0, valid_next, nullptr, stream);
}
// render.py:189-220 after the material network (iris_render.h)
extern "C" IRIS_API int iris_render_intrinsics(const iris_emitter* e, const iris_slf* slf, const float* radiance, const float* pos, const float* nrm, const float* wo,
                                      const int32_t* e0, const uint8_t* valid_next, const float* albedo, const float* roughness, const float* metallic,
                                      const float* u2, int64_t B, int spp, float* kd, float* a_prime, float* roughness_map, float* metallic_map, float* emission,
                                      float* slf_map, iris_stream_t stream) {
    if (!e || !slf || B < 0 || spp < 1 ||
        (B > 0 && (!radiance || !pos || !nrm || !wo || !e0 || !valid_next || !albedo || !roughness || !metallic || !u2 || !kd || !a_prime || !roughness_map ||
                   !metallic_map || !emission || !slf_map)))
        return fail(IRIS_ERR_ARG, "iris_render_intrinsics: bad arguments");
    if (B == 0) return IRIS_OK;
    if (B > (((int64_t)1 << 40) / spp)) return fail(IRIS_ERR_ARG, "iris_render_intrinsics: more than 2^40 samples in one call");
    RenderArgs a{};
    a.slf = slf->dev; a.radiance = radiance; a.n_rad = e->n_rad; a.B = B; a.spp = spp;
    a.pos = pos; a.nrm = nrm; a.wo = wo; a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.u2 = u2; a.e0 = e0; a.valid_next = valid_next;
    a.kd = kd; a.a_prime = a_prime; a.roughness = roughness_map; a.metallic = metallic_map; a.emission = emission; a.slf_out = slf_map;
    int lpp = 1;
    while (lpp < spp && lpp < 64) lpp <<= 1;                     // lanes per pixel: min(64, next power of two >= spp), as iris_pt_accumulate_fwd
    a.lpp = lpp;
    const int64_t n_groups = (B + 64 / lpp - 1) / (64 / lpp);    // one wave per group of 64 / lpp pixels
    return launch1d(render_intrinsics_kernel, n_groups * 64, 16384, stream, a);
}
// validation()'s material maps after the material network (iris_validate.h; train_brdf_crf.py:372-396)
extern "C" IRIS_API int iris_val_intrinsics(const iris_emitter* e, const float* radiance, const int32_t* e0, const uint8_t* valid_next, const float* albedo,
                                   const float* roughness, const float* metallic, int64_t B, int spp, float* albedo_map, float* roughness_map,
                                   float* metallic_map, float* emission, iris_stream_t stream) {
    if (!e || B < 0 || spp < 1 ||
        (B > 0 && (!radiance || !e0 || !valid_next || !albedo || !roughness || !metallic || !albedo_map || !roughness_map || !metallic_map || !emission)))
        return fail(IRIS_ERR_ARG, "iris_val_intrinsics: bad arguments");
    if (B == 0) return IRIS_OK;
    if (B > (((int64_t)1 << 40) / spp)) return fail(IRIS_ERR_ARG, "iris_val_intrinsics: more than 2^40 samples in one call");
    ValMapsArgs a{};
    a.radiance = radiance; a.n_rad = e->n_rad; a.B = B; a.spp = spp;
    a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.e0 = e0; a.valid_next = valid_next;
    a.albedo_map = albedo_map; a.roughness = roughness_map; a.metallic = metallic_map; a.emission = emission;
    int lpp = 1;
    while (lpp < spp && lpp < 64) lpp <<= 1;                     // lanes per pixel, as iris_render_intrinsics
    a.lpp = lpp;
    const int64_t n_groups = (B + 64 / lpp - 1) / (64 / lpp);    // one wave per group of 64 / lpp pixels
    return launch1d(val_intrinsics_kernel, n_groups * 64, 16384, stream, a);
}
extern "C" IRIS_API int iris_pt_nee(const iris_scene* sc, const iris_emitter* e, const float* pos, const float* nrm, const float* wo, const float* albedo,
                           const float* roughness, const float* metallic, const float* s1, const float* s2, int64_t N, float* coef1, int32_t* e1,
                           float g_eps, float pdf_eps, float mis_eps, iris_stream_t stream) {
    if (!sc || !e || !e->can_sample) return fail(IRIS_ERR_ARG, "iris_pt_nee: scene / emitter (with vertices + cdf) required");
    if (N < 0 || (N > 0 && (!pos || !nrm || !wo || !albedo || !roughness || !metallic || !s1 || !s2 || !coef1 || !e1))) return fail(IRIS_ERR_ARG, "iris_pt_nee: bad arguments");
    if (N == 0) return IRIS_OK;
    PtArgs a{};
    a.sc = sc->dev; a.em = e->dev; a.es = e->sample; a.N = N;
    a.pos = pos; a.nrm = nrm; a.wo = wo; a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.s1 = s1; a.s2 = s2;
    a.coef1 = coef1; a.e1 = e1; a.g_eps = g_eps; a.pdf_eps = pdf_eps; a.mis_eps = mis_eps;
    int tile_rays, grid;
    if (pt_tiling(N, tile_rays, grid))
        with_layout(a.sc, [&](auto t) { hipLaunchKernelGGL((pt_tiled_kernel<decltype(t)::layout, true>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, tile_rays); });
    else
        with_trace(a.sc, N, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((pt_nee_kernel<T::layout, T::joint>), trace_grid(N), dim3(kBlock), 0, (hipStream_t)stream, a);
        });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_pt_brdf_trace(const iris_scene* sc, const float* pos, const float* nrm, const float* wo, const float* albedo,
                                  const float* roughness, const float* metallic, const float* s1, const float* s2, int64_t N, float* wi,
                                  float* pdf, float* weight, float* pos_next, float* nrm_next, int64_t* tri_next, uint8_t* valid,
                                  int lobe, float lobe_roughness, iris_stream_t stream) {
    if (!sc || N < 0 || lobe < 0 || lobe > 2 ||
        (N > 0 && (!pos || !nrm || !wo || !s2 || !wi || !pdf || !weight || !pos_next || !nrm_next || !tri_next || !valid ||
                   (lobe == 0 && (!albedo || !roughness || !metallic || !s1)))))
        return fail(IRIS_ERR_ARG, "iris_pt_brdf_trace: bad arguments");
    if (N == 0) return IRIS_OK;
    PtArgs a{};
    a.sc = sc->dev; a.N = N;
    a.pos = pos; a.nrm = nrm; a.wo = wo; a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.s1 = s1; a.s2 = s2;
    a.wi_out = wi; a.brdf_pdf = pdf; a.brdf_w = weight; a.pos_next = pos_next; a.nrm_next = nrm_next; a.tri_next = tri_next; a.valid_next_hit = valid;
    a.lobe = lobe; a.lobe_rough = lobe_roughness;
    int tile_rays, grid;
    if (pt_tiling(N, tile_rays, grid))
        with_layout(a.sc, [&](auto t) { hipLaunchKernelGGL((pt_tiled_kernel<decltype(t)::layout, false>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, tile_rays); });
    else
        with_trace(a.sc, N, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((pt_brdf_trace_kernel<T::layout, T::joint>), trace_grid(N), dim3(kBlock), 0, (hipStream_t)stream, a);
        });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
// Both tracing stages of a bounce in one launch (see pt_bounce_kernel); calls below the tiling threshold run the two stages one after the other.
extern "C" IRIS_API int iris_pt_bounce(const iris_scene* sc, const iris_emitter* e, const float* pos, const float* nrm, const float* wo, const float* albedo,
                              const float* roughness, const float* metallic, const float* s1, const float* s2, const float* s1b, const float* s2b, int64_t N,
                              float* coef1, int32_t* e1, float g_eps, float pdf_eps, float mis_eps, float* wi, float* pdf, float* weight, float* pos_next,
                              float* nrm_next, int64_t* tri_next, uint8_t* valid, iris_stream_t stream) {
    if (!sc || !e || !e->can_sample) return fail(IRIS_ERR_ARG, "iris_pt_bounce: scene / emitter (with vertices + cdf) required");
    if (N < 0 || (N > 0 && (!pos || !nrm || !wo || !albedo || !roughness || !metallic || !s1 || !s2 || !s1b || !s2b || !coef1 || !e1 || !wi || !pdf || !weight || !pos_next ||
                            !nrm_next || !tri_next || !valid)))
        return fail(IRIS_ERR_ARG, "iris_pt_bounce: bad arguments");
    if (N == 0) return IRIS_OK;
    int tile_rays, grid, t1 = 0, g1 = 0;
    // Together when that makes the tiles LARGER (a reference-size batch of refine_shading, 1.3 M paths, has 512-ray tiles per stage: 111.7 -> 120.4 Mpaths/s); a call whose
    // stages already run full 4096-ray tiles each gains nothing from mixing the two ray kinds in a tile (measured -3.4 % at 21 M paths) and keeps the two launches.
    const bool full_tiles_already = pt_tiling(N, t1, g1) && t1 >= kPtTileCap;
    if (full_tiles_already || !pt_tiling(2 * N, tile_rays, grid)) {
        int rc = iris_pt_nee(sc, e, pos, nrm, wo, albedo, roughness, metallic, s1, s2, N, coef1, e1, g_eps, pdf_eps, mis_eps, stream);
        if (rc != IRIS_OK) return rc;
        return iris_pt_brdf_trace(sc, pos, nrm, wo, albedo, roughness, metallic, s1b, s2b, N, wi, pdf, weight, pos_next, nrm_next, tri_next, valid, 0, 0.0f, stream);
    }
    PtArgs a{};
    a.sc = sc->dev; a.em = e->dev; a.es = e->sample; a.N = N;
    a.pos = pos; a.nrm = nrm; a.wo = wo; a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.s1 = s1; a.s2 = s2; a.s1b = s1b; a.s2b = s2b;
    a.coef1 = coef1; a.e1 = e1; a.g_eps = g_eps; a.pdf_eps = pdf_eps; a.mis_eps = mis_eps;
    a.wi_out = wi; a.brdf_pdf = pdf; a.brdf_w = weight; a.pos_next = pos_next; a.nrm_next = nrm_next; a.tri_next = tri_next; a.valid_next_hit = valid;
    a.lobe = 0; a.lobe_rough = 0.f;
    const int tile_paths = std::max(kBlock / 2, tile_rays / 2);
    const int64_t n_tiles = (N + tile_paths - 1) / tile_paths;
    const int g2 = (int)std::min<int64_t>((int64_t)num_cus() * IRIS_PT_WAVES, n_tiles);
    with_layout(a.sc, [&](auto t) { hipLaunchKernelGGL((pt_bounce_kernel<decltype(t)::layout>), dim3(g2), dim3(kBlock), 0, (hipStream_t)stream, a, tile_paths); });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_pt_brdf_finish(const iris_emitter* e, const iris_slf* slf, const float* pos, const float* pos_next, const float* nrm_next,
                                   const float* wi, const int64_t* tri_next, const float* roughness_next, const float* pdf, const float* weight,
                                   int64_t N, float* coef2, float* const2, int32_t* e2, uint8_t* valid_next, float trace_roughness, float g_eps,
                                   iris_stream_t stream) {
    const bool slf_unreachable = roughness_next && std::isinf(trace_roughness) && trace_roughness > 0.f;      // (no roughness exceeds +inf: the cache may be NULL)
    if (!e || (!slf && !slf_unreachable) || N < 0 || (N > 0 && (!pos || !pos_next || !nrm_next || !wi || !tri_next || !pdf || !weight || !coef2 || !const2 || !e2)))      // (roughness_next may be NULL: see iris_hip.h)
        return fail(IRIS_ERR_ARG, "iris_pt_brdf_finish: bad arguments");
    if (N == 0) return IRIS_OK;
    PtArgs a{};
    a.em = e->dev; a.slf = slf ? slf->dev : SlfDev{}; a.N = N;
    a.pos = pos; a.pos_n_in = pos_next; a.nrm_n_in = nrm_next; a.wi_in = wi; a.tri_n_in = tri_next; a.rough_next = roughness_next; a.pdf_in = pdf; a.w_in = weight;
    a.coef2 = coef2; a.const2 = const2; a.e2 = e2; a.valid_next_hit = valid_next; a.trace_rough = trace_roughness; a.g_eps = g_eps;
    return launch1d(pt_brdf_finish_kernel, N, 8192, stream, a);
}
extern "C" IRIS_API int iris_pt_accumulate_fwd(const float* radiance, const int32_t* e0, const int32_t* path_of, const int32_t* e1, const float* coef1,
                                      const int32_t* e2, const float* coef2, const float* const2, int64_t B, int spp, float* L,
                                      iris_stream_t stream) {
    if (B < 0 || spp < 1 || (B > 0 && (!radiance || !e0 || !path_of || !L))) return fail(IRIS_ERR_ARG, "iris_pt_accumulate_fwd: bad arguments");
    if (B == 0) return IRIS_OK;
    int lpp = 1;
    while (lpp < spp && lpp < 64) lpp <<= 1;                     // lanes per pixel: min(64, next power of two >= spp)
    const int64_t n_groups = (B + 64 / lpp - 1) / (64 / lpp);    // one wave per group of 64 / lpp pixels
    return launch1d(pt_accumulate_fwd_kernel, n_groups * 64, 8192, stream, radiance, e0, path_of, e1, coef1, e2, coef2, const2, B, spp, lpp, L);
}
extern "C" IRIS_API int iris_pt_accumulate_bwd(const float* gL, const int32_t* e0, const int32_t* path_of, const int32_t* e1, const float* coef1,
                                      const int32_t* e2, const float* coef2, int64_t B, int spp, float* g_radiance, iris_stream_t stream) {
    if (B < 0 || spp < 1 || (B > 0 && (!gL || !e0 || !path_of || !g_radiance))) return fail(IRIS_ERR_ARG, "iris_pt_accumulate_bwd: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(pt_accumulate_bwd_kernel, B * spp, 8192, stream, gL, e0, path_of, e1, coef1, e2, coef2, B, spp, g_radiance);
}
// The accumulation of a whole training step (n_calls calls on the same rays, paths pixel-major): see pt_step_accumulate_fwd_kernel for the summation order.
static bool pt_step_sizes_ok(int64_t B, int spp, int n_calls) {
    return B >= 0 && spp >= 1 && n_calls >= 1 && (int64_t)spp * n_calls < ((int64_t)1 << 31) && B * ((int64_t)spp * n_calls) < ((int64_t)1 << 31);   // (path_of is int32)
}
extern "C" IRIS_API int iris_pt_step_accumulate_fwd(const float* radiance, const int32_t* e0, const int32_t* path_of, const int32_t* e1, const float* coef1,
                                           const int32_t* e2, const float* coef2, const float* const2, int64_t B, int spp, int n_calls, float* L,
                                           iris_stream_t stream) {
    if (!pt_step_sizes_ok(B, spp, n_calls) || (B > 0 && (!radiance || !e0 || !path_of || !L))) return fail(IRIS_ERR_ARG, "iris_pt_step_accumulate_fwd: bad arguments");
    if (B == 0) return IRIS_OK;
    int lpp = 1;
    while (lpp < spp && lpp < 64) lpp <<= 1;                     // lanes per pixel, as iris_pt_accumulate_fwd
    const int64_t n_groups = (B + 64 / lpp - 1) / (64 / lpp);
    return launch1d(pt_step_accumulate_fwd_kernel, n_groups * 64, 8192, stream, radiance, e0, path_of, e1, coef1, e2, coef2, const2, B, spp, n_calls, lpp, L);
}
extern "C" IRIS_API int iris_pt_step_accumulate_bwd(const float* gL, const int32_t* e0, const int32_t* path_of, const int32_t* e1, const float* coef1,
                                           const int32_t* e2, const float* coef2, int64_t B, int spp, int n_calls, float* g_radiance, iris_stream_t stream) {
    if (!pt_step_sizes_ok(B, spp, n_calls) || (B > 0 && (!gL || !e0 || !path_of || !g_radiance))) return fail(IRIS_ERR_ARG, "iris_pt_step_accumulate_bwd: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(pt_step_accumulate_bwd_kernel, B * n_calls * spp, 8192, stream, gL, e0, path_of, e1, coef1, e2, coef2, B, spp, n_calls, g_radiance);
}

extern "C" IRIS_API int iris_pt_apply(float* L, const int32_t* rows, float* throughput, const float* radiance, const int32_t* e, const float* coef,
                             const float* cst, const float* weight, int64_t N, int nan_to_zero, iris_stream_t stream) {
    if (N < 0 || (N > 0 && (!L || (e && (!radiance || !coef))))) return fail(IRIS_ERR_ARG, "iris_pt_apply: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(pt_apply_kernel, N, 8192, stream, L, rows, throughput, radiance, e, coef, cst, weight, N, nan_to_zero);
}

extern "C" IRIS_API uint64_t iris_pt_compact_workspace_bytes(int64_t N) {
    return N <= 0 ? 0 : (uint64_t)((N + kCompactItems - 1) / kCompactItems) * sizeof(int32_t);
}
extern "C" IRIS_API int iris_pt_compact(const uint8_t* keep, int64_t N, int n3, const float* const* src3, float* const* dst3, uint32_t negate3, int n1,
                               const float* const* src1, float* const* dst1, int ni, const int32_t* const* srci, int32_t* const* dsti, int32_t* count,
                               void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    if (N < 0 || !count || n3 < 0 || n1 < 0 || ni < 0 || n3 > kCompactMax || n1 > kCompactMax || ni > kCompactMax || (N > 0 && (!keep || !workspace)) ||
        (n3 > 0 && (!src3 || !dst3)) || (n1 > 0 && (!src1 || !dst1)) || (ni > 0 && (!srci || !dsti)))
        return fail(IRIS_ERR_ARG, "iris_pt_compact: bad arguments");
    if (N >= ((int64_t)1 << 31)) return fail(IRIS_ERR_ARG, "iris_pt_compact: more than 2^31 rows");
    if (workspace_bytes < iris_pt_compact_workspace_bytes(N)) return fail(IRIS_ERR_ARG, "iris_pt_compact: workspace smaller than iris_pt_compact_workspace_bytes(N)");
    if (N == 0) { HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream)); return IRIS_OK; }
    CompactArgs a{};
    a.keep = keep; a.N = N; a.n3 = n3; a.n1 = n1; a.ni = ni; a.negate3 = negate3; a.block_counts = (int32_t*)workspace; a.count = count;
    for (int j = 0; j < n3; ++j) { if (!src3[j] || !dst3[j]) return fail(IRIS_ERR_ARG, "iris_pt_compact: null array"); a.src3[j] = src3[j]; a.dst3[j] = dst3[j]; }
    for (int j = 0; j < n1; ++j) { if (!src1[j] || !dst1[j]) return fail(IRIS_ERR_ARG, "iris_pt_compact: null array"); a.src1[j] = src1[j]; a.dst1[j] = dst1[j]; }
    for (int j = 0; j < ni; ++j) { if (!srci[j] || !dsti[j]) return fail(IRIS_ERR_ARG, "iris_pt_compact: null array"); a.srci[j] = srci[j]; a.dsti[j] = dsti[j]; }
    const int blocks = (int)((N + kCompactItems - 1) / kCompactItems);
    hipLaunchKernelGGL(pt_compact_count_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pt_compact_move_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// the relighting stage (iris_relight.h): surface classes, spot-light next-event estimation, the fused end of a bounce
// ======================================================================================================
static bool surf_args(const int32_t* surf, int64_t n_surf, const float* cmat, int n_cmat, SurfDev& sf) {
    if (n_surf < 0 || n_cmat < 0 || (n_surf > 0 && !surf) || (n_cmat > 0 && !cmat)) return false;
    sf.surf = n_surf > 0 ? surf : nullptr; sf.cmat = cmat; sf.nf = n_surf; sf.n_cmat = n_cmat;
    return true;
}
extern "C" IRIS_API int iris_relight_surface(const int32_t* surf, int64_t n_surf, const float* cmat, int n_cmat, const int64_t* tri, int64_t N, float* albedo,
                                    float* roughness, float* metallic, uint8_t* valid, iris_stream_t stream) {
    SurfDev sf{};
    if (!surf_args(surf, n_surf, cmat, n_cmat, sf) || N < 0 || (N > 0 && (!tri || (albedo && (!roughness || !metallic)) || (!albedo && !valid))))
        return fail(IRIS_ERR_ARG, "iris_relight_surface: bad arguments");
    if (N == 0) return IRIS_OK;
    return launch1d(relight_surface_kernel, N, 8192, stream, sf, tri, N, albedo, roughness, metallic, valid);
}
extern "C" IRIS_API int iris_pt_nee_spot(const iris_scene* sc, const float* pos, const float* nrm, const float* wo, const float* albedo, const float* roughness,
                                const float* metallic, const float* pick, const float* spots, int n_spots, int64_t N, float* coef, int32_t* e,
                                iris_stream_t stream) {
    if (!sc || n_spots < 1 || !spots) return fail(IRIS_ERR_ARG, "iris_pt_nee_spot: a scene and at least one spot are required");
    if (N < 0 || (N > 0 && (!pos || !nrm || !wo || !albedo || !roughness || !metallic || !pick || !coef || !e))) return fail(IRIS_ERR_ARG, "iris_pt_nee_spot: bad arguments");
    if (N == 0) return IRIS_OK;
    SpotArgs a{};
    a.sc = sc->dev; a.N = N; a.S = n_spots;
    a.pos = pos; a.nrm = nrm; a.wo = wo; a.albedo = albedo; a.rough = roughness; a.metal = metallic; a.pick = pick; a.spots = spots; a.coef = coef; a.e = e;
    with_trace(a.sc, N, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pt_nee_spot_kernel<T::layout, T::joint>), trace_grid(N), dim3(kBlock), 0, (hipStream_t)stream, a);
    });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_relight_shade(const iris_emitter* em, const int32_t* surf, int64_t n_surf, const float* cmat, int n_cmat, const float* pos,
                                  const float* pos_next, const float* nrm_next, const float* wi, const int64_t* tri_next, const float* pdf, const float* weight,
                                  float* albedo_next, float* roughness_next, float* metallic_next, const float* radiance, const int32_t* e1, const float* coef1,
                                  const float* spot_intensity, const int32_t* e_spot, const float* coef_spot, float* L, const int32_t* rows, float* throughput,
                                  uint8_t* valid_next, int64_t N, float g_eps, iris_stream_t stream) {
    RelightShadeArgs a{};
    if (!em || !surf_args(surf, n_surf, cmat, n_cmat, a.sf) || (n_surf > 0 && n_surf != em->dev.nf) || N < 0 ||
        (N > 0 && (!pos || !pos_next || !nrm_next || !wi || !tri_next || !pdf || !weight || !albedo_next || !roughness_next || !metallic_next || !L || !throughput ||
                   !valid_next || (e1 && (!radiance || !coef1)) || (em->k > 0 && !radiance) || (e_spot && (!spot_intensity || !coef_spot)))))
        return fail(IRIS_ERR_ARG, "iris_relight_shade: bad arguments");
    if (N == 0) return IRIS_OK;
    a.em = em->dev; a.N = N;
    a.pos = pos; a.pos_next = pos_next; a.nrm_next = nrm_next; a.wi = wi; a.pdf = pdf; a.w = weight; a.tri_next = tri_next;
    a.albedo_next = albedo_next; a.rough_next = roughness_next; a.metal_next = metallic_next;
    a.radiance = radiance; a.e1 = e1; a.coef1 = coef1; a.spot_intensity = spot_intensity; a.es = e_spot; a.coef_s = coef_spot;
    a.L = L; a.rows = rows; a.throughput = throughput; a.valid_next = valid_next; a.g_eps = g_eps;
    return launch1d(relight_shade_kernel, N, 8192, stream, a);
}

// ======================================================================================================
// OpenEXR ZIP / ZIPS scanline blocks deflated on the device (iris_deflate.h)
// ======================================================================================================
struct ZipLayout { int64_t n_segs, n_chunks, seg_data, seg_len, seg_adler, chunk_len, chunk_adler, chunk_off, seg_off, total; int sf, st; };
static bool zip_layout(int n_maps, int64_t n_full, int64_t block_bytes, int64_t tail_bytes, ZipLayout& z, bool png = false) {
    if (n_maps <= 0 || n_full < 0 || tail_bytes < 0 || (n_full > 0 && block_bytes <= 0) || (n_full == 0 && tail_bytes == 0)) return false;
    if (block_bytes >= ((int64_t)1 << 31) - 64 || tail_bytes >= ((int64_t)1 << 31) - 64) return false;
    auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
    z.sf = n_full > 0 ? (int)((block_bytes + kZipSeg - 1) / kZipSeg) : 0;
    z.st = tail_bytes > 0 ? (int)((tail_bytes + kZipSeg - 1) / kZipSeg) : 0;
    z.n_segs = (int64_t)n_maps * (n_full * z.sf + z.st);
    z.n_chunks = (int64_t)n_maps * (n_full + (tail_bytes > 0 ? 1 : 0));
    if (z.n_segs >= ((int64_t)1 << 31)) return false;
    z.seg_data = 0;
    z.seg_len = up(z.seg_data + z.n_segs * kZipSegCap);
    z.seg_adler = up(z.seg_len + z.n_segs * 4);
    z.chunk_len = up(z.seg_adler + z.n_segs * 8);
    z.chunk_adler = up(z.chunk_len + z.n_chunks * 4);
    z.chunk_off = up(z.chunk_adler + z.n_chunks * 4);
    z.seg_off = up(z.chunk_off + z.n_chunks * 8);
    z.total = png ? up(z.seg_off + z.n_segs * 4) : z.seg_off;       // (the PNG streams also keep where each segment starts)
    return true;
}
extern "C" IRIS_API uint64_t iris_exr_zip_workspace_bytes(int n_maps, int64_t n_full, int64_t block_bytes, int64_t tail_bytes) {
    ZipLayout z;
    return zip_layout(n_maps, n_full, block_bytes, tail_bytes, z) ? (uint64_t)z.total : 0;
}
extern "C" IRIS_API int iris_exr_zip_encode(const uint8_t* full, const uint8_t* tail, int n_maps, int64_t n_full, int64_t block_bytes, int64_t tail_bytes,
                                          int lines_per_block, uint8_t* records, int64_t* map_offsets, void* workspace, uint64_t workspace_bytes,
                                          iris_stream_t stream) {
    ZipLayout z;
    if (!zip_layout(n_maps, n_full, block_bytes, tail_bytes, z) || lines_per_block <= 0 || !records || !map_offsets || !workspace ||
        (n_full > 0 && !full) || (tail_bytes > 0 && !tail))
        return fail(IRIS_ERR_ARG, "iris_exr_zip_encode: bad arguments");
    if ((n_full + 1) * (int64_t)lines_per_block >= ((int64_t)1 << 31)) return fail(IRIS_ERR_ARG, "iris_exr_zip_encode: scanline index beyond int32");
    if (workspace_bytes < (uint64_t)z.total) return fail(IRIS_ERR_ARG, "iris_exr_zip_encode: workspace smaller than iris_exr_zip_workspace_bytes()");
    uint8_t* ws = (uint8_t*)workspace;
    ZipArgs a{};
    a.full = full; a.tail = tail; a.M = n_maps; a.lines = lines_per_block; a.sf = z.sf; a.st = z.st;
    a.n_full = n_full; a.B = block_bytes; a.T = tail_bytes; a.records = records; a.map_offsets = map_offsets; a.record_header = 8;
    a.seg_data = ws + z.seg_data; a.seg_len = (uint32_t*)(ws + z.seg_len); a.seg_adler = (uint32_t*)(ws + z.seg_adler);
    a.chunk_len = (uint32_t*)(ws + z.chunk_len); a.chunk_adler = (uint32_t*)(ws + z.chunk_adler); a.chunk_off = (int64_t*)(ws + z.chunk_off);
    hipLaunchKernelGGL(zip_segment_kernel, dim3((unsigned)z.n_segs), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(zip_chunk_kernel, dim3((unsigned)std::min<int64_t>((z.n_chunks + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(zip_offsets_kernel, dim3(1), dim3(kZipScanThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(zip_emit_kernel, dim3((unsigned)z.n_chunks), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// 8-bit PNG files on the device (iris_png.h): scanline bytes of a group of images, then one zlib stream per image
// ======================================================================================================
extern "C" IRIS_API void iris_png_magma_table(uint8_t* rgb) { std::memcpy(rgb, kPngMagmaHost, sizeof(kPngMagmaHost)); }
extern "C" IRIS_API int64_t iris_png_row_bytes(int H, int W, int channels, int magma) {
    const int64_t H2 = H - H % 2, W2 = W - W % 2;
    if (H2 <= 0 || W2 <= 0 || (channels != 1 && channels != 3) || (magma && channels != 1)) return 0;
    return H2 * (1 + W2 * (magma ? 3 : channels));
}
extern "C" IRIS_API int iris_png_rows(const void* const* images, const float* divisors, const uint8_t* magma, int n_images, int H, int W, int channels, int is_u8,
                                    uint8_t* rows, iris_stream_t stream) {
    if (!images || !divisors || !magma || !rows || n_images <= 0) return fail(IRIS_ERR_ARG, "iris_png_rows: bad arguments");
    if (channels != 1 && channels != 3) return fail(IRIS_ERR_ARG, "iris_png_rows: images have 1 or 3 channels");
    for (int m = 0; m < n_images; ++m) {
        if (!images[m]) return fail(IRIS_ERR_ARG, "iris_png_rows: a NULL image");
        if (magma[m] && channels != 1) return fail(IRIS_ERR_ARG, "iris_png_rows: a magma image has one channel");
        if ((magma[m] != 0) != (magma[0] != 0)) return fail(IRIS_ERR_ARG, "iris_png_rows: the images of one call are all magma or none is (equal output sizes)");
        if (!(divisors[m] > 0.f) || std::isinf(divisors[m])) return fail(IRIS_ERR_ARG, "iris_png_rows: a divisor is positive and finite");
    }
    const int64_t block = iris_png_row_bytes(H, W, channels, magma[0]);
    if (block <= 0) return fail(IRIS_ERR_ARG, "iris_png_rows: the image cropped to even height and width is empty");
    for (int m0 = 0; m0 < n_images; m0 += kPngMaxImages) {
        PngRowsArgs a{};
        a.M = std::min(kPngMaxImages, n_images - m0);
        for (int m = 0; m < a.M; ++m) { a.img[m] = images[m0 + m]; a.div[m] = divisors[m0 + m]; a.magma |= (magma[m0 + m] ? 1u : 0u) << m; }
        a.H = H; a.W = W; a.H2 = H - H % 2; a.W2 = W - W % 2; a.cout = magma[0] ? 3 : channels; a.block_bytes = block; a.rows = rows + (int64_t)m0 * block;
        const int64_t n = (int64_t)a.H2 * a.W2;
        const dim3 grid((unsigned)std::min<int64_t>((n + kPngThreads - 1) / kPngThreads, 2048), (unsigned)a.M);
        if (channels == 3 && !is_u8) hipLaunchKernelGGL((png_rows_kernel<3, false>), grid, dim3(kPngThreads), 0, (hipStream_t)stream, a);
        else if (channels == 3) hipLaunchKernelGGL((png_rows_kernel<3, true>), grid, dim3(kPngThreads), 0, (hipStream_t)stream, a);
        else if (!is_u8) hipLaunchKernelGGL((png_rows_kernel<1, false>), grid, dim3(kPngThreads), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((png_rows_kernel<1, true>), grid, dim3(kPngThreads), 0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API uint64_t iris_png_stream_bound(int64_t block_bytes) { return block_bytes > 0 ? (uint64_t)png_stream_bound(block_bytes) : 0; }
extern "C" IRIS_API uint64_t iris_png_workspace_bytes(int n_images, int64_t block_bytes) {
    ZipLayout z;
    return zip_layout(n_images, 1, block_bytes, 0, z, true) ? (uint64_t)z.total : 0;
}
extern "C" IRIS_API int iris_png_encode(const uint8_t* rows, int n_images, int64_t block_bytes, uint8_t* streams, int64_t* offsets, void* workspace,
                                      uint64_t workspace_bytes, iris_stream_t stream) {
    ZipLayout z;
    if (!zip_layout(n_images, 1, block_bytes, 0, z, true) || !rows || !streams || !offsets || !workspace) return fail(IRIS_ERR_ARG, "iris_png_encode: bad arguments");
    if (workspace_bytes < (uint64_t)z.total) return fail(IRIS_ERR_ARG, "iris_png_encode: workspace smaller than iris_png_workspace_bytes()");
    uint8_t* ws = (uint8_t*)workspace;
    ZipArgs a{};
    a.full = rows; a.M = n_images; a.lines = 1; a.sf = z.sf; a.st = 0; a.n_full = 1; a.B = block_bytes; a.T = 0; a.records = streams; a.map_offsets = offsets;
    a.seg_data = ws + z.seg_data; a.seg_len = (uint32_t*)(ws + z.seg_len); a.seg_adler = (uint32_t*)(ws + z.seg_adler);
    a.chunk_len = (uint32_t*)(ws + z.chunk_len); a.chunk_adler = (uint32_t*)(ws + z.chunk_adler); a.chunk_off = (int64_t*)(ws + z.chunk_off);
    a.seg_off = (uint32_t*)(ws + z.seg_off); a.record_header = 0;
    hipLaunchKernelGGL(zip_segment_kernel, dim3((unsigned)z.n_segs), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(png_chunk_kernel, dim3((unsigned)n_images), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(zip_offsets_kernel, dim3(1), dim3(kZipScanThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(png_emit_kernel, dim3((unsigned)z.n_segs), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// Baseline JPEG frames on the device (iris_jpeg.h): the entropy-coded data of a group of equal-size images
// ======================================================================================================
struct JpegLayout { int H2, W2, mx, my; int64_t n_blocks, n_intervals, cap, coef, slots, bit_len, bit_off, cat, ivl_bytes, ivl_len, ivl_off, total; };
static bool jpeg_layout(int n_images, int H, int W, JpegLayout& z) {
    z.H2 = H - H % 2; z.W2 = W - W % 2;
    if (n_images <= 0 || z.H2 <= 0 || z.W2 <= 0 || z.H2 > 65535 || z.W2 > 65535) return false;        // (SOF0 holds the sizes in 16 bits)
    z.mx = (z.W2 + 15) / 16; z.my = (z.H2 + 15) / 16;
    z.cap = z.my * jpeg_interval_bound(z.mx);
    z.n_intervals = (int64_t)n_images * z.my;
    z.n_blocks = z.n_intervals * z.mx * 6;
    if (z.cap >= ((int64_t)1 << 31) || z.n_blocks >= ((int64_t)1 << 31)) return false;
    auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
    z.coef = 0;
    z.slots = up(z.coef + z.n_blocks * 64 * 2);
    z.bit_len = up(z.slots + z.n_blocks * kJpegSlotWords * 4);
    z.bit_off = up(z.bit_len + z.n_blocks * 4);
    z.cat = up(z.bit_off + z.n_blocks * 4);
    z.ivl_bytes = up(z.cat + z.n_intervals * jpeg_interval_words(z.mx) * 4);
    z.ivl_len = up(z.ivl_bytes + z.n_intervals * 4);
    z.ivl_off = up(z.ivl_len + z.n_intervals * 4);
    z.total = up(z.ivl_off + z.n_intervals * 8);
    return true;
}
extern "C" IRIS_API void iris_jpeg_tables(uint8_t* out) {
    std::memcpy(out, kJpegQuantHost, 128);
    std::memcpy(out + 128, kJpegZigHost.nat, 64);
    out += 192;
    for (const JpegSpec* s : {&kJpegDcLuma, &kJpegAcLuma, &kJpegDcChroma, &kJpegAcChroma}) {
        std::memcpy(out, s->bits, 16);
        std::memcpy(out + 16, s->vals, s->n);
        out += 16 + s->n;
    }
}
extern "C" IRIS_API uint64_t iris_jpeg_stream_bound(int H, int W) {
    JpegLayout z;
    return jpeg_layout(1, H, W, z) ? (uint64_t)z.cap : 0;
}
extern "C" IRIS_API uint64_t iris_jpeg_workspace_bytes(int n_images, int H, int W) {
    JpegLayout z;
    return jpeg_layout(n_images, H, W, z) ? (uint64_t)z.total : 0;
}
extern "C" IRIS_API int iris_jpeg_encode(const void* const* images, const float* divisors, const uint8_t* magma, int n_images, int H, int W, int channels, int is_u8,
                                       int quality, uint8_t* streams, int64_t* offsets, void* workspace, uint64_t workspace_bytes, iris_stream_t stream) {
    JpegLayout z;
    if (!images || !divisors || !magma || !streams || !offsets || !workspace || n_images <= 0) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: bad arguments");
    if (channels != 1 && channels != 3) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: images have 1 or 3 channels");
    if (quality < 1 || quality > 100) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: the quality is 1..100");
    for (int m = 0; m < n_images; ++m) {
        if (!images[m]) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: a NULL image");
        if (magma[m] && channels != 1) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: a magma image has one channel");
        if (!(divisors[m] > 0.f) || std::isinf(divisors[m])) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: a divisor is positive and finite");
    }
    if (!jpeg_layout(n_images, H, W, z)) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: the image cropped to even height and width is empty, or too large");
    if (workspace_bytes < (uint64_t)z.total) return fail(IRIS_ERR_ARG, "iris_jpeg_encode: workspace smaller than iris_jpeg_workspace_bytes()");
    uint8_t* ws = (uint8_t*)workspace;
    const int64_t per_image = (int64_t)z.my * z.mx * 6;
    for (int m0 = 0; m0 < n_images; m0 += kPngMaxImages) {
        JpegTransformArgs a{};
        a.M = std::min(kPngMaxImages, n_images - m0);
        for (int m = 0; m < a.M; ++m) { a.img[m] = images[m0 + m]; a.div[m] = divisors[m0 + m]; a.magma |= (magma[m0 + m] ? 1u : 0u) << m; }
        a.H = H; a.W = W; a.H2 = z.H2; a.W2 = z.W2; a.mx = z.mx; a.my = z.my;
        a.scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        a.coef = (int16_t*)(ws + z.coef) + (int64_t)m0 * per_image * 64;
        const dim3 grid((unsigned)((per_image + kJpegThreads / 64 - 1) / (kJpegThreads / 64)), (unsigned)a.M);
        if (channels == 3 && !is_u8) hipLaunchKernelGGL((jpeg_transform_kernel<3, false>), grid, dim3(kJpegThreads), 0, (hipStream_t)stream, a);
        else if (channels == 3) hipLaunchKernelGGL((jpeg_transform_kernel<3, true>), grid, dim3(kJpegThreads), 0, (hipStream_t)stream, a);
        else if (!is_u8) hipLaunchKernelGGL((jpeg_transform_kernel<1, false>), grid, dim3(kJpegThreads), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((jpeg_transform_kernel<1, true>), grid, dim3(kJpegThreads), 0, (hipStream_t)stream, a);
    }
    JpegArgs a{};
    a.mx = z.mx; a.my = z.my; a.n_blocks = z.n_blocks; a.n_intervals = z.n_intervals;
    a.coef = (const int16_t*)(ws + z.coef); a.slots = (uint32_t*)(ws + z.slots); a.bit_len = (uint32_t*)(ws + z.bit_len); a.bit_off = (uint32_t*)(ws + z.bit_off);
    a.cat = (uint32_t*)(ws + z.cat); a.ivl_bytes = (uint32_t*)(ws + z.ivl_bytes); a.ivl_len = (uint32_t*)(ws + z.ivl_len); a.ivl_off = (int64_t*)(ws + z.ivl_off);
    a.streams = streams;
    ZipArgs s{};                                                    // zip_offsets_kernel: an interval is a chunk, an image a map; no record header
    s.M = n_images; s.n_full = z.my; s.T = 0; s.record_header = 0; s.chunk_len = a.ivl_len; s.chunk_off = a.ivl_off; s.map_offsets = offsets;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((z.n_blocks + kJpegThreads - 1) / kJpegThreads)), dim3(kJpegThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(jpeg_assemble_kernel, dim3((unsigned)z.n_intervals), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(zip_offsets_kernel, dim3(1), dim3(kZipScanThreads), 0, (hipStream_t)stream, s);
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3((unsigned)z.n_intervals), dim3(kZipThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// 8-bit image resize on the device (iris_resize.h): the scannetpp layout's --res_scale
// ======================================================================================================
extern "C" IRIS_API int iris_resize_tables(int mode, int ns, int nd, int32_t* ofs, int16_t* coef) {
    if (mode != IRIS_RESIZE_LINEAR && mode != IRIS_RESIZE_NEAREST) return fail(IRIS_ERR_ARG, "iris_resize_tables: the mode is IRIS_RESIZE_LINEAR or IRIS_RESIZE_NEAREST");
    if (ns < 1 || nd < 1 || ns > kResizeMaxSide || nd > kResizeMaxSide) return fail(IRIS_ERR_ARG, "iris_resize_tables: an axis has 1..65535 samples");
    if (!ofs || (mode == IRIS_RESIZE_LINEAR && !coef)) return fail(IRIS_ERR_ARG, "iris_resize_tables: a NULL table");
    resize_axis_table(mode == IRIS_RESIZE_NEAREST ? kResizeNearest : kResizeLinear, ns, nd, ofs, coef);
    return IRIS_OK;
}
template <int C>
static void resize_launch(int mode, dim3 grid, hipStream_t st, const ResizeArgs& a) {
    if (mode == kResizeHalf) hipLaunchKernelGGL((resize_kernel<C, kResizeHalf>), grid, dim3(kResizeThreads), 0, st, a);
    else if (mode == kResizeNearest) hipLaunchKernelGGL((resize_kernel<C, kResizeNearest>), grid, dim3(kResizeThreads), 0, st, a);
    else hipLaunchKernelGGL((resize_kernel<C, kResizeLinear>), grid, dim3(kResizeThreads), 0, st, a);
}
extern "C" IRIS_API int iris_resize_u8(const void* const* images, int n_images, int Hs, int Ws, int channels, int mode, const int32_t* xofs, const int16_t* xcoef,
                                     const int32_t* yofs, const int16_t* ycoef, uint8_t* out, int Ht, int Wt, iris_stream_t stream) {
    if (!images || !out || n_images <= 0) return fail(IRIS_ERR_ARG, "iris_resize_u8: bad arguments");
    if (channels != 1 && channels != 3) return fail(IRIS_ERR_ARG, "iris_resize_u8: images have 1 or 3 channels");
    if (mode != IRIS_RESIZE_LINEAR && mode != IRIS_RESIZE_NEAREST) return fail(IRIS_ERR_ARG, "iris_resize_u8: the mode is IRIS_RESIZE_LINEAR or IRIS_RESIZE_NEAREST");
    if (Hs < 1 || Ws < 1 || Ht < 1 || Wt < 1 || Hs > kResizeMaxSide || Ws > kResizeMaxSide || Ht > kResizeMaxSide || Wt > kResizeMaxSide)
        return fail(IRIS_ERR_ARG, "iris_resize_u8: a side has 1..65535 pixels");
    for (int m = 0; m < n_images; ++m)
        if (!images[m]) return fail(IRIS_ERR_ARG, "iris_resize_u8: a NULL image");
    int kernel_mode = mode == IRIS_RESIZE_NEAREST ? kResizeNearest : kResizeLinear;
    if (mode == IRIS_RESIZE_LINEAR && Hs == 2 * Ht && Ws == 2 * Wt) kernel_mode = kResizeHalf;       // OpenCV's switch to the area path: BOTH axes exactly 2
    if (kernel_mode != kResizeHalf && (!xofs || !yofs || (kernel_mode == kResizeLinear && (!xcoef || !ycoef)))) return fail(IRIS_ERR_ARG, "iris_resize_u8: a NULL table");
    const int64_t block = (int64_t)Ht * Wt * channels;
    for (int m0 = 0; m0 < n_images; m0 += kResizeMaxImages) {
        ResizeArgs a{};
        const int M = std::min(kResizeMaxImages, n_images - m0);
        for (int m = 0; m < M; ++m) a.img[m] = static_cast<const uint8_t*>(images[m0 + m]);
        a.xofs = xofs; a.yofs = yofs; a.xcoef = xcoef; a.ycoef = ycoef; a.Hs = Hs; a.Ws = Ws; a.Ht = Ht; a.Wt = Wt; a.block_bytes = block;
        a.out = out + (int64_t)m0 * block;
        const int64_t n_dwords = (block + 3) / 4 + 1;
        const dim3 grid((unsigned)std::min<int64_t>((n_dwords + kResizeThreads - 1) / kResizeThreads, 4096), (unsigned)M);
        if (channels == 3) resize_launch<3>(kernel_mode, grid, (hipStream_t)stream, a);
        else resize_launch<1>(kernel_mode, grid, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// ======================================================================================================
// 8(f)-2: G-buffer pooling builders (the stages that produce vslf.npz / emitter.pth)
// ======================================================================================================
// VoxelSLF.scatter_add (model/slf.py:56-61): radiance[idx] += rgb, count[idx] += 1 with idx = spatial_idx(x).
// Samples that fall into an empty voxel (idx = -1) are dropped (torch would raise on the negative index).
__global__ void slf_scatter_add_kernel(SlfDev s, const float* __restrict__ x, const float* __restrict__ rgb, int64_t B, float* __restrict__ acc,
                                       unsigned long long* __restrict__ count) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        pool_voxel(s, ld3(x + i * 3), ld3(rgb + i * 3), acc, count);      // iris_prebake.h: shared with pool_view_kernel
    }
}
extern "C" IRIS_API int iris_slf_scatter_add(const iris_slf* s, const float* x, const float* rgb, int64_t B, float* radiance_acc, int64_t* count,
                                    iris_stream_t stream) {
    if (!s || B < 0 || (B > 0 && (!x || !rgb || !radiance_acc || !count))) return fail(IRIS_ERR_ARG, "iris_slf_scatter_add: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(slf_scatter_add_kernel, B, 8192, stream, s->dev, x, rgb, B, radiance_acc, (unsigned long long*)count);
}
// slf_bake.py:104-110: occupancy histogram of the voxel grid, hist[x + y*H + z*H*H] += 1 (float counts, exact below 2^24)
__global__ void voxel_histogram_kernel(const float* __restrict__ x, int64_t B, float vmin, float den, int H, float* __restrict__ hist) {
    SlfDev s{}; s.H = H; s.vmin = vmin; s.den = den;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        pool_hist(hist, s, ld3(x + i * 3));
    }
}
extern "C" IRIS_API int iris_voxel_histogram(const float* x, int64_t B, double voxel_min, double voxel_max, int H, float* hist, iris_stream_t stream) {
    if (B < 0 || H <= 0 || (B > 0 && (!x || !hist))) return fail(IRIS_ERR_ARG, "iris_voxel_histogram: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(voxel_histogram_kernel, B, 8192, stream, x, B, (float)voxel_min, (float)(voxel_max - voxel_min), H, hist);
}
// extract_emitter_ldr.py:90-95 (torch_scatter.scatter(..., reduce='sum')): out[idx[i]] += values[i], count[idx[i]] += 1; idx < 0 skipped
__global__ void scatter_add_rows_kernel(const float* __restrict__ values, const int64_t* __restrict__ idx, int64_t B, int64_t F, float* __restrict__ out,
                                        float* __restrict__ count) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        pool_triangle(idx[i], F, ld3(values + i * 3), out, count);
    }
}
extern "C" IRIS_API int iris_scatter_add_rows(const float* values, const int64_t* idx, int64_t B, int64_t F, float* out, float* count, iris_stream_t stream) {
    if (B < 0 || F < 0 || (B > 0 && (!values || !idx || !out))) return fail(IRIS_ERR_ARG, "iris_scatter_add_rows: bad arguments");
    if (B == 0) return IRIS_OK;
    return launch1d(scatter_add_rows_kernel, B, 8192, stream, values, idx, B, F, out, count);
}

// The rays of a per-view call (iris_view_rays -> ViewRays, iris_batch.h), checked and filled for entry point fn; r.B is the ray count afterwards.
static int view_rays_args(const char* fn, const iris_view_rays& v, ViewRays& r) {
    const std::string name(fn);
    r.from_camera = v.camera != nullptr;
    if (r.from_camera) {
        if (v.H <= 0 || v.W <= 0) return fail(IRIS_ERR_ARG, name + ": a camera needs a positive image size");
        std::memcpy(r.camera, v.camera, sizeof(r.camera));
        r.H = v.H; r.W = v.W; r.synthetic = v.synthetic != 0;
        r.B = (int64_t)v.H * v.W;
    } else {
        if (v.B < 0 || (v.B > 0 && (!v.rays_o || !v.rays_d || v.ray_stride < 3))) return fail(IRIS_ERR_ARG, name + ": bad rays");
        r.rays_o = v.rays_o; r.rays_d = v.rays_d; r.ray_stride = v.ray_stride; r.B = v.B;
    }
    return IRIS_OK;
}
// iris_debug_set("pool_combine", 0): per-lane atomics, the comparison arm of tools/bench_prebake.py and tools/bench_fuse_segmentation.py
static int pool_combine() { return g_opt_pool_combine >= 0 ? g_opt_pool_combine != 0 : 1; }

// 5c-11: a view's primary hits pooled where they land (iris_prebake.h)
extern "C" IRIS_API int iris_pool_view(const iris_scene* s, const iris_pool_view_args* v, iris_stream_t stream) {
    if (!s || !v) return fail(IRIS_ERR_ARG, "iris_pool_view: bad arguments");
    PoolViewArgs a{};
    if (const int rc = view_rays_args("iris_pool_view", v->rays, a.rays)) return rc;
    const int64_t B = a.rays.B;
    const bool pools = v->slf || v->tri_sum;
    if (pools && !v->rgb && B > 0) return fail(IRIS_ERR_ARG, "iris_pool_view: a pooling sink without a radiance store");
    if (v->slf && (!v->slf_acc || !v->slf_count)) return fail(IRIS_ERR_ARG, "iris_pool_view: the voxel pool needs its sum and count buffers");
    if (v->tri_sum && v->n_tri < 0) return fail(IRIS_ERR_ARG, "iris_pool_view: negative triangle count");
    if (v->hist && v->hist_H <= 0) return fail(IRIS_ERR_ARG, "iris_pool_view: the histogram needs a positive resolution");
    if (v->crf_grid && (!v->crf_inv_table || v->crf_n < 2 || v->crf_n > kCrfMaxKnots || (v->exposure && v->n_exposure != 1 && v->n_exposure != B)))
        return fail(IRIS_ERR_ARG, "iris_pool_view: bad response tables or exposure count");
    if (B == 0) return IRIS_OK;
    a.rgb = v->rgb; a.rgb_u8 = v->rgb_is_u8 != 0;
    a.crf.grid = v->crf_grid; a.crf.table = v->crf_inv_table; a.crf.n = v->crf_n;
    a.crf.exposure = v->exposure; a.crf.n_exposure = v->n_exposure; a.crf.exposure_value = v->exposure_value; a.crf.B = B;
    a.bounds = v->bounds;
    a.hist = v->hist;
    a.hist_grid.H = v->hist_H; a.hist_grid.vmin = (float)v->voxel_min; a.hist_grid.den = (float)(v->voxel_max - v->voxel_min);      // as iris_voxel_histogram
    if (v->slf) { a.has_slf = 1; a.slf = v->slf->dev; a.slf_acc = v->slf_acc; a.slf_count = (unsigned long long*)v->slf_count; }
    a.tri_sum = v->tri_sum; a.tri_count = v->tri_count; a.n_tri = v->n_tri;
    a.combine = pool_combine();
    with_trace(s->dev, B, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pool_view_kernel<T::layout, T::joint>), trace_grid(B), dim3(kBlock), 0, (hipStream_t)stream, s->dev, a);
    });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// 5c-16: segmentation fusion -- a view's label vote per triangle, the rows' winners, a view painted from a per-triangle table (iris_labels.h)
static int label_view_args(const char* fn, const iris_scene* s, const iris_label_view_args* v, LabelViewArgs& a) {
    const std::string name(fn);
    if (!s || !v) return fail(IRIS_ERR_ARG, name + ": bad arguments");
    if (const int rc = view_rays_args(fn, v->rays, a.rays)) return rc;
    if (v->n_tri < 0) return fail(IRIS_ERR_ARG, name + ": negative triangle count");
    a.n_tri = v->n_tri;
    return IRIS_OK;
}
extern "C" IRIS_API int iris_label_vote(const iris_scene* s, const iris_label_view_args* v, iris_stream_t stream) {
    LabelViewArgs a{};
    if (const int rc = label_view_args("iris_label_vote", s, v, a)) return rc;
    if (v->n_labels < 1) return fail(IRIS_ERR_ARG, "iris_label_vote: n_labels < 1");
    if (a.rays.B > 0 && (!v->ids || !v->hist)) return fail(IRIS_ERR_ARG, "iris_label_vote: the vote needs the pixels' ids and the histogram");
    if (a.rays.B == 0 || a.n_tri == 0 || v->n_labels == 1) return IRIS_OK;      // (one column: only column 0, which is never written)
    a.ids = v->ids; a.ids_u8 = v->ids_is_u8 != 0; a.hist = v->hist; a.n_labels = v->n_labels;
    a.combine = pool_combine();
    with_trace(s->dev, a.rays.B, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((label_vote_kernel<T::layout, T::joint>), trace_grid(a.rays.B), dim3(kBlock), 0, (hipStream_t)stream, s->dev, a);
    });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
extern "C" IRIS_API int iris_label_argmax(const uint32_t* hist, int64_t F, int32_t n_labels, int32_t* tri_label, iris_stream_t stream) {
    if (F < 0 || n_labels < 1 || (F > 0 && (!hist || !tri_label))) return fail(IRIS_ERR_ARG, "iris_label_argmax: bad arguments");
    if (F == 0) return IRIS_OK;
    return launch1d(label_argmax_kernel, (F + kArgmaxRows - 1) / kArgmaxRows * 64, 1 << 16, stream, hist, F, (int)n_labels, tri_label);      // one wave per kArgmaxRows rows
}
extern "C" IRIS_API int iris_label_view(const iris_scene* s, const iris_label_view_args* v, iris_stream_t stream) {
    LabelViewArgs a{};
    if (const int rc = label_view_args("iris_label_view", s, v, a)) return rc;
    if (a.rays.B > 0 && (!v->out || (a.n_tri > 0 && !v->table))) return fail(IRIS_ERR_ARG, "iris_label_view: the view needs the table and the output");
    if (a.rays.B == 0) return IRIS_OK;
    a.table = v->table; a.out = v->out; a.out_u8 = v->out_is_u8 != 0; a.miss_value = v->miss_value;
    with_trace(s->dev, a.rays.B, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((label_view_kernel<T::layout, T::joint>), trace_grid(a.rays.B), dim3(kBlock), 0, (hipStream_t)stream, s->dev, a);
    });
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
