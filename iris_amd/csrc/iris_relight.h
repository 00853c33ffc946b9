// The relighting stage (reference: render_relight.py, which hands the whole job to Mitsuba's `path` integrator with model/fipt_bsdf.py as its BSDF): the per-bounce
// stages that the integrator of utils/relight.py needs on top of iris_pt.h.
//   relight_surface_kernel  the surface class of a batch of hits: constant-material override, absorbers end the path
//   pt_nee_spot_kernel      next-event estimation for spot lights (delta lights: no BRDF-sampling counterpart, no MIS)
//   relight_shade_kernel    everything of a bounce after the material network as ONE launch: surface class of the sampled hit, pt_brdf_finish_kernel's arithmetic
//                           without the radiance cache, the three accumulations of pt_apply_kernel, the throughput update
// Plain C++, no atomics (rows are unique), -ffp-contract=off like the neighbours.
#pragma once
#include "iris_pt.h"

namespace iris {

// per-triangle surface class of the composed mesh: 0 = network (the room, shaded by material_net), -1 = absorber (a lamp switched off), g > 0 = constant-material
// row g - 1 of cmat (G,5): albedo rgb, roughness, metallic.  surf NULL: every triangle is class 0.
struct SurfDev { const int32_t* surf; const float* cmat; int64_t nf; int32_t n_cmat; };

// class of triangle `tri` (-1 = miss: class 0, left alone); a constant-material hit overwrites its material row (albedo NULL: the class alone)
__device__ __forceinline__ int relight_surface1(const SurfDev& s, int64_t tri, float* __restrict__ albedo, float* __restrict__ rough, float* __restrict__ metal, int64_t i) {
    if (!s.surf || tri < 0 || tri >= s.nf) return 0;
    const int c = s.surf[tri];
    if (albedo && c > 0 && c <= s.n_cmat) {
        const float* m = s.cmat + (int64_t)(c - 1) * 5;
        st3(albedo + i * 3, mk3(m[0], m[1], m[2])); rough[i] = m[3]; metal[i] = m[4];
    }
    return c;
}

__global__ void relight_surface_kernel(SurfDev s, const int64_t* __restrict__ tri, int64_t N, float* __restrict__ albedo, float* __restrict__ rough,
                                       float* __restrict__ metal, uint8_t* __restrict__ valid) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = relight_surface1(s, tri[i], albedo, rough, metal, i);
        if (valid && c < 0) valid[i] = 0;                                  // valid &= surf >= 0
    }
}

// ---- spot lights ----------------------------------------------------------------------------------------------------------------------------------------------
// spots (S, kSpotRow): origin xyz, axis xyz (unit), cutoff, beam (radians), cos(cutoff), cos(beam).  Falloff of Mitsuba 3's `spot` plug-in AS DOCUMENTED (unpinned:
// Mitsuba is not available to compare with): 1 inside the beam, linear in the ANGLE between beam and cutoff, 0 outside.
constexpr int kSpotRow = 10;
struct SpotArgs {
    SceneDev sc;
    int64_t N; int S;
    const float *pos, *nrm, *wo, *albedo, *rough, *metal;   // (N,3),(N,3),(N,3),(N,3),(N),(N)
    const float* pick;                                       // (N) uniform: j = min(floor(pick * S), S - 1)
    const float* spots;                                      // (S, kSpotRow)
    float* coef; int32_t* e;                                 // (N,3), (N): contribution = throughput * coef * spot_intensity[e], e = -1: none
};

__device__ __forceinline__ float spot_falloff(float c, float cutoff, float beam, float cos_cutoff, float cos_beam) {
    if (c >= cos_beam) return 1.f;
    if (c > cos_cutoff) return (cutoff - acosf(c)) / (cutoff - beam);
    return 0.f;
}

template <int LAYOUT, bool JOINT = false>
__global__ __launch_bounds__(kBlock, JOINT ? IRIS_JOINT_WAVES : 1) void pt_nee_spot_kernel(SpotArgs a) {
    __shared__ uint32_t s_stack[kStackLds * kBlock];
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * kBlock) {
        const f3 x = ld3(a.pos + i * 3), n = ld3(a.nrm + i * 3), wo = ld3(a.wo + i * 3);
        int j = (int)(a.pick[i] * (float)a.S);
        j = min(max(j, 0), a.S - 1);
        const float* sp = a.spots + (int64_t)j * kSpotRow;
        const f3 dlt = sub3(mk3(sp[0], sp[1], sp[2]), x);
        const float d2 = (dlt.x * dlt.x + dlt.y * dlt.y) + dlt.z * dlt.z;
        const float d = sqrtf(d2);
        const f3 wi = t_normalize(dlt);
        const float c = t_dot(mk3(-wi.x, -wi.y, -wi.z), mk3(sp[3], sp[4], sp[5]));
        const float fall = spot_falloff(c, sp[6], sp[7], sp[8], sp[9]);
        // the shadow ray only where light can arrive: a path picks one of S spots at random (the disco ball: 40 cones of 20 degrees), so most lanes of a wave lie
        // outside their spot's cone and have nothing to trace; the traversal's wave votes count the lanes that are in it
        Hit h; h.slot = -1; h.t = 0.f;
        if (fall > 0.f) {
            const f3 o = mk3(x.x + kRayEps * wi.x, x.y + kRayEps * wi.y, x.z + kRayEps * wi.z);
            h = trace_bvh4<LAYOUT, false, kStackLds, false, JOINT>(a.sc, o, wi, s_stack + threadIdx.x);
        }
        const bool occluded = h.slot >= 0 && h.t < (d - kRayEps) * (1.f - 1e-4f);
        const bool lit = !occluded && fall > 0.f;
        Mat m; m.albedo = ld3(a.albedo + i * 3); m.rough = a.rough[i]; m.metal = a.metal[i];
        f3 brdf; float brdf_pdf;
        eval_brdf1(wi, wo, n, m, brdf, brdf_pdf);                          // (carries NoL)
        const float k = lit ? ((float)a.S * fall) / fmaxf(d2, 1e-12f) : 0.f;
        st3(a.coef + i * 3, lit ? mk3(k * brdf.x, k * brdf.y, k * brdf.z) : mk3(0.f, 0.f, 0.f));
        a.e[i] = lit ? j : -1;
    }
}

// ---- the fused end of a bounce ----------------------------------------------------------------------------------------------------------------------------------
struct RelightShadeArgs {
    EmitDev em; SurfDev sf;
    int64_t N;
    const float *pos, *pos_next, *nrm_next, *wi, *pdf, *w;   // the BRDF stage's outputs (iris_pt_brdf_trace / iris_pt_bounce)
    const int64_t* tri_next;
    float *albedo_next, *rough_next, *metal_next;            // the material rows at the sampled hits: overwritten where the hit is a constant material
    const float* radiance;                                   // (K,3) emitter table, as iris_pt_apply takes it
    const int32_t* e1; const float* coef1;                   // the emitter-sampling stage's pair
    const float* spot_intensity; const int32_t* es; const float* coef_s;      // the spot stage's pair (es NULL: no spots)
    float* L; const int32_t* rows; float* throughput; uint8_t* valid_next;
    float g_eps;
};

// one term of pt_apply_kernel: v = 0 + coef * table[e] (e >= 0), v = t * v, NaN -> 0
__device__ __forceinline__ f3 relight_term(const float* __restrict__ table, int e, f3 c, f3 t) {
    f3 v = mk3(0.f, 0.f, 0.f);
    if (e >= 0) { const f3 r = ld3(table + (int64_t)e * 3); v = mk3(v.x + c.x * r.x, v.y + c.y * r.y, v.z + c.z * r.z); }
    v = mk3(t.x * v.x, t.y * v.y, t.z * v.z);
    if (v.x != v.x) v.x = 0.f;
    if (v.y != v.y) v.y = 0.f;
    if (v.z != v.z) v.z = 0.f;
    return v;
}

__global__ __launch_bounds__(256) void relight_shade_kernel(RelightShadeArgs a) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t tri = a.tri_next[i];
        // 1. the surface class of the sampled hit (its material row is the next bounce's)
        const int cls = relight_surface1(a.sf, tri, a.albedo_next, a.rough_next, a.metal_next, i);
        // 2. pt_brdf_finish_kernel without the radiance cache, operation for operation
        const f3 x = ld3(a.pos + i * 3), pn = ld3(a.pos_next + i * 3), nn = ld3(a.nrm_next + i * 3), wi = ld3(a.wi + i * 3);
        const bool vis = tri != -1;
        int ord = -1;
        if (vis) ord = a.em.emit_ord[tri];
        const bool is_area = ord >= 0;
        float emit_pdf = 0.f;
        if (is_area) emit_pdf = a.em.emitter_pdf / fmaxf(a.em.area[ord], 1e-12f);
        const bool valid_next = (!is_area) && vis;
        const f3 dlt = sub3(x, pn);
        const float d2 = (dlt.x * dlt.x + dlt.y * dlt.y) + dlt.z * dlt.z;
        float G = fabsf(t_dot(mk3(-nn.x, -nn.y, -nn.z), wi)) / fmaxf(d2, a.g_eps);
        if (!valid_next) G = 1.f;
        const float brdf_pdf = a.pdf[i] * G;
        float w_mis = 0.f;
        if (brdf_pdf > 0.f && !isinf(emit_pdf)) w_mis = brdf_pdf * brdf_pdf / (emit_pdf * emit_pdf + brdf_pdf * brdf_pdf);
        if (isinf(brdf_pdf) || emit_pdf == 0.f) w_mis = 1.f;
        const f3 w = ld3(a.w + i * 3);
        const f3 coef2 = mk3(w.x * w_mis, w.y * w_mis, w.z * w_mis);
        // 3. the accumulations in pt_apply_kernel's order: emitter sample, spot sample, BRDF sample; then the throughput
        const f3 t = ld3(a.throughput + i * 3);
        float* q = a.L + (int64_t)(a.rows ? a.rows[i] : i) * 3;
        f3 acc = ld3(q);
        f3 v;
        if (a.e1) {                                                        // (NULL: a table without area lights, nothing was sampled)
            v = relight_term(a.radiance, a.e1[i], ld3(a.coef1 + i * 3), t);
            acc = mk3(acc.x + v.x, acc.y + v.y, acc.z + v.z);
        }
        if (a.es) {
            v = relight_term(a.spot_intensity, a.es[i], ld3(a.coef_s + i * 3), t);
            acc = mk3(acc.x + v.x, acc.y + v.y, acc.z + v.z);
        }
        v = relight_term(a.radiance, is_area ? ord : -1, coef2, t);
        acc = mk3(acc.x + v.x, acc.y + v.y, acc.z + v.z);
        st3(q, acc);
        st3(a.throughput + i * 3, mk3(t.x * w.x, t.y * w.y, t.z * w.z));
        // 4. the path goes on from a network or constant-material surface
        a.valid_next[i] = (valid_next && cls >= 0) ? 1 : 0;
    }
}

}  // namespace iris
