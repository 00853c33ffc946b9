/*
 * iris_hip.h -- C ABI of libiris_hip.so, the MI355X (gfx950) implementation of the bake_shading hot path
 * of facebookresearch/iris.
 *
 * The reference has no FFI of its own: the path is ordinary Python calls into Mitsuba/OptiX and ATen.  The
 * entry points below are therefore exactly the calls a binding of that path needs, one per reference
 * callable (cited per function as reference-file:line).  See INTEGRATION.md for the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer to contiguous memory owned by the caller (a torch tensor), except
 *     the inputs of the *_create functions, which are HOST pointers copied during the call.
 *   - f32 = IEEE binary32; idx arrays are int64 (the reference's torch.long); masks are uint8 (torch.bool).
 *   - Work is enqueued on the caller's hipStream_t and is asynchronous; nothing here synchronises.
 *   - Handles are immutable after creation (except iris_emitter_set_radiance) and may be shared by streams.
 *   - Return value 0 = OK; non-zero = error, message from iris_last_error() (thread local).
 *   - No C++ exception crosses this boundary.  There is no CPU fallback: without a HIP device every
 *     compute entry point fails with IRIS_ERR_HIP.
 */
#ifndef IRIS_HIP_H
#define IRIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define IRIS_API __attribute__((visibility("default")))
#else
#define IRIS_API
#endif

typedef void *iris_stream_t; /* hipStream_t */

typedef struct iris_scene iris_scene;     /* triangle mesh + BVH            (mitsuba scene, bake_shading.py:55-61) */
typedef struct iris_slf iris_slf;         /* VoxelSLF                       (model/slf.py:16-39)                   */
typedef struct iris_emitter iris_emitter; /* SLFEmitter's emitter tables    (model/emitter.py:134-173)             */
typedef struct iris_ngp iris_ngp;         /* NGPBRDF's hash grid + MLP      (model/brdf.py:213-260)                */

enum { IRIS_OK = 0, IRIS_ERR_ARG = 1, IRIS_ERR_HIP = 2, IRIS_ERR_BUILD = 3 };

#define IRIS_RAY_EPSILON 8.940696716308594e-05f /* mitsuba.math.RayEpsilon (float32) = 1500 * 2^-24 */

/* BVH node layouts (reported by iris_scene_get_info; iris_scene_create always builds IRIS_BVH4_Q8) */
enum { IRIS_BVH_DEFAULT = 0, IRIS_BVH4_F32 = 1 /* 128-B nodes, f32 planes (A/B baseline, iris_hip_debug.h) */, IRIS_BVH4_Q8 = 3 /* 64-B nodes, 8-bit planes */ };

typedef struct {
    int64_t n_vertices, n_triangles;
    int32_t layout;        /* IRIS_BVH4_F32 | IRIS_BVH4_Q8 */
    int32_t n_nodes;       /* wide nodes */
    int32_t node_bytes;    /* bytes per node record (64: quantised planes); the default layout keeps EIGHT records per node, one per ray octant
                              (children in that octant's front-to-back order, planes pre-swapped near / far): table = 8 * n_nodes * node_bytes */
    int32_t tri_bytes;     /* stride of a leaf-triangle record (64: component-major (p0.x,p1.x,p2.x,id) (y...) (z...), csrc/iris_trace.h) */
    int32_t depth;         /* wide-tree depth */
    int32_t n_leaf_records;/* leaf-triangle records: n_triangles + the extra references of split long triangles */
    float   sah_cost;      /* cost of the WIDE tree as the collapse minimises it: sum over wide nodes of A_node + sum over leaves of A_leaf * records *
                              tri_cost (0.7), areas relative to the root, duplicated references of split triangles included (csrc/bvh_build.cpp) */
    float   build_seconds;
} iris_scene_info;

/* ---- handles ----------------------------------------------------------------------------------------- */

/* mitsuba.load_dict({'type':'scene','shape_id':{...}})  (bake_shading.py:55-61).  Host SAH build + upload. */
IRIS_API int iris_scene_create(const float *verts, int64_t nv, const int32_t *faces, int64_t nf, int device, iris_scene **out);
IRIS_API void iris_scene_destroy(iris_scene *);
IRIS_API int iris_scene_get_info(const iris_scene *, iris_scene_info *out);

/* VoxelSLF(mask, voxel_min, voxel_max) + load_state_dict (model/slf.py:18-39, model/emitter.py:144-147).
 * inds: (H,H,H) int64 [z][y][x], -1 = empty; radiance: (kv,3).  voxel_min/max are the python floats stored in
 * vslf.npz (slf_bake.py:140-145); the denominator is float32(voxel_max - voxel_min) as in torch-CPU. */
IRIS_API int iris_slf_create(const int64_t *inds, int H, const float *radiance, int64_t kv, double voxel_min, double voxel_max,
                    int device, iris_slf **out);
/* the same from DEVICE buffers (inds int64 (H,H,H), radiance (kv,3) on `device`): the pre-bake stages build the grid on the GPU (slf_bake.py:116-118) */
IRIS_API int iris_slf_create_dev(const int64_t *inds_dev, int H, const float *radiance_dev, int64_t kv, double voxel_min, double voxel_max,
                    int device, iris_slf **out, iris_stream_t);
/* refresh the radiance rows from a DEVICE pointer (kv,3): mean pooling rewrites them (slf_bake.py:138, slf_refine.py:106) */
IRIS_API int iris_slf_set_radiance(iris_slf *, const float *radiance_dev, int64_t kv, iris_stream_t);
IRIS_API void iris_slf_destroy(iris_slf *);

/* SLFEmitter.__init__ (model/emitter.py:149-173): is_emitter (nf) bool, radiance (n_rad,3) indexed by EMITTER
 * ORDINAL (model/emitter.py:203), area (k).  emitter_idx / emitter_pdf=1/k are derived here. */
/* verts (k,3,3) = emitter_vertices and cdf (k) = emitter_cdf (model/emitter.py:155,170) are only needed by
 * iris_sample_emitter / iris_pt_nee and may be NULL. */
IRIS_API int iris_emitter_create(const uint8_t *is_emitter, int64_t nf, const float *radiance, int64_t n_rad, const float *area,
                        int64_t k, const float *verts, const float *cdf, int device, iris_emitter **out);
/* SLFEmitterLearn.radiance is a parameter (model/emitter.py:268): refresh the device copy from a DEVICE pointer. */
IRIS_API int iris_emitter_set_radiance(iris_emitter *, const float *radiance_dev, int64_t n_rad, iris_stream_t);
IRIS_API void iris_emitter_destroy(iris_emitter *);

/* ---- a1: ray generation ------------------------------------------------------------------------------ */
/* get_direction + to_world (utils/dataset/real_ldr.py:49-83; ScanNet++ utils/dataset/scannetpp/dataset.py:202-215).
 * K (9) and c2w (12) are passed BY VALUE from the host (row-major).  rays_o, rays_d: (H*W,3).  ray_diff: also
 * dxdu, dydv and un-normalised rays_d. */
IRIS_API int iris_raygen_real(const float K[9], const float c2w[12], int H, int W, int ray_diff, float *rays_o, float *rays_d,
                     float *dxdu, float *dydv, iris_stream_t);
/* get_ray_directions + get_rays (utils/dataset/synthetic_ldr.py:21-57) */
IRIS_API int iris_raygen_synthetic(float focal, const float c2w[12], int H, int W, int ray_diff, float *rays_o, float *rays_d,
                          float *dxdu, float *dydv, iris_stream_t);
/* The trainers' pixel batch: what Inv*DatasetLDR(pixel=True).__getitem__ slices from its host table (utils/dataset/real_ldr.py:399-427), from a
 * list of global pixel ids.  ALL pointers are DEVICE pointers.  ids (B) int64: view * H*W + y*W + x, each in [0, V*H*W) -- bounding them is the
 * caller's; an id outside the range reads nothing and yields a row of zeros (segmentation -1).  cameras (V,24) f32, 16-B aligned, per view
 * K[9] | c2w[12] | focal | 2 pad (row-major; K is unused when synthetic, focal when not).
 * Stores, each NULL or per pixel of all views in id order: rgb and int_albedo (N,3), uint8 when *_is_u8 else float32; segmentation (N) int32;
 * positions (N,3) f32; exposure (V) f32, per VIEW.
 * Outputs, each NULL or written in full (an output whose store is NULL is an error): rays (B,12) f32, 16-B aligned, = [o | d | dxdu | dydv], the bits
 * iris_raygen_real / iris_raygen_synthetic write for that view and pixel with the same ray_diff (ray_diff = 0: d normalised, dxdu = dydv = 0);
 * rgbs, int_albedo (B,3) f32, a uint8 level u decoded as (float)((double)u / 255.0); segmentation (B) int64; exposure (B,1) f32; positions (B,3)
 * f32.  One launch; B = 0 is a no-op. */
IRIS_API int iris_pixel_batch(const int64_t *ids, int64_t B, const float *cameras, int64_t V, int H, int W, int ray_diff, int synthetic,
                     const void *rgb, int rgb_is_u8, const void *int_albedo, int int_albedo_is_u8, const int32_t *segmentation,
                     const float *positions, const float *exposure, float *out_rays, float *out_rgbs, float *out_int_albedo,
                     int64_t *out_segmentation, float *out_exposure, float *out_positions, iris_stream_t);

/* ---- a2: ray_intersect(scene, xs, ds)  (utils/path_tracing.py:17-48) ---------------------------------- */
/* Any output pointer may be NULL.  Miss: idx=-1, valid=0, pos/nrm/uv=0. */
IRIS_API int iris_intersect(const iris_scene *, const float *xs, const float *ds, int64_t B, float *pos, float *nrm, float *uv,
                   int64_t *idx, uint8_t *valid, iris_stream_t);

/* ---- a3/a4: BaseBRDF.sample_diffuse / sample_specular (model/brdf.py:78-88, :112-136) ------------------- */
IRIS_API int iris_sample_diffuse(const float *u2, const float *normal, int64_t B, float *wi, float *pdf, float *weight,
                        iris_stream_t);
IRIS_API int iris_sample_specular(const float *u2, const float *wo, const float *normal, float roughness, int64_t B, float *wi,
                         float *pdf, float *w0, float *w1, iris_stream_t);
/* the same with one roughness per sample (model/brdf.py:36-59 specular_sampler is called with a Bx1 roughness by sample_brdf) */
IRIS_API int iris_sample_specular_v(const float *u2, const float *wo, const float *normal, const float *roughness, int64_t B,
                           float *wi, float *pdf, float *w0, float *w1, iris_stream_t);

/* ---- a5: VoxelSLF.spatial_idx/forward (model/slf.py:41-70), SLFEmitter.eval_emitter (model/emitter.py:180-221) */
/* The voxel coordinate of every entry point that takes positions (this one, iris_eval_emitter, iris_slf_scatter_add, iris_voxel_histogram, the bake and
 * the view pools) is the reference's float32 expression ((x - voxel_min) / (voxel_max - voxel_min) * H).long().clamp(0, H - 1), one IEEE operation per step.
 * The cast: truncation toward zero where the value is finite and of magnitude below 2^63, INT64_MIN otherwise (NaN, +-inf, magnitude >= 2^63), then the
 * clamp -- so a huge finite coordinate below 2^63 lands in cell H - 1, and NaN, +inf and 2^63 and above in cell 0.  No position reads outside the grid. */
IRIS_API int iris_slf_lookup(const iris_slf *, const float *x, int64_t B, int64_t *idx /*nullable*/, float *rgb /*nullable*/,
                    iris_stream_t);
/* roughness: NULL <=> the reference's roughness=None; otherwise (B) f32.  The iris_slf may be NULL when the cache cannot be reached: roughness NULL, or
 * trace_roughness = +inf (AreaEmitter, model/emitter.py:69-98, has no cache). */
IRIS_API int iris_eval_emitter(const iris_emitter *, const iris_slf *, const float *position, const int64_t *triangle_idx,
                      const float *roughness, float trace_roughness, int64_t B, float *Le, float *emit_pdf,
                      uint8_t *valid_next, iris_stream_t);

/* ---- a3..a7 fused: the bake loop body (bake_shading.py:108-123 diffuse, :168-188 specular) -------------- */
/* pos,nrm[,wo]: (P,3) records of the valid pixels.  u2: (P*spp,2) explicit uniforms in the reference's order
 * (row = pixel*spp + sample), or NULL -> in-kernel Philox4x32-10 keyed by (seed, pix_id[p]*spp+s, stream);
 * pix_id (P) int32 nullable (defaults to p) makes the sample set independent of how pixels are sharded.
 * Ld/Ls0/Ls1: (P,3) = mean over spp of Le, Le*g0, Le*g1.  tri_next (P*spp) int64, nullable: the per-sample hit triangle
 * (the reference's `triangle_idx` of ray_intersect, bake_shading.py:117 / :180).
 * workspace: device scratch of iris_bake_workspace_bytes() bytes for the tile-sorted kernel (8 tile-queue counters, the
 * workgroups' per-ray slots -- sampled direction, then hit -- and their traversal-stack overflow slabs; contents are
 * scratch, nothing survives the call); NULL (or spp > iris_bake_tile_max_spp()) selects the simpler pixel-per-wave kernel.  Both give
 * identical bits. */
IRIS_API uint64_t iris_bake_workspace_bytes(int64_t P, int spp, int specular);   /* 0 if spp > iris_bake_tile_max_spp() */
IRIS_API int iris_bake_tile_max_spp(void);   /* largest spp the tile-sorted / view kernels take (5120: the LDS ray list) */
IRIS_API int iris_bake_diffuse(const iris_scene *, const iris_emitter *, const iris_slf *, const float *pos, const float *nrm,
                      int64_t P, int spp, const float *u2, uint64_t seed, uint32_t stream_id, const int32_t *pix_id,
                      float *Ld, int64_t *tri_next, void *workspace, uint64_t workspace_bytes, iris_stream_t);
IRIS_API int iris_bake_specular(const iris_scene *, const iris_emitter *, const iris_slf *, const float *pos, const float *nrm,
                       const float *wo, float roughness, int64_t P, int spp, const float *u2, uint64_t seed,
                       uint32_t stream_id, const int32_t *pix_id, float *Ls0, float *Ls1, int64_t *tri_next,
                       void *workspace, uint64_t workspace_bytes, iris_stream_t);

/* All lobes of one view (bake_shading.py:93-204) in ONE launch with one tile queue: n_lobes <= 8; roughness[l] < 0 selects the
 * diffuse lobe (out1[l] may be NULL), otherwise the specular lobe of that roughness; spp[l] <= iris_bake_tile_max_spp(); Philox uniforms only.
 * roughness / spp / stream_ids / out0 / out1 are HOST arrays.  Outputs are bit-identical to the per-lobe entry points. */
IRIS_API int iris_bake_view(const iris_scene *, const iris_emitter *, const iris_slf *, const float *pos, const float *nrm, const float *wo,
                   const int32_t *pix_id, int64_t P, int n_lobes, const float *roughness, const int32_t *spp,
                   const uint32_t *stream_ids, uint64_t seed, float *const *out0, float *const *out1, void *workspace,
                   uint64_t workspace_bytes, iris_stream_t);

/* ---- (e) multi-GPU: one view sharded over the ranks of a node in interleaved row stripes (no reference counterpart: bake_shading.py:41 pins one
 * device).  After the single collective, `gathered` holds (world, n_maps, n_max, 3): rank r's maps at its local pixels (its rows -- stripe s of
 * stripe_rows rows belongs to rank s % world -- ascending, row-major, padded to n_max); `full` (n_maps, H*W, 3) receives the image order. */
IRIS_API int iris_unstripe_maps(const float *gathered, int world, int n_maps, int64_t n_max, int H, int W, int stripe_rows, float *full, iris_stream_t);

/* ---- a10: lerp_specular (utils/ops.py:99-118): specular (B,R,3), roughness (B) -> (B,3) ------------------ */
IRIS_API int iris_lerp_specular(const float *specular, const float *roughness, int64_t B, int R, float *out, iris_stream_t);

/* ---- a3 / a4 helpers (utils/ops.py:12-96) as calls of their own; the bake and path-tracing kernels use the same device functions fused.
 * get_normal_space: normal (B,3) -> (B,3,3), columns tangent, bitangent, normal.  double_sided: N (B,3) flipped in place towards V.
 * angle2xyz: theta, phi (B) -> unit (B,3).  ggx_terms, element-wise over B (the caller broadcasts):
 *   op 0 D_GGX(a = cos_h, b = roughness)   1 G1_GGX_Schlick(a = NoV, b = roughness)   2 G_Smith(a = NoV, b = NoL, c = roughness)
 *   op 3 fresnelSchlick(a = VoH, b = F0)   4 fresnelSchlick_sep(a = VoH) -> out = 1 - x, out2 = x with x = (1 - VoH)^5 */
IRIS_API int iris_get_normal_space(const float *normal, int64_t B, float *out, iris_stream_t);
IRIS_API int iris_double_sided(const float *V, float *N, int64_t B, iris_stream_t);
IRIS_API int iris_angle2xyz(const float *theta, const float *phi, int64_t B, float *out, iris_stream_t);
IRIS_API int iris_ggx_terms(int op, const float *a, const float *b, const float *c, int64_t B, float *out, float *out2, iris_stream_t);

/* ---- a9 (BASELINE cfg 5): path_tracing_single (utils/path_tracing.py:320-407) ------------------------------ */
/* Building blocks of the call surface: */
/* SLFEmitter.sample_emitter (model/emitter.py:224-255): s1 (N), s2 (N,2), position (N,3) -> wi (N,3), pdf (N), tri (N) */
IRIS_API int iris_sample_emitter(const iris_emitter *, const float *s1, const float *s2, const float *position, int64_t N, float *wi,
                        float *pdf, int64_t *tri, iris_stream_t);
/* BaseBRDF.eval_brdf (model/brdf.py:138-175): albedo (N,3), roughness (N), metallic (N) -> brdf (N,3), pdf (N) */
IRIS_API int iris_eval_brdf(const float *wi, const float *wo, const float *normal, const float *albedo, const float *roughness,
                   const float *metallic, int64_t N, float *brdf, float *pdf, iris_stream_t);
/* BaseBRDF.sample_brdf (model/brdf.py:177-210) -> wi (N,3), pdf (N), brdf/pdf weight (N,3) */
IRIS_API int iris_sample_brdf(const float *s1, const float *s2, const float *wo, const float *normal, const float *albedo,
                     const float *roughness, const float *metallic, int64_t N, float *wi, float *pdf, float *weight,
                     iris_stream_t);
/* Stages.  The material network is third party (tiny-cuda-nn) and is evaluated by the caller between them, exactly where
 * the reference calls material_net (:355, :392).  L is linear in emitter.radiance, the only tensor that receives gradient:
 * stages emit (emitter ordinal, rgb coefficient) pairs, accumulate_fwd gathers, accumulate_bwd scatter-adds. */
/* :338-340  wi = normalize(rays_d + dx_du*(u-0.5) + dy_dv*(v-0.5)); dudv = the reference's torch.rand(2,B,spp,1) */
IRIS_API int iris_pt_jitter(const float *rays_d, const float *dxdu, const float *dydv, const float *dudv, int64_t B, int spp, float *wi,
                   iris_stream_t);
/* :344  eval_emitter(position, wi, triangle_idx) with the radiance gather factored out: e0 = emitter ordinal or -1 */
IRIS_API int iris_pt_primary_emit(const iris_emitter *, const int64_t *tri, int64_t N, int32_t *e0, uint8_t *valid_next, iris_stream_t);
/* :357-382  emitter sampling + visibility ray + geometry term + eval_brdf + MIS -> term1 = coef1 * radiance[e1].
 * g_eps / pdf_eps / mis_eps: the clamp_min constants of the caller: 1e-6,1e-6,1e-6 in path_tracing_single (:370,:373,:379),
 * 1e-12,1e-12,none(<=0) in trace_indirect (:445,:448,:453). */
IRIS_API int iris_pt_nee(const iris_scene *, const iris_emitter *, const float *pos, const float *nrm, const float *wo, const float *albedo,
                const float *roughness, const float *metallic, const float *s1, const float *s2, int64_t N, float *coef1, int32_t *e1,
                float g_eps, float pdf_eps, float mis_eps, iris_stream_t);
/* :338-344 as ONE launch (the un-compacted mode of path_tracing_single): jitter, closest hit of rays_o[b] + t * wi, the primary hit's emitter ordinal, which paths
 * continue.  dudv (2,B,spp) as iris_pt_jitter; wi, wo = -wi, pos, nrm (B*spp,3) as iris_pt_jitter / iris_intersect give them; e0, valid_next as iris_pt_primary_emit;
 * path_of[i] = i where the path continues (a hit that is not an emitter), -1 otherwise. */
IRIS_API int iris_pt_primary(const iris_scene *, const iris_emitter *, const float *rays_o, const float *rays_d, const float *dxdu, const float *dydv,
                    const float *dudv, int64_t B, int spp, float *wi, float *wo, float *pos, float *nrm, int32_t *e0, uint8_t *valid_next, int32_t *path_of,
                    iris_stream_t);
/* render.py:179-184 as ONE launch, the head of the render stage's intrinsics pass: ds = normalize(rays_d + dx_du*u + dy_dv*v) with u, v in [0,1) -- render.py:180
 * does NOT subtract 0.5, unlike :338-339 --, closest hit of rays_o[b] + t * ds, the primary hit's emitter ordinal.  iris_pt_primary's kernel and outputs (the jitter is
 * one device function with the offset as a parameter), without path_of.  From them: vis = valid_next | (e0 >= 0); emission = e0 >= 0 ? radiance[e0] : 0. */
IRIS_API int iris_render_primary(const iris_scene *, const iris_emitter *, const float *rays_o, const float *rays_d, const float *dxdu, const float *dydv,
                        const float *dudv, int64_t B, int spp, float *wi, float *wo, float *pos, float *nrm, int32_t *e0, uint8_t *valid_next, iris_stream_t);
/* render.py:189-220 after the material network, ONE launch.  Per sample i = b*spp + s (N = B*spp rows, pixel-major): pos, nrm, wo, e0, valid_next as
 * iris_render_primary gives them; albedo (N,3), roughness (N), metallic (N) = material_net(pos); u2 (N,2) the draw of :197; radiance: the emitter's (n_rad,3) tensor
 * itself, as iris_pt_accumulate_fwd takes it (rows beyond the emitter handle's count are never read).
 *   kd_ = albedo*(1-m); ks_ = 0.04*(1-m) + albedo*m; g0, g1 = sample_specular(u2, wo, nrm, roughness)[2:] (iris_sample_specular_v's arithmetic; the direction is
 *   neither traced nor stored); a_prime_ = g0*ks_ + g1 + kd_; emission_ = e0 >= 0 ? radiance[e0] : 0;
 *   keep = (valid_next | e0 >= 0) & ((emission_.r + emission_.g) + emission_.b == 0)  -- an emitter triangle whose radiance row sums to zero stays a surface (:202);
 *   where !keep: kd_ = a_prime_ = 1, roughness_ = 1, metallic_ = 0 (:209-212), selected: a miss's non-finite GGX terms never reach a map;
 *   slf_ = VoxelSLF lookup at pos for EVERY sample (:205 does not mask it): 0 in an empty voxel; a miss is looked up at the position the intersector gives a miss, (0,0,0).
 * SUMMATION ORDER (a contract):  map[b] += (x_0 + x_1 + ... + x_{spp-1}) * (1.0f / spp), samples added in increasing s, in float32 -- `map += x.reshape(-1,spp,C).mean(1)`
 * with a sequential sum.  The six maps are the caller's: kd (B,3), a_prime (B,3), roughness (B), metallic (B), emission (B,3), slf (B,3).  No atomics, every element
 * written by one thread: bitwise reproducible.  spp: any positive int. */
IRIS_API int iris_render_intrinsics(const iris_emitter *, const iris_slf *, const float *radiance, const float *pos, const float *nrm, const float *wo,
                           const int32_t *e0, const uint8_t *valid_next, const float *albedo, const float *roughness, const float *metallic, const float *u2,
                           int64_t B, int spp, float *kd, float *a_prime, float *roughness_map, float *metallic_map, float *emission, float *slf_map,
                           iris_stream_t);
/* :384-391  lobe sampling + next intersection.  lobe 0: sample_brdf(s1,s2,wo,normal,mat); lobe 1: sample_diffuse(s2,normal)
 * (path_tracing_det_diff :93-97, weight 1); lobe 2: sample_specular(s2,wo,normal,lobe_roughness) (path_tracing_det_spec :174-178),
 * weight = (g0,g1,0). */
IRIS_API int iris_pt_brdf_trace(const iris_scene *, const float *pos, const float *nrm, const float *wo, const float *albedo,
                       const float *roughness, const float *metallic, const float *s1, const float *s2, int64_t N, float *wi,
                       float *pdf, float *weight, float *pos_next, float *nrm_next, int64_t *tri_next, uint8_t *valid,
                       int lobe, float lobe_roughness, iris_stream_t);
/* trace_indirect's two tracing stages of a bounce (utils/path_tracing.py:434-471) in ONE launch: iris_pt_nee with the draws (s1, s2) and iris_pt_brdf_trace
 * (lobe 0: sample_brdf) with the draws (s1b, s2b) on the same N paths -- the visibility ray and the BRDF ray of a path leave from the same point; their rays are
 * sorted by direction together and traced by the same persistent lanes.  Outputs as the two calls' (same bits). */
IRIS_API int iris_pt_bounce(const iris_scene *, const iris_emitter *, const float *pos, const float *nrm, const float *wo, const float *albedo,
                   const float *roughness, const float *metallic, const float *s1, const float *s2, const float *s1b, const float *s2b, int64_t N,
                   float *coef1, int32_t *e1, float g_eps, float pdf_eps, float mis_eps, float *wi, float *pdf, float *weight, float *pos_next,
                   float *nrm_next, int64_t *tri_next, uint8_t *valid, iris_stream_t);
/* :394-404  eval_emitter(..., mat_next.roughness, 0.0) + geometry term + MIS -> term2 = coef2 * radiance[e2] + const2.
 * roughness_next may be NULL: "every roughness exceeds trace_roughness" -- the only use of mat_next in the reference's path_tracing_single is the test
 * roughness > trace_roughness = 0.0 (model/emitter.py:209), and NGPBRDF's roughness is sigmoid * 0.98 + 0.02 >= 0.02 (model/brdf.py:258): a caller that knows its
 * material network's lower bound skips the second network evaluation (same outputs, bit for bit).  The iris_slf may be NULL when roughness_next is given and
 * trace_roughness = +inf: no roughness exceeds it, the cache is never read. */
IRIS_API int iris_pt_brdf_finish(const iris_emitter *, const iris_slf *, const float *pos, const float *pos_next, const float *nrm_next,
                        const float *wi, const int64_t *tri_next, const float *roughness_next, const float *pdf, const float *weight,
                        int64_t N, float *coef2, float *const2, int32_t *e2, uint8_t *valid_next /*nullable*/, float trace_roughness,
                        float g_eps, iris_stream_t);
/* trace_indirect's accumulation (utils/path_tracing.py:454-456,:462,:484-486): L[rows[i]] += throughput[i] * (coef[i]*radiance[e[i]]
 * + cst[i]) with NaN -> 0, then throughput[i] *= weight[i].  rows, throughput, e/coef, cst, weight are each nullable. */
IRIS_API int iris_pt_apply(float *L, const int32_t *rows, float *throughput, const float *radiance, const int32_t *e, const float *coef,
                  const float *cst, const float *weight, int64_t N, int nan_to_zero, iris_stream_t);
/* trace_indirect's end of a bounce (utils/path_tracing.py:488-501: `position = position[valid_next]` and its siblings): the rows with keep[i] != 0 are moved to the front
 * of the output arrays IN ORDER, as boolean indexing does -- n3 arrays of 3 floats per row (bit k of negate3: dst3[k] = -src3[k], the reference's `wo = -wi`), n1 of one
 * float, ni of one int32 (each at most 6; the pointer arrays are host arrays of device pointers, read during the call); *count (device int32) receives the number of rows
 * kept.  Outputs must hold N rows and must not alias the inputs.  Two launches on the stream, no host round trip, no index tensors.  workspace: device scratch of
 * iris_pt_compact_workspace_bytes(N) bytes. */
IRIS_API uint64_t iris_pt_compact_workspace_bytes(int64_t N);
IRIS_API int iris_pt_compact(const uint8_t *keep, int64_t N, int n3, const float *const *src3, float *const *dst3, uint32_t negate3,
                    int n1, const float *const *src1, float *const *dst1, int ni, const int32_t *const *srci, int32_t *const *dsti,
                    int32_t *count, void *workspace, uint64_t workspace_bytes, iris_stream_t);

/* ---- the relighting stage (render_relight.py; iris_amd/csrc/iris_relight.h) -------------------------------------- */
/* Surface classes of the composed mesh (utils/lights.py compose): surf (n_surf) int32 per triangle -- 0 = network (shaded by the material network), -1 = absorber
 * (a lamp switched off: a path that hits it ends and adds nothing), g > 0 = constant material, row g - 1 of cmat (n_cmat,5): albedo rgb, roughness, metallic.
 * n_surf = 0: every triangle is class 0.
 * iris_relight_surface: for the hits tri (N) (-1 = miss: left alone) a constant-material hit overwrites its albedo (N,3) / roughness (N) / metallic (N) row in place;
 * valid (N, nullable) &= surf >= 0.  albedo NULL (then roughness and metallic are not read either): only valid is updated. */
IRIS_API int iris_relight_surface(const int32_t *surf, int64_t n_surf, const float *cmat, int n_cmat, const int64_t *tri, int64_t N, float *albedo,
                         float *roughness, float *metallic, uint8_t *valid, iris_stream_t);
/* Next-event estimation for spot lights (delta lights: no MIS).  spots (n_spots,10): origin xyz, unit axis xyz, cutoff, beam (radians), cos(cutoff), cos(beam).
 * Per path: j = min(floor(pick * n_spots), n_spots - 1); wi = normalize(o_j - x), d = |o_j - x|; c = dot(-wi, axis_j); falloff = 1 (c >= cos beam),
 * (cutoff - acos c) / (cutoff - beam) (cos cutoff < c < cos beam), 0 (c <= cos cutoff) -- Mitsuba 3's `spot` plug-in as documented, unpinned; the shadow ray starts at
 * x + RayEpsilon wi and the spot is occluded iff its closest hit lies nearer than (d - RayEpsilon)(1 - 1e-4);
 * coef (N,3) = n_spots * falloff / max(d^2, 1e-12) * eval_brdf(wi, wo, n, material).brdf (which carries NoL), 0 when occluded; e (N) = j when lit, else -1.
 * The contribution of the path is throughput * coef * spot_intensity[e]. */
IRIS_API int iris_pt_nee_spot(const iris_scene *, const float *pos, const float *nrm, const float *wo, const float *albedo, const float *roughness,
                     const float *metallic, const float *pick, const float *spots, int n_spots, int64_t N, float *coef, int32_t *e, iris_stream_t);
/* Everything of a relit bounce after the material network, ONE launch.  Per path i: (1) the surface class of tri_next[i], the constant-material override of the
 * row i of albedo_next / roughness_next / metallic_next (the next bounce's material); (2) iris_pt_brdf_finish's arithmetic without the radiance cache -- emitter
 * ordinal e2, emit_pdf, geometry term, power-2 MIS weight w_mis; (3) in iris_pt_apply's order and arithmetic, each product NaN -> 0:
 *   L[rows[i]] += t * (coef1 * radiance[e1]);  += t * (coef_spot * spot_intensity[e_spot]) (e_spot given);  += t * ((weight * w_mis) * radiance[e2]);  t *= weight
 * with t = throughput[i]; (4) valid_next[i] = the hit is a surface that is neither an emitter nor an absorber.  radiance (K,3) as iris_pt_apply takes it.
 * e1 / coef1 and e_spot / coef_spot / spot_intensity are nullable pairs; rows nullable (identity).  rows must be unique: no atomics.
 * CONTRACT: with n_surf = 0 and no spots the L, throughput and valid_next written are the bits of iris_pt_apply(e1) -> iris_pt_brdf_finish(trace_roughness = +inf)
 * -> iris_pt_apply(e2, const2, weight) on the same inputs with finite weights. */
IRIS_API int iris_relight_shade(const iris_emitter *, const int32_t *surf, int64_t n_surf, const float *cmat, int n_cmat, const float *pos,
                       const float *pos_next, const float *nrm_next, const float *wi, const int64_t *tri_next, const float *pdf, const float *weight,
                       float *albedo_next, float *roughness_next, float *metallic_next, const float *radiance, const int32_t *e1, const float *coef1,
                       const float *spot_intensity, const int32_t *e_spot, const float *coef_spot, float *L, const int32_t *rows, float *throughput,
                       uint8_t *valid_next, int64_t N, float g_eps, iris_stream_t);

/* :406  L (B,3) = mean over spp; path_of (B*spp) maps a path to its row in the compacted stage arrays (or -1).
 * radiance: the (n_rad,3) parameter tensor itself (model/emitter.py:268). */
IRIS_API int iris_pt_accumulate_fwd(const float *radiance, const int32_t *e0, const int32_t *path_of, const int32_t *e1, const float *coef1,
                           const int32_t *e2, const float *coef2, const float *const2, int64_t B, int spp, float *L,
                           iris_stream_t);
/* dL/d radiance: g_radiance (n_rad,3), zero-initialised by the caller, += scatter of gL (B,3) */
IRIS_API int iris_pt_accumulate_bwd(const float *gL, const int32_t *e0, const int32_t *path_of, const int32_t *e1, const float *coef1,
                           const int32_t *e2, const float *coef2, int64_t B, int spp, float *g_radiance, iris_stream_t);
/* The reference's training step (train_emitter.py:181-189, initialize.py:172-180: n_calls = SPP // spp calls of path_tracing_single on the same rays, summed) as ONE
 * accumulation.  Paths are pixel-major, path i = (b * n_calls + c) * spp + s; the arrays are iris_pt_accumulate_fwd's with n_calls * B * spp rows (< 2^31).
 * SUMMATION ORDER (a contract: the result is the loop's `L = 0; L += L_c` bit for bit):
 *   L[b] = (((m_0) + m_1) + ...) + m_{n_calls-1},   m_c = (sum over s = 0 .. spp-1, in that order, of term(b,c,s)) * (1.0f / spp)
 * with iris_pt_accumulate_fwd's per-sample term -- every call's mean is rounded before the calls are added, in call order, in float32.
 * n_calls = 1 gives iris_pt_accumulate_fwd's bits. */
IRIS_API int iris_pt_step_accumulate_fwd(const float *radiance, const int32_t *e0, const int32_t *path_of, const int32_t *e1, const float *coef1,
                                const int32_t *e2, const float *coef2, const float *const2, int64_t B, int spp, int n_calls, float *L,
                                iris_stream_t);
/* its dL/d radiance: the sum of the n_calls per-call gradients as one scatter (float atomics) over all paths, g = gL[b] * (1.0f / spp) for every call of pixel b;
 * g_radiance (n_rad,3) zero-initialised by the caller */
IRIS_API int iris_pt_step_accumulate_bwd(const float *gL, const int32_t *e0, const int32_t *path_of, const int32_t *e1, const float *coef1,
                                const int32_t *e2, const float *coef2, int64_t B, int spp, int n_calls, float *g_radiance, iris_stream_t);

/* ---- 8(f)-2: pooling builders of the stages that write vslf.npz / emitter.pth ------------------------------- */
/* VoxelSLF.scatter_add (model/slf.py:56-61): radiance_acc (kv,3) f32 += rgb, count (kv) int64 += 1 at spatial_idx(x) */
IRIS_API int iris_slf_scatter_add(const iris_slf *, const float *x, const float *rgb, int64_t B, float *radiance_acc, int64_t *count,
                         iris_stream_t);
/* occupancy histogram of slf_bake.py:104-110: hist (H^3) f32, index x + y*H + z*H*H */
IRIS_API int iris_voxel_histogram(const float *x, int64_t B, double voxel_min, double voxel_max, int H, float *hist, iris_stream_t);
/* per-triangle sums of extract_emitter_ldr.py:90-95: out (F,3) += values (B,3) at idx (B); count (F) f32 nullable */
IRIS_API int iris_scatter_add_rows(const float *values, const int64_t *idx, int64_t B, int64_t F, float *out, float *count, iris_stream_t);

/* ---- 8(f)-3: the shading cache resident in HBM + the BRDF trainer's shading combine --------------------------- */
/* Floats per packed row for R roughness levels (R <= 8): [d.rgb 0 | per level: spec0.rgb spec1.rgb], padded to 16 B (40 for R=6).
 * The VALUES are the reference's (pixels, 3+6R) table of utils/dataset/scannetpp/dataset.py:359-377; the order is ours. */
IRIS_API int iris_cache_row_floats(int R);
/* pack the 1+2R maps (n,3) of one view into rows (n, iris_cache_row_floats(R)); spec0 / spec1 are HOST arrays of R device pointers */
IRIS_API int iris_cache_pack(const float *diffuse, const float *const *spec0, const float *const *spec1, int64_t n, int R, float *rows,
                    iris_stream_t);
/* the loader's batch slice (dataset.py:409-414): out (B, 3+6R) = [diffuse | specular0 (R,3) | specular1 (R,3)] of rows[idx] (idx NULL = identity) */
IRIS_API int iris_cache_gather(const float *rows, const int64_t *idx, int64_t B, int R, float *out, iris_stream_t);
/* train_brdf_crf.py:195-203 fused with the slice: L (B,3) = kd*diffuse + ks*lerp_specular(spec0,rough) + lerp_specular(spec1,rough),
 * kd = albedo*(1-metallic), ks = 0.04*(1-metallic) + albedo*metallic; albedo (B,3), metallic (B), roughness (B) */
IRIS_API int iris_shade_cached_fwd(const float *rows, const int64_t *idx, const float *albedo, const float *metallic, const float *roughness,
                          int64_t B, int R, float *L, iris_stream_t);
/* its gradient for an incoming gL (B,3): g_albedo (B,3), g_metallic (B), g_roughness (B); any output may be NULL */
IRIS_API int iris_shade_cached_bwd(const float *rows, const int64_t *idx, const float *albedo, const float *metallic, const float *roughness,
                          const float *gL, int64_t B, int R, float *g_albedo, float *g_metallic, float *g_roughness, iris_stream_t);

/* ---- 8(f)-4: denoiser substitute for mitsuba.OptixDenoiser (bake_shading.py:81,129,198-200) --------------------- */
/* Variance-guided edge-avoiding a-trous filter over (H,W,3) maps, guided by the primary hits of the view: normal / position (H*W,3) f32
 * and valid (H*W) u8 (each nullable: no guide of that kind).  in / out: HOST arrays of n_maps device pointers (in[m] == out[m] allowed);
 * maps are filtered four at a time sharing the geometric weights.  iterations in [1,8] (stride 2^i); defaults used by the Python
 * mirror: 5, sigma_l 16, sigma_n 128, sigma_p 0.05 (tools/tune_denoise.py).  Not bit-comparable with OptiX (closed): judged on PSNR against a high-spp bake. */
IRIS_API uint64_t iris_denoise_workspace_bytes(int H, int W);
IRIS_API int iris_denoise(const float *normal, const float *position, const uint8_t *valid, int H, int W, int n_maps, const float *const *in,
                 float *const *out, int iterations, float sigma_l, float sigma_n, float sigma_p, void *workspace, uint64_t workspace_bytes,
                 iris_stream_t);

/* ---- the material network of the refine / emitter-training / BRDF-training stages ------------------------ */
/* NGPBRDF (model/brdf.py:213-260; loaded and frozen at refine_shading.py:83-92, train_emitter.py:67-77): tiny-cuda-nn
 * NetworkWithInputEncoding(3, 5, HashGrid{n_levels 32, 2 features, log2_hashmap_size 19, base 16, per_level_scale 1.3},
 * FullyFusedMLP{64 neurons, 2 hidden layers, ReLU}) + sigmoid.  params: HOST float32[n_params] = the `mlp.params` tensor of the reference's
 * state dict ([MLP weights 64x64, 64x64, 16x64 row-major | grid tables level by level, 2 features per entry]); n_params must equal
 * iris_ngp_n_params().  params may be NULL: an all-zero network whose parameters live on the device and arrive through iris_ngp_set_params_dev.
 * tiny-cuda-nn is third party: the published algorithm is implemented, parity unpinned (oracle/ngp_torch.py). */
IRIS_API int64_t iris_ngp_n_params(void);
IRIS_API int iris_ngp_create(const float *params, int64_t n_params, double voxel_min, double voxel_max, int device, iris_ngp **out);
/* forward(position): position (N,3) f32 world space -> albedo (N,3), roughness (N) in [0.02,1], metallic (N), all f32 device pointers.
 * Outputs lie on the HALF grid as the reference's do (model/brdf.py:255: the network's half output -> sigmoid -> half -> .float(); roughness * 0.98 + 0.02
 * in f32 afterwards).  The handle owns the feature buffer the two kernels of a call exchange (2^20 points x 128 B); calls on ONE handle from different
 * streams or host threads are serialised by the library (a device-side event wait, a host mutex); different handles are independent. */
IRIS_API int iris_ngp_forward(const iris_ngp *, const float *position, int64_t N, float *albedo, float *roughness, float *metallic, iris_stream_t);
/* Training (train_brdf_crf.py:163-207: material(positions) -> loss -> backward() -> Adam over mlp.params).
 * set_params_dev: params_dev = DEVICE float32[n_params] (16-byte aligned), the master copy an optimizer updates -> the handle's half weights and tables,
 * rounded to nearest even as iris_ngp_create rounds; one kernel on the stream, no host copy.
 * backward: the gradient of the parameters given the cotangents of forward's three outputs; position has no gradient (the reference's comes from
 * ray_intersect).  Straight-through: every rounding to half of the forward has derivative 1; d/dz of the output stage is g * s (1 - s) with s the forward's
 * half-grid sigmoid (* 0.98 for roughness); ReLU masks from the recomputed pre-activations.  Nothing is saved by forward: backward re-encodes and recomputes.
 * dz is multiplied by loss_scale before it is rounded to half (tiny-cuda-nn's default is 128) and the result divided by it again; a scaled gradient beyond
 * the half range gives inf, as in the library.  grad_params: DEVICE float32[n_params], ADDED to.  Entries [0, 9216) (the three matrices) are summed in a
 * fixed order: bitwise reproducible; the table entries receive f32 atomic adds: reproducible up to summation order.  Rows 5..15 of the padded output
 * matrix receive exactly 0.  workspace: DEVICE, 16-byte aligned, at least iris_ngp_backward_workspace_bytes(N) bytes, free for reuse once the stream has
 * passed the call.  N = 0 is a no-op.  Both calls are ordered against the other calls of the same handle as forwards are. */
IRIS_API int iris_ngp_set_params_dev(iris_ngp *, const float *params_dev, int64_t n_params, iris_stream_t);
IRIS_API uint64_t iris_ngp_backward_workspace_bytes(int64_t N);
IRIS_API int iris_ngp_backward(const iris_ngp *, const float *position, int64_t N, const float *g_albedo, const float *g_roughness, const float *g_metallic,
                      float loss_scale, float *grad_params, void *workspace, uint64_t workspace_bytes, iris_stream_t);
IRIS_API void iris_ngp_destroy(iris_ngp *);

/* ---- the trainers' optimizer step ---------------------------------------------------------------------------------- */
/* torch.optim.Adam (no amsgrad, no maximize; weight_decay is L2: added to the gradient) on DEVICE float32 buffers of n entries, in place, one pass.
 * step counts from 1 (the step being taken).  The host forms w1 = 1 - beta1, w2 = 1 - beta2, step_size = lr / (1 - beta1^step) and
 * bc2 = sqrt(1 - beta2^step) in double and rounds each to float once, as it does beta2, eps and weight_decay; per element, in float32 without contraction:
 *     g' = wd != 0 ? g + wd p : g;   m' = m + w1 (g' - m);   v' = v beta2 + (w2 g') g';   p' = p - step_size (m' / (sqrtf(v') / bc2 + eps)).
 * Checked on the host before anything is launched: step >= 1; lr and eps finite and positive; 0 <= beta < 1; weight_decay >= 0 and finite; n >= 0;
 * no NULL pointer when n > 0.  n = 0 is a no-op.
 * iris_adam_step: any n, 4-byte-aligned pointers; 16-byte accesses where all four pointers are 16-byte aligned, one element per thread otherwise and
 *   for the last n % 4 entries: the same bits either way.  The four buffers must not overlap.
 * iris_ngp_adam_step: the step of NGPBRDF's mlp.params (n_params == iris_ngp_n_params(), all four pointers 16-byte aligned) which, in the same pass,
 *   writes the handle's half copy of the new parameters (round to nearest even: what iris_ngp_set_params_dev would make of them), so that the next
 *   forward needs no refresh.  Ordered against the handle's other calls as iris_ngp_set_params_dev is. */
IRIS_API int iris_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, double lr, double beta1,
                   double beta2, double eps, double weight_decay, iris_stream_t);
IRIS_API int iris_ngp_adam_step(iris_ngp *, float *params_dev, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n_params, int64_t step,
                       double lr, double beta1, double beta2, double eps, double weight_decay, iris_stream_t);

/* ---- the BRDF trainer's roughness-metallic propagation regulariser (train_brdf_crf.py:212-290) ------------------------ */
/* All six calls work on the batch SORTED by segment id: sorted_seg, order = torch.sort(segmentation, stable=True) (N int64 each; a stable sort keeps a
 * segment's pixels in ascending index, the order of the reference's torch.where).  Position q of the sorted batch holds pixel order[q].  N < 2^31 - 64.
 * runs: (N, 2) int32, per position the (start, count) of its segment's run, from two binary searches in sorted_seg; no segment count is ever needed
 * (sum over segments of a mean = sum over pixels of term / count).  Nothing here synchronises or depends on data in the size of an output. */
IRIS_API int iris_prop_runs(const int64_t *sorted_seg, int64_t N, int32_t *runs, iris_stream_t);
/* The local ranks the Philox mode of the semantic branch draws: draws (N, K) int64 indexed by PIXEL, draws[i][k] in [0, count of i's segment) =
 * word (k / 64) % 4 of the Philox4x32-10 block with counter (64 (k / 256) + k % 64, i, 0x50524F50, 0) and key seed, modulo the count (every row is
 * filled, also those of segments with fewer than K members, which the loss does not use). */
IRIS_API int iris_prop_draws(const int32_t *runs, const int64_t *order, int64_t N, int K, uint64_t seed, int64_t *draws, iris_stream_t);
/* Semantic branch (:243-290).  roughness, metallic (N), albedo, positions (N, 3) by pixel.  normalise != 0: positions = (positions - voxel_min) /
 * (voxel_max - voxel_min) * 2 - 1 first (:244).  Pixel i of a segment with c members mem[0..c) has, when c < K, the c partners mem[0..c), else K partners
 * mem[d]: d = draws[i][k] (clamped into [0, c)) when draws is given, the ranks of iris_prop_draws(seed) when it is NULL.  Per partner j
 * w = exp(-(|a_i - a_j|^2 / sigma_albedo^2) / 2) exp(-(|p_i - p_j|^2 / sigma_pos^2) / 2);  W_i = 1e-4 + sum w;  l_i = |sum w r_j / W_i - r_i| + |sum w m_j / W_i - m_i|;
 * loss[0] = ls * sum_i l_i / c_i.  One wave per pixel, lane l sums draws k = l, l + 64, ... in that order, fixed-order reductions: bitwise reproducible.
 * Kept for the backward: records (N, 8) f32 (per position a.xyz p.xyz r m), saved (N, 4) f32 (W, sign(rbar - r), sign(mbar - m), 0), both 16-byte aligned;
 * terms (N) f32 scratch.  N = 0 writes loss[0] = 0. */
IRIS_API int iris_prop_semantic_fwd(const int32_t *runs, const int64_t *order, const float *roughness, const float *metallic, const float *albedo,
                           const float *positions, int64_t N, int K, const int64_t *draws, uint64_t seed, double sigma_albedo, double sigma_pos,
                           int normalise, double voxel_min, double voxel_max, float ls, float *records, float *saved, float *terms, float *loss,
                           iris_stream_t);
/* Its gradient for the cotangent g_loss[0] (device), with the forward's runs, order, records, saved, draws / seed, K, sigmas and ls:
 * g_roughness[k] = -sign_r(k) g_k + sum over the draws (i, j = k) of sign_r(i) g_i w_ij / W_i, g_i = ls g_loss / c_i (the partners' r_j are not detached in the
 * reference); g_metallic likewise; albedo and positions get none.  The draws and weights are regenerated.  The propagated part is summed per segment in LDS
 * (segments up to 8192 members; larger ones add straight to memory) and flushed with f32 atomics into g_sorted (2 N f32 scratch, zeroed by the call), so
 * the gradient is reproducible up to summation order, not bitwise.  g_roughness, g_metallic (N) are overwritten. */
IRIS_API int iris_prop_semantic_bwd(const int32_t *runs, const int64_t *order, const float *records, const float *saved, int64_t N, int K, const int64_t *draws,
                           uint64_t seed, double sigma_albedo, double sigma_pos, float ls, const float *g_loss, float *g_sorted, float *g_roughness,
                           float *g_metallic, iris_stream_t);
/* Part branch (:216-238): w_i = (1 - r_i) + 1e-4 (detached), S_s = sum w, M_s = sum w m / S_s, R_s = sum w r / S_s over segment s,
 * loss[0] = lp / N * sum_i (|m_i - M_s(i)| + |r_i - R_s(i)|).  No atomics: bitwise reproducible.  Kept for the backward: seg_means (N, 4) f32, row `start`
 * of a run = (S, M, R, 0), 16-byte aligned; signs (N, 2) f32 (sign(m - M), sign(r - R)) per position, 8-byte aligned; terms (N) scratch. */
IRIS_API int iris_prop_part_fwd(const int32_t *runs, const int64_t *order, const float *roughness, const float *metallic, int64_t N, float lp, float *seg_means,
                       float *signs, float *terms, float *loss, iris_stream_t);
/* g_metallic[k] = lp g_loss / N (sign_m(k) - w_k / S_s sum_{i in s} sign_m(i)), g_roughness likewise with the r signs (no gradient through w); overwritten. */
IRIS_API int iris_prop_part_bwd(const int32_t *runs, const int64_t *order, const float *roughness, const float *seg_means, const float *signs, int64_t N, float lp,
                       const float *g_loss, float *g_roughness, float *g_metallic, iris_stream_t);

/* ---- the trainers' albedo regulariser (train_brdf_crf.py:292-306 with utils/loss.py:14-37; initialize.py:188-201) ---------------------- */
/* Works on the sorted batch of the propagation calls: runs from iris_prop_runs, order = torch.sort(segmentation, stable=True)'s permutation; N < 2^31 - 64.
 * albedo, prior (N, 3) f32 by pixel.  T_s = (sum over segment s of prior) / count, tbar_i = T_s(i);
 *   fit_scale == 0:  k = 1;                                                              (initialize.py:201)
 *   fit_scale != 0:  k = sum(tbar * albedo) / sum(tbar * tbar) over the 3 N entries (utils/loss.py:14-20; the scale multiplies the prior);
 *   loss[0] = weight / (3 N) * sum (k tbar - albedo)^2.
 * k[0] is written on the device and read there by the backward: nothing synchronises.  sum(tbar * tbar) = 0 gives k = NaN and a NaN loss, as the reference.
 * One wave per segment sums the priors lane-strided in position order; every other sum is a fixed tree per 256 positions and one fixed-order pass over
 * those partials; no atomics: two calls on the same inputs agree bit for bit.  Kept for the backward: seg_means (N, 4) f32, row `start` of a run =
 * (T.x, T.y, T.z, 0), other rows unwritten, 16-byte aligned; k.  partials: 3 * min(ceil(N / 256), 4096) f32 of scratch, 8-byte aligned.
 * N = 0 writes loss[0] = 0 and leaves k alone. */
IRIS_API int iris_loss_albedo_fwd(const int32_t *runs, const int64_t *order, const float *albedo, const float *prior, int64_t N, int fit_scale,
                         float weight, float *seg_means, float *partials, float *k, float *loss, iris_stream_t);
/* g_albedo[i] = weight * 2 / (3 N) * g_loss[0] * (albedo_i - k tbar_i) with the forward's seg_means and k (k is a constant of the backward, as the
 * reference's .item() makes it); one plain store per entry, every pixel written once; the prior gets no gradient. */
IRIS_API int iris_loss_albedo_bwd(const int32_t *runs, const int64_t *order, const float *albedo, const float *seg_means, const float *k, int64_t N, float weight,
                         const float *g_loss, float *g_albedo, iris_stream_t);

/* ---- the photometric step loss of the emitter and initialisation stages (train_emitter.py:189-195, initialize.py:180-184), response model frozen ------- */
/* L_sum (B, 3) f32: the integrator's sum over n_calls calls; grid, table, n, exposure, n_exposure, exposure_value: as iris_crf_fwd takes them (below);
 * rgbs_gt (B, 3) f32.  Per entry: L = L_sum / (float)n_calls (a division), rgb = the lookup of iris_crf_fwd (the same bits), d = rgb - gt.
 *   loss[0]  = (sum d^2) / (3 B): squares and sums in double -- xor butterfly per wave, the waves of a workgroup in wave order, the workgroups' partials
 *              in a fixed order by one workgroup --, rounded to f32 once
 *   psnr[0]  = -10 log10(max(loss[0], 1e-5))
 *   dL_sum (B, 3) = ((2 d) / (float)(3 B)) * s / (float)n_calls, s = what iris_crf_bwd gives as g_hdr for g_ldr = 1 (slope * e_i; 0 where hdr * e_i leaves [0, 1]
 *              and on a flat segment): the gradient of loss[0] by L_sum.  Plain stores, every entry once.
 * No gradient by the table or by rgbs_gt.  A pass over the pixels and a one-workgroup pass over its partials, whose number depends on B only; no atomics:
 * two calls on the same inputs agree bit for bit.  workspace: iris_loss_photometric_workspace_bytes(B) bytes (8 * min(ceil(B / 256), 4096)), 8-byte aligned.
 * B >= 1, 1 <= n_calls <= 2^24. */
IRIS_API uint64_t iris_loss_photometric_workspace_bytes(int64_t B);
IRIS_API int iris_loss_photometric(const float *L_sum, int n_calls, const float *grid, const float *table, int n, const float *exposure, int64_t n_exposure,
                          float exposure_value, const float *rgbs_gt, int64_t B, float *loss, float *psnr, float *dL_sum, void *workspace,
                          uint64_t workspace_bytes, iris_stream_t);

/* ---- the camera response model EmorCRF (crf/model_crf.py:32-122) ---------------------------------------------------------------------- */
/* The interpolator is this project's contract (the reference's torch_interpolations is third-party and has no ROCm build: parity unpinned).  Knots p[0..n)
 * non-decreasing, values v[0..n), query q:  r = first index with p[r] >= q, clamped to n - 1 (torch.bucketize);  l = max(r - 1, 0);  dl = max(q - p[l], 0);
 * dr = max(p[r] - q, 0);  both zero -> both 1;  out = (v[l] dr + v[r] dl) / (dl + dr), each operation rounded once, in this order.
 * d out / d q = (v[r] - v[l]) / (dl + dr), 0 where both were zero;  d out / d v[l] = dr / (dl + dr), d out / d v[r] = dl / (dl + dr).
 * grid: (n) f32 knots shared by the three channels.  PRECONDITION: grid is torch.linspace(0, 1, n) in float32 (uniform up to rounding).  The segment
 * is guessed as ceil(q (n - 1)) and corrected by a walk against these values, so it is bucketize's for every q; on the uniform grid the walk takes at
 * most one step.  Any other non-decreasing grid still gives bucketize's segment and in-range reads, but the walk is then O(n) per lookup.  2 <= n <= 1024 (the tables live in LDS).  A NaN or infinite input gives an unspecified value
 * and no out-of-range access.  exposure: device pointer to n_exposure = 1 or B values, or NULL: the host value exposure_value.  B = 0 is a no-op. */
/* model_crf.py:68-86: ldr[i][c] = interp(grid, table[c], clip(hdr[i][c] * e_i, 0, 1)); table (3, n), hdr and ldr (B, 3) */
IRIS_API int iris_crf_fwd(const float *grid, const float *table, int n, const float *hdr, const float *exposure, int64_t n_exposure, float exposure_value,
                 int64_t B, float *ldr, iris_stream_t);
/* model_crf.py:88-106 after get_inv_crf: hdr[i][c] = interp(grid, inv_table[c], clip(ldr[i][c], 0, 1)) / e_i.  No gradient. */
IRIS_API int iris_crf_lookup_inv(const float *grid, const float *inv_table, int n, const float *ldr, const float *exposure, int64_t n_exposure,
                        float exposure_value, int64_t B, float *hdr, iris_stream_t);
/* Gradient of iris_crf_fwd for the cotangent g_ldr (B, 3); either output may be NULL.
 * g_hdr (B, 3) = g_ldr * slope * e_i where 0 <= hdr * e_i <= 1 (torch.clip's gradient: 1 on the closed interval), else 0.
 * g_table (3, n): sum over the pixels of the two weights above times g_ldr (no clip mask: the lookup reads the table at the clipped value too).  Summed
 * per workgroup in LDS, one partial slab per workgroup stored to workspace (iris_crf_bwd_workspace_bytes(B, n) bytes, at most 3 MiB), the slabs added in
 * slab order: no global atomics; reproducible up to the order of the LDS adds inside a workgroup.  The slab count depends on B only. */
IRIS_API uint64_t iris_crf_bwd_workspace_bytes(int64_t B, int n);
IRIS_API int iris_crf_bwd(const float *grid, const float *table, int n, const float *hdr, const float *exposure, int64_t n_exposure, float exposure_value,
                 int64_t B, const float *g_ldr, float *g_hdr, float *g_table, void *workspace, uint64_t workspace_bytes, iris_stream_t);
/* get_inv_crf (model_crf.py:22-30, 45-55) for the three channels in one launch: d = neighbouring differences of table[c]; d += -min(d) if that is negative;
 * d /= sum(d); knots = (0, prefix sums of d); inv_table[c] = interp(knots, values grid, at grid).  A tree sum and a parallel scan: agrees with torch's
 * sequential cumsum up to summation order. */
IRIS_API int iris_crf_inv_table(const float *grid, const float *table, int n, float *inv_table, iris_stream_t);

/* ---- image-quality metrics: SSIM and the squared error behind PSNR (render.py:236-239) ------------------------ */
/* a, b: image stacks (N, H, W, C) float32, interleaved, C 1 or 3, H and W >= 7; data_range R > 0.  The contract is skimage's
 * structural_similarity defaults restated (uniform 7 x 7 window, K1 0.01, K2 0.03, sample covariance, only the windows that lie fully inside the
 * image), with the window moments taken of the window shifted by its own centre pixel -- arithmetic and operation order: iris_amd/csrc/iris_metrics.h.
 * sums (N, C, 2) float64, per image and channel: [0] sum of ((double)a - (double)b)^2 over the H W pixels, [1] sum of S over the (H - 6)(W - 6) windows;
 * PSNR = 10 log10(R^2 C H W / sum_c sums[c][0]), SSIM = mean_c sums[c][1] / ((H - 6)(W - 6)).  ssim_map (N, H - 6, W - 6, C) float32 receives S of
 * every window, or NULL: not written; the sums are the same bits either way.  Partial sums go through workspace
 * (iris_image_metrics_workspace_bytes() bytes, 8-byte aligned; 0: the shape is not supported) with plain stores and are added in a fixed order: no
 * atomics, bitwise reproducible for a given shape.  A non-finite pixel makes its image's sums NaN.  Two launches on the stream. */
IRIS_API uint64_t iris_image_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);
IRIS_API int iris_image_metrics(const float *a, const float *b, int32_t N, int32_t H, int32_t W, int32_t C, float data_range, double *sums,
                       float *ssim_map, void *workspace, uint64_t workspace_bytes, iris_stream_t);

/* ---- material metrics: the sums behind the reference's material table (utils/metric_brdf.py:32-92) ------------- */
/* N views of H x W pixels, every map contiguous (device).  Ground truth as the EXR files hold it, float32: emit_gt, albedo_gt, kd_gt (N, H, W, 3),
 * rough_gt (N, H, W).  Estimates: emit (N, H, W, 3) float32; albedo, kd (N, H, W, 3) and rough (N, H, W), each either uint8 code values (its *_is_u8
 * flag set: a PNG as read) or float32, quantised as the render stage's PNG writer does, q(x) = trunc(min(max(x, 0), 1) * 255.f), NaN -> 0.  The per-pixel
 * contract, in code values and exact, is stated in iris_amd/csrc/iris_matmetrics.h.  sums (N, 8) 8-byte words per view: [0] S_albedo, [1] S_kd, [2] S_rough
 * (sums of squared code differences), [3] n_gt, [4] n_est, [5] n_and, [6] n_or (pixel counts of the two emitter masks, their intersection and union), all
 * uint64; [7] S_emit, a double: the sum over the 3 H W values of (log((double)emit + 1) - log((double)emit_gt + 1))^2, non-finite when a term is.
 * Partial sums go through workspace (iris_material_metrics_workspace_bytes() bytes, 8-byte aligned; 0: the size is not supported -- N, H, W >= 1,
 * H W <= 2^30, N ceil(H W / 512) < 2^31) with plain stores and are added in a fixed order: no atomics, the same bits on every call for a given shape.
 * Two launches on the stream, whatever N. */
typedef struct iris_material_metrics_args {
    const float *emit_gt, *albedo_gt, *kd_gt, *rough_gt;
    const float *emit;
    const void *albedo, *kd, *rough;
    uint64_t *sums;
    void *workspace;
    uint64_t workspace_bytes;
    int32_t albedo_is_u8, kd_is_u8, rough_is_u8;
    int32_t N, H, W;
} iris_material_metrics_args;
IRIS_API uint64_t iris_material_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W);
IRIS_API int iris_material_metrics(const iris_material_metrics_args *, iris_stream_t);

/* ---- the trainers' validation (train_brdf_crf.py:331-499; the same lines in train_emitter.py and initialize.py) -- */
/* validation_step (:456-499) after the material network: N views of H x W pixels, every map contiguous (device).  albedo (N, H W, 3), metallic (N, H W)
 * float32: the network's outputs at the pixel-centre primary hits, for all pixels; valid (N, H W) u8.  Per pixel and channel, each operation one correctly
 * rounded float32 operation (no contraction):  est = valid ? albedo_c * (1.0f - metallic) : 0;  d = gt_c * m - est * m;  q = d * d.
 *   gt_is_u8 == 0 (synthetic): gt (N, H W, 3) float32 (DiffCol), emit (N, H W, 3) float32, lut NULL;  m = ((e0 + e1) + e2 == 0) ? 1 : 0  (:461)
 *   gt_is_u8 != 0 (ldr): gt (N, H W, 3) the photograph's 8-bit codes, read through lut, 256 float32 of the caller's (rgb^(1/2.2) clamped to [0,1], :486),
 *                        emit NULL;  m = 1  (:463)
 * sums (N) doubles, 8-byte aligned: S_n = sum over the view's pixels and channels of (double)q, in a fixed order -- per thread pixels ascending and channels
 * 0, 1, 2; blocks of 512 pixels added by a fixed tree; the blocks' partials, stored into workspace (iris_val_kd_loss_workspace_bytes() bytes, 8-byte aligned;
 * 0: the size is not supported -- N, H, W >= 1, H W <= 2^30, N ceil(H W / 512) < 2^31) with plain stores, added in index order by a second launch.  No
 * atomics: the same bits on every call, and for a view alone or at any row of a stack.  val/loss = S / (3 H W).  Two launches on the stream, whatever N. */
typedef struct iris_val_kd_loss_args {
    const float *albedo, *metallic;
    const uint8_t *valid;
    const void *gt;
    const float *emit;
    const float *lut;
    double *sums;
    void *workspace;
    uint64_t workspace_bytes;
    int32_t gt_is_u8;
    int32_t N, H, W;
} iris_val_kd_loss_args;
IRIS_API uint64_t iris_val_kd_loss_workspace_bytes(int32_t N, int32_t H, int32_t W);
IRIS_API int iris_val_kd_loss(const iris_val_kd_loss_args *, iris_stream_t);
/* validation()'s material maps (:372-396) after the material network, ONE launch over iris_render_primary's outputs (the same un-centred jitter).  Per sample
 * i = b*spp + s (N = B*spp rows, pixel-major): e0, valid_next as iris_render_primary gives them; albedo (N,3), roughness (N), metallic (N) = material_net(pos);
 * radiance: the emitter's (n_rad,3) tensor itself (rows beyond the emitter handle's count are never read).
 *   emission_ = e0 >= 0 ? radiance[e0] : 0;  keep = (valid_next | e0 >= 0) & ((emission_.r + emission_.g) + emission_.b == 0);
 *   albedo_ = keep ? albedo : 0; roughness_ = keep ? roughness : 0; metallic_ = keep ? metallic : 0; emission_ is not masked.
 * A masked sample counts as 0 (iris_render_intrinsics: as the default material), and it is SELECTED, where the reference multiplies by 0 (:393-395): the two
 * differ only where the network returns a non-finite value at a masked sample.
 * SUMMATION ORDER (a contract):  map[b] += (x_0 + x_1 + ... + x_{spp-1}) * (1.0f / spp), samples added in increasing s, in float32, as iris_render_intrinsics.
 * The four maps are the caller's: albedo_map (B,3), roughness_map (B), metallic_map (B), emission (B,3).  No atomics, every element written by one thread:
 * bitwise reproducible.  spp: any positive int. */
IRIS_API int iris_val_intrinsics(const iris_emitter *, const float *radiance, const int32_t *e0, const uint8_t *valid_next, const float *albedo,
                        const float *roughness, const float *metallic, int64_t B, int spp, float *albedo_map, float *roughness_map, float *metallic_map,
                        float *emission, iris_stream_t);

/* ---- texture export: UV rasteriser, per-texel resolve, quantisation (utils/export.py:77-135) ------------------- */
/* The reference rasterises the UV triangles with nvdiffrast (third party, GL): parity is unpinned and the contract is this project's, exact in integers
 * (iris_amd/csrc/iris_texture.h).  Texture of H rows x W columns, both in [1, 8192]; texel (r, c) has its centre at
 * u = (c + .5) / W, v = (r + .5) / H, row 0 at v ~ 0.  vt (n_vt, 2) float32 UVs (finite, in [-1, 2]: the caller checks), ft (F, 3) int32 indices into vt;
 * v (n_v, 3) float32 positions, f (F, 3) int32 indices into v.  UVs are snapped to 1 / 256 texel, coverage is decided by int64 edge functions with a
 * top-left rule, the lowest face index wins where triangles overlap.  A triangle that names a vertex out of range covers nothing.
 * iris_uv_raster: ids (H W) int32 receives the face index per texel, -1 where uncovered.  workspace: iris_uv_raster_workspace_bytes(F) bytes, 8-byte
 *   aligned.  Integer atomicMin only: the result does not depend on scheduling.  Two memsets and two launches on the stream.
 * iris_uv_resolve: for the texels [texel0, texel0 + n) of a texture rasterised into ids: bary (n, 2) float32 (weights of vertices 0 and 1; NULL: not
 *   written) and xyz (n, 3) float32, the position interpolated in float32 as ((b0 v0) + (b1 v1)) + (b2 v2), b2 = 1 - b0 - b1.  Uncovered: zeros.
 * iris_texture_quantize: albedo (n, 3), roughness (n), metallic (n) float32 of the same texel range -> bytes 3 texel0 .. 3 (texel0 + n) of the two uint8
 *   RGB images of n_texels texels (albedo; roughness, metallic, 0): clamp to [0, 1] with NaN -> 0, times 255 in float32, truncated; 0 where ids < 0.
 *   The images must be 4-byte aligned. */
IRIS_API uint64_t iris_uv_raster_workspace_bytes(int64_t F);
IRIS_API int iris_uv_raster(const float *vt, int64_t n_vt, const int32_t *ft, int64_t F, int32_t H, int32_t W, int32_t *ids, void *workspace,
                   uint64_t workspace_bytes, iris_stream_t);
IRIS_API int iris_uv_resolve(const float *vt, int64_t n_vt, const int32_t *ft, const float *v, int64_t n_v, const int32_t *f, int64_t F, int32_t H, int32_t W,
                    const int32_t *ids, int64_t texel0, int64_t n, float *bary, float *xyz, iris_stream_t);
IRIS_API int iris_texture_quantize(const float *albedo, const float *roughness, const float *metallic, const int32_t *ids, int64_t texel0, int64_t n,
                          int64_t n_texels, uint8_t *albedo_img, uint8_t *rm_img, iris_stream_t);

/* ---- texture export: the area-proportional atlas and the seam dilation (no counterpart in the reference, which calls xatlas) ---- */
/* One chart per face, sized by the face's area: exact in integers and float64 (iris_amd/csrc/iris_atlas.h; restated in numpy by
 * tests/atlas_ref.py).  tex_res = R: a square power of two in [4, 8192]; F at most 2^23 (two faces per 4 x 4 cell of the largest texture).
 * iris_atlas_measure: v (n_v, 3) float32, f (F, 3) int32 -> S (F) float64 and corner (F) uint8.  In float64, every product and sum rounded on its own, sums
 *   left to right: e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2, S = cx^2 + cy^2 + cz^2 (four times the squared area; no square root anywhere); l0 = |p2 - p1|^2,
 *   l1 = |p0 - p2|^2, l2 = |p1 - p0|^2; corner = argmax(l0, l1, l2), first maximum: the vertex opposite the longest edge.  A face that names a vertex outside
 *   [0, n_v), or whose S is not finite or not > 0, gets S = 0 and corner = 0.
 * iris_atlas_density: D_j = M[j mod 2] 2^floor(j / 2), M = (1, 1.4142135623730951), the squared number of texels per unit area at step j of the ladder
 *   [-800, 800]; 0 outside it.  A host function.
 * iris_atlas_classes: S, j -> k (F) uint8 and hist (16 int64 on the device, zeroed by the call).  A cell of class k is 2^k x 2^k texels, KMIN = 2,
 *   2^KMAX = R; k_f is the smallest k in [KMIN, KMAX] with 4 16^k >= S_f D_j (one rounded product), KMAX when none (S = 0 gives KMIN).  hist[k] counts the
 *   faces of class k, hist[14] those the lower clamp raised (64 >= S_f D_j), hist[15] those no class in range satisfies.  Integer atomics only: the counters
 *   do not depend on scheduling.  Two faces share a cell, cells_k = ceil(hist[k] / 2); step j FITS when sum_k cells_k 4^k <= R^2.  Every k_f is
 *   non-decreasing in j; the sum is too, except where a face that moves up fills the free half of a cell of the next class (the sum then drops by the cell it
 *   left).  The step used is the one ONE stated bisection returns: lo = -800 (it must fit), hi = 801; mid = floor((lo + hi) / 2) becomes lo when it fits and
 *   hi when not, until hi - lo = 1; j = lo.  That j fits and j + 1 does not (or j = 800); past such a dip a larger step may fit, and is not looked for.  One
 *   memset and one launch on the stream.
 * iris_atlas_place: k and corner as above, order (F) int64 = the faces sorted by class with the face index breaking ties (a STABLE sort of k), hist_host =
 *   the 14 class counters of the chosen step ON THE HOST -> vt (3 F, 2) float32; ft is arange(3 F).  Refused unless the counters sum to F and fit.  Position
 *   i of order is rank r = i - (faces of lower classes) of its class and sits in cell r / 2 of that class, the lower half for even r, the upper half for odd r.
 *   Classes are laid out from the largest down: base_k = sum_{k' > k} cells_k' 4^k', texel offset o = base_k + (r / 2) 4^k, and the cell's corner is
 *   x0 = the even bits of o compacted, y0 = the odd bits (Morton order): o is a multiple of 4^k, so the cells tile without overlap.  With x1 = x0 + 2^k,
 *   y1 = y0 + 2^k, in texels:  lower P0 = (x0 + .25, y0 + .25), P1 = (x1 - .5, y0 + .25), P2 = (x0 + .25, y1 - .5);  upper P0 = (x1 - .25, y1 - .25),
 *   P1 = (x0 + .5, y1 - .25), P2 = (x1 - .25, y0 + .5).  Mesh corner (corner + i) mod 3 takes P_i / R: the winding is kept, the longest edge lies on the
 *   diagonal, and the float32 UVs are exact.  One launch.
 * iris_texture_dilate: ids (H, W) int32 as iris_uv_raster leaves it, the two (H, W, 3) uint8 images of iris_texture_quantize, 0 <= n <= 4, any H and W
 *   in [1, 8192].  An uncovered texel (ids < 0) takes the bytes of the covered texel within Chebyshev distance n with the smallest squared Euclidean
 *   distance, then the smallest row, then the smallest column; none: left as it is.  In place, one launch (none for n = 0): covered texels are only read,
 *   uncovered ones only written.  ids is not changed. */
IRIS_API int iris_atlas_measure(const float *v, int64_t n_v, const int32_t *f, int64_t F, double *S, uint8_t *corner, iris_stream_t);
IRIS_API double iris_atlas_density(int32_t j);
IRIS_API int iris_atlas_classes(const double *S, int64_t F, int32_t j, int32_t tex_res, uint8_t *k, int64_t *hist, iris_stream_t);
IRIS_API int iris_atlas_place(const uint8_t *k, const uint8_t *corner, const int64_t *order, int64_t F, int32_t tex_res, const int64_t *hist_host, float *vt,
                     iris_stream_t);
IRIS_API int iris_texture_dilate(const int32_t *ids, int32_t H, int32_t W, int32_t n, uint8_t *albedo_img, uint8_t *rm_img, iris_stream_t);

/* ---- OpenEXR ZIP / ZIPS writer, device half ------------------------------------------------------------- */
/* Deflate of the scanline blocks of n_maps maps (utils/exr.py scanline_blocks_torch): full (n_maps, n_full, block_bytes) and tail (n_maps, tail_bytes)
 * hold the PREDICTED bytes (reordered, delta-coded) of every block, device uint8, contiguous.  records receives, map by map, every chunk record as the
 * file stores it (int32 y = chunk * lines_per_block, int32 size, data): data is a zlib stream of the predicted bytes when that is shorter than the block,
 * else the raw (un-predicted) block -- OpenEXR's ZIP rule.  records must hold n_maps * (n_full * (block_bytes + 8) + (tail_bytes ? tail_bytes + 8 : 0))
 * bytes; map_offsets (device int64, n_maps + 1) receives where each map's records start and, last, their total size.  workspace: device scratch of
 * iris_exr_zip_workspace_bytes() bytes (0: the sizes are not supported).  Four launches on the stream, no host round trip. */
IRIS_API uint64_t iris_exr_zip_workspace_bytes(int n_maps, int64_t n_full, int64_t block_bytes, int64_t tail_bytes);
IRIS_API int iris_exr_zip_encode(const uint8_t *full, const uint8_t *tail, int n_maps, int64_t n_full, int64_t block_bytes, int64_t tail_bytes,
                        int lines_per_block, uint8_t *records, int64_t *map_offsets, void *workspace, uint64_t workspace_bytes, iris_stream_t);

/* ---- 8-bit PNG files, device half (render_video.py's eight files per frame; utils/png.py) ----------------- */
/* iris_png_rows: n_images equal-size images (H, W, channels), channels 1 or 3, float32 or (is_u8) uint8, device pointers -> their PNG scanline bytes.  Per
 * float value v = x / divisor (IEEE), NaN -> 0, clamp to [0,1], q = (uint8) trunc(v * 255): (np.clip(image, 0, 1) * 255).astype(np.uint8).  A magma image
 * (channels 1) sends q through OpenCV's COLORMAP_MAGMA and is written as RGB.  The image is cropped to even height and width (H2, W2) and every row is
 * written as [1][Sub-filtered bytes] (PNG filter type 1, bpp = output channels): rows (device) receives n_images blocks of
 * iris_png_row_bytes(H, W, channels, magma) = H2 * (1 + W2 * output channels) bytes (0: such an image cannot be written -- an empty crop, channels not
 * 1 or 3, magma with 3 channels).  `images`, `divisors` and `magma` are HOST arrays of n_images entries (they travel in the kernel arguments); the images
 * of one call are all magma or none is.  One launch per 16 images.
 * iris_png_encode: rows = n_images blocks of block_bytes (device) -> streams: the zlib stream (RFC 1950) of each block, back to back; offsets (device int64,
 * n_images + 1): where each starts and, last, their total size.  The encoder is iris_exr_zip_encode's (segments of 16 KiB, one deflate block each, matches
 * at distance 1, a stored block when that is not larger); every image is one chunk and its output is always the stream.  streams must hold n_images *
 * iris_png_stream_bound(block_bytes) bytes (header 2 + at most block_bytes + 5 per segment + Adler-32 4); workspace: iris_png_workspace_bytes() bytes
 * (0: unsupported size).  Four launches, no host round trip.  iris_png_magma_table: the 256 x 3 R,G,B table (HOST pointer, 768 bytes). */
IRIS_API int64_t iris_png_row_bytes(int H, int W, int channels, int magma);
IRIS_API int iris_png_rows(const void *const *images, const float *divisors, const uint8_t *magma, int n_images, int H, int W, int channels, int is_u8,
                  uint8_t *rows, iris_stream_t);
IRIS_API uint64_t iris_png_stream_bound(int64_t block_bytes);
IRIS_API uint64_t iris_png_workspace_bytes(int n_images, int64_t block_bytes);
IRIS_API int iris_png_encode(const uint8_t *rows, int n_images, int64_t block_bytes, uint8_t *streams, int64_t *offsets, void *workspace,
                    uint64_t workspace_bytes, iris_stream_t);
IRIS_API void iris_png_magma_table(uint8_t *rgb);

/* ---- baseline JPEG frames, device half (render_video.py --video mjpeg; utils/jpeg.py; the contract: DESIGN.md 5c-14) ----------------- */
/* iris_jpeg_encode: n_images equal-size images as iris_png_rows takes them (the same quantiser, MAGMA table and even crop (H2, W2); magma per image) -> the
 * entropy-coded data of one baseline JPEG each: Y Cb Cr at 2x2 1x1 1x1 whatever the input (a grey map has Cb = Cr = 128), integer colour conversion and DCT,
 * the Annex K tables scaled by `quality` (1..100, the IJG rule), one restart interval per MCU row (byte-aligned with 1-bits, FF -> FF 00, RSTm after every
 * interval but the last).  streams (device) receives the data back to back -- what stands between the SOS header and EOI --, offsets (device int64,
 * n_images + 1) where each starts and, last, their total size.  streams must hold n_images * iris_jpeg_stream_bound(H, W) bytes: per MCU row twice the
 * longest bit string the tables can produce (22 bits for a DC and 26 for each of 63 AC coefficients per block, six blocks per MCU) plus the marker -- many
 * times the raw image, so copy offsets first and then the used bytes.  workspace: iris_jpeg_workspace_bytes() bytes.  Both return 0 for an unsupported size
 * (an empty crop, more than 65535 pixels a side).  One launch per 16 images and four more on the stream, no host round trip.
 * iris_jpeg_tables (HOST pointer, 604 bytes): the luma and chroma quantisation tables of Annex K in natural order (2 x 64), the natural index of every
 * zigzag position (64), then BITS (16) and HUFFVAL of the tables DC luma (12), AC luma (162), DC chroma (12), AC chroma (162): what the file's headers hold. */
IRIS_API uint64_t iris_jpeg_stream_bound(int H, int W);
IRIS_API uint64_t iris_jpeg_workspace_bytes(int n_images, int H, int W);
IRIS_API int iris_jpeg_encode(const void *const *images, const float *divisors, const uint8_t *magma, int n_images, int H, int W, int channels, int is_u8,
                     int quality, uint8_t *streams, int64_t *offsets, void *workspace, uint64_t workspace_bytes, iris_stream_t);
IRIS_API void iris_jpeg_tables(uint8_t *out);

/* ---- 8-bit image resize, device half (the scannetpp layout's --res_scale; utils/resize.py; the contract: DESIGN.md 5c-15) ----------------- */
/* iris_resize_tables (HOST function, HOST pointers, no device needed): one axis of ns source and nd destination samples (1..65535 each) -> ofs (nd) the
 * first source index of every destination sample and, for IRIS_RESIZE_LINEAR, coef (nd, 2) the int16 weights of that sample and the next (index
 * min(s + 1, ns - 1)); IRIS_RESIZE_NEAREST fills ofs only (coef may be NULL).
 *   linear: OpenCV's 8-bit INTER_LINEAR: scale = 1 / (nd / ns) in double, f = float32((d + 0.5) scale - 0.5), s = floor(f), f = float32(f - s); s < 0 -> s = 0,
 *           f = 0; s >= ns - 1 -> s = ns - 1, f = 0; weights rint(float32(1 - f) 2048), rint(f 2048), half to even.
 *   nearest: PIL's Image.NEAREST: a = ns / nd in double, x = a / 2, then per sample in order index min(floor(x), ns - 1) and x += a (accumulated addition).
 * iris_resize_u8: n_images equal-size uint8 images (Hs, Ws, channels), channels 1 or 3 interleaved, device pointers in a HOST array (they travel in the
 * kernel arguments, as iris_png_rows') -> out (device): n_images blocks of Ht * Wt * channels bytes.  The tables are DEVICE copies of
 * iris_resize_tables' for (Ws, Wt) and (Hs, Ht).  Linear: horizontal R = S[s] w0 + S[s+1] w1 in int32, vertical
 * (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2; when Hs == 2 Ht and Ws == 2 Wt (both) the library takes OpenCV's exact-2 path itself,
 * (a + b + c + d + 2) >> 2 over each 2 x 2 block, and the tables are unused (may be NULL).  Nearest: out[y][x] = S[yofs[y]][xofs[x]]; the weights are
 * unused.  All-integer and free of atomics: bitwise reproducible.  One launch per 16 images, no host round trip. */
enum { IRIS_RESIZE_LINEAR = 0, IRIS_RESIZE_NEAREST = 1 };
IRIS_API int iris_resize_tables(int mode, int ns, int nd, int32_t *ofs, int16_t *coef);
IRIS_API int iris_resize_u8(const void *const *images, int n_images, int Hs, int Ws, int channels, int mode, const int32_t *xofs, const int16_t *xcoef,
                   const int32_t *yofs, const int16_t *ycoef, uint8_t *out, int Ht, int Wt, iris_stream_t);

/* ---- 5c-17: the exported textures read back (utils/closest.py, model/texture.py; the contracts: DESIGN.md 5c-17) ----------------- */
/* iris_closest_point: per query point xs[i] (B, 3) the closest point of the scene's mesh.  tri (B) int64 = the ORIGINAL face index, -1 when there is none (a
 * mesh without a triangle of non-zero area, a query point that is not finite); bary (B, 2) = (b1, b2) as iris_intersect's uv, b1, b2 >= 0, b1 + b2 <= 1;
 * pos (B, 3) = (1 - b1 - b2) p0 + b1 p1 + b2 p2 as iris_intersect interpolates it; dist2 (B) the squared distance as computed, +inf when tri = -1.  Any output
 * pointer may be NULL.  The closest point of a triangle is the vertex / edge / interior classification in float32; the winner is the lexicographic minimum of
 * (dist2, original index); triangles whose float32 cross product is exactly zero are skipped.  A scene in the default layout (IRIS_BVH4_Q8) only.  No atomics, no
 * workspace, bitwise reproducible.  One launch; B = 0 launches nothing.
 * iris_texture_sample: tri (B) int64 and bary (B, 2) as above, ft (F, 3) int32 and vt (n_vt, 2) f32 the UV triangles of the export, the two (H, W, 3) uint8
 * images, H and W in [1, 8192] -> albedo (B, 3), roughness (B), metallic (B) f32: a bilinear fetch in the rasteriser's texel convention (texel (r, c) has its
 * centre at u = (c + .5) / W, v = (r + .5) / H), bytes as byte / 255, lerp form; albedo linear, roughness = max(channel 0 of rm, 0.02), metallic = channel 1 of
 * rm; tri outside [0, F) gives zeros and roughness 0.02.
 * iris_texture_material: iris_closest_point, then iris_texture_sample at its (tri, bary), as ONE launch and bit for bit the two-call composition. */
IRIS_API int iris_closest_point(const iris_scene *, const float *xs, int64_t B, int64_t *tri, float *bary, float *pos, float *dist2, iris_stream_t);
IRIS_API int iris_texture_sample(const int64_t *tri, const float *bary, int64_t B, const int32_t *ft, int64_t F, const float *vt, int64_t n_vt,
                        const uint8_t *albedo_img, const uint8_t *rm_img, int32_t H, int32_t W, float *albedo, float *roughness, float *metallic, iris_stream_t);
IRIS_API int iris_texture_material(const iris_scene *, const float *xs, int64_t B, const int32_t *ft, int64_t F, const float *vt, int64_t n_vt,
                          const uint8_t *albedo_img, const uint8_t *rm_img, int32_t H, int32_t W, float *albedo, float *roughness, float *metallic, iris_stream_t);

/* ---- 5c-20: the trainable texture (model/texture.py TextureBRDF, utils/texture.py fit_textures; the contract: DESIGN.md 5c-20) ----------------- */
/* iris_texture_sample_f32: iris_texture_sample with ONE float32 image texels (H, W, 5) = albedo r, g, b, roughness, metallic per texel in place of the two 8-bit
 * images: the same float32 UV, clamp, taps and lerp form, step for step; the taps are the texel values themselves (no / 255); roughness = max(lerp, 0.02); tri
 * outside [0, F) gives zeros and roughness 0.02.  With texels = byte / 255 (a float32 division) the outputs equal iris_texture_sample's bit for bit.
 * iris_texture_sample_f32_bwd: the same point inputs and texels, and the outputs' gradients g_albedo (B, 3), g_roughness (B), g_metallic (B); ADDS into g_texels
 * (H, W, 5), which the caller zeroes (or keeps, to accumulate): per point and channel w00 g, w01 g, w10 g, w11 g to the four taps, w00 = (1 - fx)(1 - fy),
 * w01 = fx (1 - fy), w10 = (1 - fx) fy, w11 = fx fy in float32; taps that the clamp merges (x1 == x0, y1 == y0) sum on one texel.  The roughness gradient passes
 * only where the interpolated value is > 0.02; rows without a triangle add nothing; there is no gradient for bary, vt or positions.  The adds are float atomics on
 * global memory, twenty per point: REPRODUCIBLE TO ROUNDING, NOT BIT FOR BIT (the arrival order is not fixed); per texel channel within (n + 4) 2^-24 sum |w g| of the
 * exact sum over its n contributions.  Both: one launch, a grid-stride loop over B with 64-bit indices; B = 0 launches nothing; H and W in [1, 8192]. */
IRIS_API int iris_texture_sample_f32(const int64_t *tri, const float *bary, int64_t B, const int32_t *ft, int64_t F, const float *vt, int64_t n_vt,
                            const float *texels, int32_t H, int32_t W, float *albedo, float *roughness, float *metallic, iris_stream_t);
IRIS_API int iris_texture_sample_f32_bwd(const int64_t *tri, const float *bary, int64_t B, const int32_t *ft, int64_t F, const float *vt, int64_t n_vt,
                                const float *texels, int32_t H, int32_t W, const float *g_albedo, const float *g_roughness, const float *g_metallic,
                                float *g_texels, iris_stream_t);

/* ---- misc --------------------------------------------------------------------------------------------- */
/* Philox uniforms exactly as the bake kernels draw them (for tests): u2[i] = U(seed, idx0+i, stream_id). */
IRIS_API int iris_philox_u2(uint64_t seed, uint64_t idx0, uint32_t stream_id, int64_t n, float *u2, iris_stream_t);
IRIS_API const char *iris_last_error(void);
IRIS_API const char *iris_version(void);

/* ---- the rays of a per-view call (iris_pool_view, iris_label_vote, iris_label_view): the first member of its argument structure -------- */
/* camera != NULL: HOST pointer to 24 floats K[9] | c2w[12] | focal | 2 pad (a row of the trainers' camera table); the rays are those of
 * iris_raygen_real / iris_raygen_synthetic (ray_diff = 0) for pixel i = y W + x of an H x W view, and B is H W.  camera == NULL: B explicit rays,
 * ray i at rays_o + i ray_stride and rays_d + i ray_stride floats (device; ray_stride >= 3; an (N,6) tensor: rays_d = rays_o + 3, ray_stride = 6). */
typedef struct {
    const float *camera;
    int32_t H, W, synthetic;
    const float *rays_o, *rays_d;
    int64_t ray_stride, B;
} iris_view_rays;

/* ---- 5c-11: one view's primary hits pooled where they land (slf_bake.py, slf_refine.py, extract_emitter_ldr.py) -------- */
/* One launch per view and pass: per pixel a primary ray, its closest hit (iris_intersect's traversal and position, bit for bit) and, for a hit, any subset
 * of four sinks, selected by which pointers are non-NULL (none: the launch only traces).  A miss contributes to nothing.  No intermediate tensors, no
 * host synchronisation.  Float sums are float atomics: equal to a sequential scatter up to summation order; counts, histogram and bounds are exact. */
typedef struct {
    iris_view_rays rays;
    /* radiance of ray i: row i of a (B,3) store, uint8 decoded as float(double(u) / 255) or float32 as stored; NULL when no pooling sink is given.
     * crf_grid != NULL: passed through the inverse response, interp(crf_grid, crf_inv_table[c], clip(v, 0, 1)) / exposure -- iris_crf_lookup_inv's
     * arithmetic and its exposure convention (exposure NULL: exposure_value; else n_exposure = 1 or B device values). */
    const void *rgb;
    int32_t rgb_is_u8;
    const float *crf_grid, *crf_inv_table;
    int32_t crf_n;
    const float *exposure;
    int64_t n_exposure;
    float exposure_value;
    /* sink 1, bounds: 2 device floats [min, max] over all three coordinates of all hit positions; the caller initialises them (the reference: 1000, 0).
     * Reduced per wave and workgroup, two integer atomics per workgroup; a zero's sign is not kept. */
    float *bounds;
    /* sink 2, occupancy: hist (hist_H^3) f32 [z][y][x] += 1, iris_voxel_histogram's voxel of the position */
    float *hist;
    double voxel_min, voxel_max;
    int32_t hist_H;
    /* sink 3, voxel pool: iris_slf_scatter_add of (position, radiance); a position in an empty voxel is dropped */
    const iris_slf *slf;
    float *slf_acc;
    int64_t *slf_count;
    /* sink 4, triangle pool: tri_sum (n_tri,3) += radiance and tri_count (n_tri) f32 += 1 (nullable) at the hit triangle: iris_scatter_add_rows */
    float *tri_sum, *tri_count;
    int64_t n_tri;
} iris_pool_view_args;
IRIS_API int iris_pool_view(const iris_scene *, const iris_pool_view_args *, iris_stream_t);

/* ---- 5c-16: segmentation fusion (utils/fuse_segmentation.py): per-triangle label vote, the rows' winners, a view painted from a table -------- */
/* One launch per view for the vote and for the painting: per pixel a primary ray and its closest hit (iris_intersect's traversal, bit for bit).  No
 * intermediate tensors, no host synchronisation.  Every result is an integer count or a copy of a table entry: exact and bitwise reproducible. */
typedef struct {
    iris_view_rays rays;
    /* rows of hist / entries of table (the scene's triangle count); a hit on a triangle index >= n_tri is treated as a miss */
    int64_t n_tri;
    /* iris_label_vote.  ids: the id of pixel i, B values (device), float32 -- truncated toward zero, torch's .long() -- or uint8.  hist: (n_tri, n_labels)
     * uint32 (device), hist[tri n_labels + id] += 1 for a hit with 1 <= id < n_labels.  Ids that are 0, negative, NaN, infinite or >= n_labels are
     * dropped, and so are misses; column 0 is never written.  iris_label_view ignores these four. */
    const void *ids;
    int32_t ids_is_u8;
    uint32_t *hist;
    int32_t n_labels;
    /* iris_label_view.  table: n_tri int32 (device).  out: B values (device), out[i] = table[tri] on a hit and miss_value otherwise, written as float32
     * or, with out_is_u8, as the value's low byte (miss_value -1 -> 255, a table entry 300 -> 44).  iris_label_vote ignores these four. */
    const int32_t *table;
    void *out;
    int32_t out_is_u8, miss_value;
} iris_label_view_args;
IRIS_API int iris_label_vote(const iris_scene *, const iris_label_view_args *, iris_stream_t);
/* tri_label[t] (F int32, device) = the column c in [1, n_labels) of row t of hist (F, n_labels) uint32 with the highest count -- counts compare as unsigned,
 * equal counts go to the LOWER column (the first occurrence, as numpy's and torch-CPU's argmax) --, or 0 when every such column is 0.  Column 0 is not
 * read.  One wave per row. */
IRIS_API int iris_label_argmax(const uint32_t *hist, int64_t F, int32_t n_labels, int32_t *tri_label, iris_stream_t);
IRIS_API int iris_label_view(const iris_scene *, const iris_label_view_args *, iris_stream_t);

#ifdef __cplusplus
}
#endif
#endif /* IRIS_HIP_H */
