"""ctypes binding of libiris_hip.so (include/iris_hip.h).  Fails loudly when the library is missing."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IRIS_HIP_LIB") or os.path.join(_HERE, "libiris_hip.so")   # IRIS_HIP_LIB: A/B builds of the same ABI

BVH_DEFAULT, BVH4_F32, BVH4_Q8 = 0, 1, 3
BAKE_AUTO, BAKE_PIXEL_PER_WAVE, BAKE_TILE_SORTED = 0, 1, 2


class IrisError(RuntimeError):
    pass


class SceneInfo(C.Structure):
    _fields_ = [("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("layout", C.c_int32), ("n_nodes", C.c_int32),
                ("node_bytes", C.c_int32), ("tri_bytes", C.c_int32), ("depth", C.c_int32), ("n_leaf_records", C.c_int32),
                ("sah_cost", C.c_float), ("build_seconds", C.c_float)]


_P, _I64, _I32, _F, _D, _U64, _U32 = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_uint64, C.c_uint32


class ViewRays(C.Structure):
    """iris_view_rays (include/iris_hip.h), filled by utils.gbuffer.view_rays_args"""
    _fields_ = [("camera", _P), ("H", C.c_int32), ("W", C.c_int32), ("synthetic", C.c_int32), ("rays_o", _P), ("rays_d", _P), ("ray_stride", _I64), ("B", _I64)]


class PoolViewArgs(C.Structure):
    """iris_pool_view_args (include/iris_hip.h); a field left alone is NULL / 0"""
    _fields_ = [("rays", ViewRays), ("rgb", _P), ("rgb_is_u8", C.c_int32), ("crf_grid", _P), ("crf_inv_table", _P), ("crf_n", C.c_int32), ("exposure", _P), ("n_exposure", _I64),
                ("exposure_value", _F), ("bounds", _P), ("hist", _P), ("voxel_min", _D), ("voxel_max", _D), ("hist_H", C.c_int32), ("slf", _P), ("slf_acc", _P),
                ("slf_count", _P), ("tri_sum", _P), ("tri_count", _P), ("n_tri", _I64)]


class LabelViewArgs(C.Structure):
    """iris_label_view_args (include/iris_hip.h); a field left alone is NULL / 0"""
    _fields_ = [("rays", ViewRays), ("n_tri", _I64), ("ids", _P), ("ids_is_u8", C.c_int32), ("hist", _P), ("n_labels", C.c_int32), ("table", _P), ("out", _P),
                ("out_is_u8", C.c_int32), ("miss_value", C.c_int32)]

class MaterialMetricsArgs(C.Structure):
    """iris_material_metrics_args (include/iris_hip.h)"""
    _fields_ = [("emit_gt", _P), ("albedo_gt", _P), ("kd_gt", _P), ("rough_gt", _P), ("emit", _P), ("albedo", _P), ("kd", _P), ("rough", _P), ("sums", _P),
                ("workspace", _P), ("workspace_bytes", _U64), ("albedo_is_u8", C.c_int32), ("kd_is_u8", C.c_int32), ("rough_is_u8", C.c_int32),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class ValKdLossArgs(C.Structure):
    """iris_val_kd_loss_args (include/iris_hip.h); a field left alone is NULL / 0"""
    _fields_ = [("albedo", _P), ("metallic", _P), ("valid", _P), ("gt", _P), ("emit", _P), ("lut", _P), ("sums", _P), ("workspace", _P),
                ("workspace_bytes", _U64), ("gt_is_u8", C.c_int32), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]

# name -> argtypes (restype is int unless listed in _RESTYPE)
PROTOTYPES = {
    "iris_scene_create": [_P, _I64, _P, _I64, _I32, C.POINTER(_P)],
    "iris_debug_scene_create": [_P, _I64, _P, _I64, _I32, _I32, C.POINTER(_P)],
    "iris_scene_destroy": [_P],
    "iris_scene_get_info": [_P, C.POINTER(SceneInfo)],
    "iris_slf_create": [_P, _I32, _P, _I64, _D, _D, _I32, C.POINTER(_P)],
    "iris_slf_create_dev": [_P, _I32, _P, _I64, _D, _D, _I32, C.POINTER(_P), _P],
    "iris_slf_set_radiance": [_P, _P, _I64, _P],
    "iris_slf_destroy": [_P],
    "iris_emitter_create": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I32, C.POINTER(_P)],
    "iris_emitter_set_radiance": [_P, _P, _I64, _P],
    "iris_emitter_destroy": [_P],
    "iris_raygen_real": [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P],
    "iris_raygen_synthetic": [_F, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P],
    "iris_pixel_batch": [_P, _I64, _P, _I64, _I32, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "iris_intersect": [_P, _P, _P, _I64, _P, _P, _P, _P, _P, _P],
    "iris_sample_diffuse": [_P, _P, _I64, _P, _P, _P, _P],
    "iris_sample_specular": [_P, _P, _P, _F, _I64, _P, _P, _P, _P, _P],
    "iris_sample_specular_v": [_P, _P, _P, _P, _I64, _P, _P, _P, _P, _P],
    "iris_slf_lookup": [_P, _P, _I64, _P, _P, _P],
    "iris_eval_emitter": [_P, _P, _P, _P, _P, _F, _I64, _P, _P, _P, _P],
    "iris_bake_workspace_bytes": [_I64, _I32, _I32],
    "iris_bake_diffuse": [_P, _P, _P, _P, _P, _I64, _I32, _P, _U64, _U32, _P, _P, _P, _P, _U64, _P],
    "iris_bake_specular": [_P, _P, _P, _P, _P, _P, _F, _I64, _I32, _P, _U64, _U32, _P, _P, _P, _P, _P, _U64, _P],
    "iris_debug_bake_diffuse": [_P, _P, _P, _P, _P, _I64, _I32, _P, _U64, _U32, _P, _P, _P, _P, _P, _I32, _P, _U64, _P],
    "iris_debug_bake_specular": [_P, _P, _P, _P, _P, _P, _F, _I64, _I32, _P, _U64, _U32, _P, _P, _P, _P, _P, _P, _I32, _P, _U64, _P],
    "iris_debug_set": [C.c_char_p, C.c_longlong],
    "iris_debug_build_flags": [],
    "iris_debug_source_hash": [],
    "iris_bake_view": [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _U64, _P, _P, _P, _U64, _P],
    "iris_lerp_specular": [_P, _P, _I64, _I32, _P, _P],
    "iris_unstripe_maps": [_P, _I32, _I32, _I64, _I32, _I32, _I32, _P, _P],
    "iris_get_normal_space": [_P, _I64, _P, _P],
    "iris_double_sided": [_P, _P, _I64, _P],
    "iris_angle2xyz": [_P, _P, _I64, _P, _P],
    "iris_ggx_terms": [_I32, _P, _P, _P, _I64, _P, _P, _P],
    "iris_philox_u2": [_U64, _U64, _U32, _I64, _P, _P],
    "iris_ngp_n_params": [],
    "iris_ngp_create": [_P, _I64, C.c_double, C.c_double, C.c_int, _P],
    "iris_ngp_forward": [_P, _P, _I64, _P, _P, _P, _P],
    "iris_ngp_set_params_dev": [_P, _P, _I64, _P],
    "iris_ngp_backward_workspace_bytes": [_I64],
    "iris_ngp_backward": [_P, _P, _I64, _P, _P, _P, _F, _P, _P, C.c_uint64, _P],
    "iris_ngp_destroy": [_P],
    "iris_adam_step": [_P, _P, _P, _P, _I64, _I64, _D, _D, _D, _D, _D, _P],
    "iris_ngp_adam_step": [_P, _P, _P, _P, _P, _I64, _I64, _D, _D, _D, _D, _D, _P],
    "iris_debug_ngp_encode": [_P, _P, _I64, _P, _P],
    "iris_sample_emitter": [_P, _P, _P, _P, _I64, _P, _P, _P, _P],
    "iris_eval_brdf": [_P, _P, _P, _P, _P, _P, _I64, _P, _P, _P],
    "iris_sample_brdf": [_P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P],
    "iris_pt_jitter": [_P, _P, _P, _P, _I64, _I32, _P, _P],
    "iris_pt_primary_emit": [_P, _P, _I64, _P, _P, _P],
    "iris_pt_nee": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _F, _F, _F, _P],
    "iris_pt_brdf_trace": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _I32, _F, _P],
    "iris_pt_brdf_finish": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _F, _F, _P],
    "iris_pt_primary": [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P, _P],
    "iris_render_primary": [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P],
    "iris_render_intrinsics": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P],
    "iris_pt_apply": [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P],
    "iris_pt_bounce": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P],
    "iris_pt_compact_workspace_bytes": [_I64],
    "iris_pt_compact": [_P, _I64, _I32, _P, _P, C.c_uint32, _I32, _P, _P, _I32, _P, _P, _P, _P, C.c_uint64, _P],
    "iris_relight_surface": [_P, _I64, _P, _I32, _P, _I64, _P, _P, _P, _P, _P],
    "iris_pt_nee_spot": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I64, _P, _P, _P],
    "iris_relight_shade": [_P, _P, _I64, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _F, _P],
    "iris_pt_accumulate_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P],
    "iris_pt_accumulate_bwd": [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P],
    "iris_pt_step_accumulate_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P, _P],
    "iris_pt_step_accumulate_bwd": [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P, _P],
    "iris_slf_scatter_add": [_P, _P, _P, _I64, _P, _P, _P],
    "iris_voxel_histogram": [_P, _I64, _D, _D, _I32, _P, _P],
    "iris_scatter_add_rows": [_P, _P, _I64, _I64, _P, _P, _P],
    "iris_pool_view": [_P, _P, _P],
    "iris_label_vote": [_P, _P, _P],
    "iris_label_argmax": [_P, _I64, _I32, _P, _P],
    "iris_label_view": [_P, _P, _P],
    "iris_cache_row_floats": [_I32],
    "iris_cache_pack": [_P, _P, _P, _I64, _I32, _P, _P],
    "iris_cache_gather": [_P, _P, _I64, _I32, _P, _P],
    "iris_shade_cached_fwd": [_P, _P, _P, _P, _P, _I64, _I32, _P, _P],
    "iris_shade_cached_bwd": [_P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P],
    "iris_prop_runs": [_P, _I64, _P, _P],
    "iris_prop_draws": [_P, _P, _I64, _I32, _U64, _P, _P],
    "iris_prop_semantic_fwd": [_P, _P, _P, _P, _P, _P, _I64, _I32, _P, _U64, _D, _D, _I32, _D, _D, _F, _P, _P, _P, _P, _P],
    "iris_prop_semantic_bwd": [_P, _P, _P, _P, _I64, _I32, _P, _U64, _D, _D, _F, _P, _P, _P, _P, _P],
    "iris_prop_part_fwd": [_P, _P, _P, _P, _I64, _F, _P, _P, _P, _P, _P],
    "iris_prop_part_bwd": [_P, _P, _P, _P, _P, _I64, _F, _P, _P, _P, _P],
    "iris_loss_albedo_fwd": [_P, _P, _P, _P, _I64, _I32, _F, _P, _P, _P, _P, _P],
    "iris_loss_albedo_bwd": [_P, _P, _P, _P, _P, _I64, _F, _P, _P, _P],
    "iris_loss_photometric_workspace_bytes": [_I64],
    "iris_loss_photometric": [_P, _I32, _P, _P, _I32, _P, _I64, _F, _P, _I64, _P, _P, _P, _P, _U64, _P],
    "iris_crf_fwd": [_P, _P, _I32, _P, _P, _I64, _F, _I64, _P, _P],
    "iris_crf_lookup_inv": [_P, _P, _I32, _P, _P, _I64, _F, _I64, _P, _P],
    "iris_crf_bwd_workspace_bytes": [_I64, _I32],
    "iris_crf_bwd": [_P, _P, _I32, _P, _P, _I64, _F, _I64, _P, _P, _P, _P, _U64, _P],
    "iris_crf_inv_table": [_P, _P, _I32, _P, _P],
    "iris_denoise_workspace_bytes": [_I32, _I32],
    "iris_denoise": [_P, _P, _P, _I32, _I32, _I32, _P, _P, _I32, _F, _F, _F, _P, _U64, _P],
    "iris_image_metrics_workspace_bytes": [_I32, _I32, _I32, _I32],
    "iris_image_metrics": [_P, _P, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _U64, _P],
    "iris_material_metrics_workspace_bytes": [_I32, _I32, _I32],
    "iris_material_metrics": [_P, _P],
    "iris_val_kd_loss_workspace_bytes": [_I32, _I32, _I32],
    "iris_val_kd_loss": [_P, _P],
    "iris_val_intrinsics": [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P],
    "iris_uv_raster_workspace_bytes": [_I64],
    "iris_uv_raster": [_P, _I64, _P, _I64, _I32, _I32, _P, _P, _U64, _P],
    "iris_debug_uv_raster": [_P, _I64, _P, _I64, _I32, _I32, _P, _P, _U64, _I32, _P],
    "iris_uv_resolve": [_P, _I64, _P, _P, _I64, _P, _I64, _I32, _I32, _P, _I64, _I64, _P, _P, _P],
    "iris_texture_quantize": [_P, _P, _P, _P, _I64, _I64, _I64, _P, _P, _P],
    "iris_atlas_measure": [_P, _I64, _P, _I64, _P, _P, _P],
    "iris_atlas_density": [_I32],
    "iris_atlas_classes": [_P, _I64, _I32, _I32, _P, _P, _P],
    "iris_atlas_place": [_P, _P, _P, _I64, _I32, _P, _P, _P],
    "iris_texture_dilate": [_P, _I32, _I32, _I32, _P, _P, _P],
    "iris_closest_point": [_P, _P, _I64, _P, _P, _P, _P, _P],
    "iris_texture_sample": [_P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _I32, _I32, _P, _P, _P, _P],
    "iris_texture_material": [_P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _I32, _I32, _P, _P, _P, _P],
    "iris_texture_sample_f32": [_P, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _I32, _P, _P, _P, _P],
    "iris_texture_sample_f32_bwd": [_P, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _I32, _P, _P, _P, _P, _P],
    "iris_exr_zip_workspace_bytes": [_I32, _I64, _I64, _I64],
    "iris_exr_zip_encode": [_P, _P, _I32, _I64, _I64, _I64, _I32, _P, _P, _P, _U64, _P],
    "iris_png_row_bytes": [_I32, _I32, _I32, _I32],
    "iris_png_rows": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P],
    "iris_png_stream_bound": [_I64],
    "iris_png_workspace_bytes": [_I32, _I64],
    "iris_png_encode": [_P, _I32, _I64, _P, _P, _P, _U64, _P],
    "iris_png_magma_table": [_P],
    "iris_jpeg_stream_bound": [_I32, _I32],
    "iris_jpeg_workspace_bytes": [_I32, _I32, _I32],
    "iris_jpeg_encode": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _U64, _P],
    "iris_jpeg_tables": [_P],
    "iris_resize_tables": [_I32, _I32, _I32, _P, _P],
    "iris_resize_u8": [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _I32, _P],
    "iris_bake_tile_max_spp": [],
    "iris_last_error": [],
    "iris_version": [],
}
_RESTYPE = {"iris_scene_destroy": None, "iris_slf_destroy": None, "iris_emitter_destroy": None,
            "iris_last_error": C.c_char_p, "iris_version": C.c_char_p, "iris_debug_build_flags": C.c_char_p, "iris_debug_source_hash": C.c_char_p, "iris_ngp_n_params": C.c_int64, "iris_ngp_destroy": None, "iris_bake_workspace_bytes": C.c_uint64, "iris_pt_compact_workspace_bytes": C.c_uint64, "iris_denoise_workspace_bytes": C.c_uint64,
            "iris_exr_zip_workspace_bytes": C.c_uint64, "iris_ngp_backward_workspace_bytes": C.c_uint64, "iris_crf_bwd_workspace_bytes": C.c_uint64,
            "iris_loss_photometric_workspace_bytes": C.c_uint64,
            "iris_png_row_bytes": C.c_int64, "iris_png_stream_bound": C.c_uint64, "iris_png_workspace_bytes": C.c_uint64, "iris_png_magma_table": None,
            "iris_jpeg_stream_bound": C.c_uint64, "iris_jpeg_workspace_bytes": C.c_uint64, "iris_jpeg_tables": None,
            "iris_image_metrics_workspace_bytes": C.c_uint64, "iris_material_metrics_workspace_bytes": C.c_uint64, "iris_val_kd_loss_workspace_bytes": C.c_uint64, "iris_uv_raster_workspace_bytes": C.c_uint64, "iris_atlas_density": C.c_double}

_lib = None


def lib():
    """The loaded library.  Raises (never falls back) when libiris_hip.so has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IrisError(f"{LIB_PATH} is missing: build it with `make -C iris_amd/csrc` or "
                            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, argtypes in PROTOTYPES.items():
            fn = getattr(l, name)  # AttributeError if the symbol is not exported
            fn.argtypes = argtypes
            fn.restype = _RESTYPE.get(name, C.c_int)
        _lib = l
    return _lib


def source_hash():
    """sha256 over the sources the BAKE kernels are compiled from (device / traversal / tile / bake headers, the host file that sizes and launches them, the BVH
    builder, the ABI headers) and the compiler flags embedded in the LOADED library (iris_debug_build_flags: -fno-slp-vectorize, the scheduler strategy and the
    -D tuning overrides are worth several per cent): stamps counter profiles (tools/pmc_summary.py) so that bench.py can refuse counters that were taken on other
    kernels or on another build of the same sources.  (The headers of the other stages -- material network, shading cache, denoiser, path-tracing stages -- are
    not part of the stamp: bake_view_kernel does not include them.)"""
    import hashlib
    h = hashlib.sha256()
    h.update(lib().iris_debug_build_flags())
    root = os.path.dirname(_HERE)
    files = [os.path.join("iris_amd", "csrc", f) for f in ("bvh_build.cpp", "bvh_build.h", "iris_bake.h", "iris_device.h", "iris_hip.hip", "iris_tile.h", "iris_trace.h")]
    files += [os.path.join("include", "iris_hip.h"), os.path.join("include", "iris_hip_debug.h")]
    for f in files:
        h.update(f.encode()); h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def device_index(device):
    """The HIP device ordinal a torch device names: `torch.device('cuda')` (no index) is torch's CURRENT device on this rank, not device 0 -- one process per
    GPU sets it once (torch.cuda.set_device(LOCAL_RANK)) and then passes index-less devices around."""
    device = torch.device(device)
    if device.type != "cuda":
        raise IrisError(f"{device}: the HIP path needs a GPU device (there is no CPU fallback)")
    return device.index if device.index is not None else torch.cuda.current_device()


class Native:
    """The ONE owner of a native object (iris_scene / iris_slf / iris_emitter / iris_ngp): its pointer, the entry point that destroys it and the device
    ordinal (device_index) it was created for, with the tensor_keys of the tensors it was filled from (`keys`, a list: they describe this object and leave with
    it).  The pointer is destroyed exactly once, by free() or when the owner is collected.  copy.copy, copy.deepcopy and pickle never duplicate it: the copy
    is an EMPTY owner (ptr None, no keys), so a deep copy or unpickle of a module builds its own native object on first use.  (A SHALLOW copy of a module
    shares the module's tensors and, with them, this one owner: nothing is destroyed before both are gone.)"""

    def __init__(self, ptr=None, destroy=None, device=None, keys=()):
        self.ptr, self.destroy, self.device, self.keys = ptr, destroy, device, list(keys)

    def free(self):
        d = self.__dict__               # (plain dict access: at interpreter shutdown little else can be relied on)
        p, d["ptr"] = d.get("ptr"), None
        if p:
            d["destroy"](p)

    def __del__(self):
        try:
            self.free()
        except Exception:     # noqa  (interpreter shutdown: the library, or the helpers the call needs, may be gone already)
            pass

    def __reduce__(self):
        return (Native, ())


class tensor_key:
    """What a device-side copy of tensor `t` was made from: the tensor OBJECT, its _version, its data_ptr() and its device.  A change in any of the four means the
    copy is stale: an in-place write bumps _version; a rebound buffer (`vslf.radiance = vslf.radiance / n`) is a new object even when the caching allocator hands it
    the address -- and _version 0 -- of the tensor that was uploaded before; `p.data = other` and Module.to() keep the object and its _version and change only
    data_ptr().  The tensor object itself is kept (not only its data_ptr): holding the reference keeps that address from being reused while the key is alive.
    tensor_key() matches nothing, and that is what a copy or unpickle of a key is: the key is dropped with the native object it describes."""
    __slots__ = ("t", "version", "ptr", "device")

    def __init__(self, t=None):
        self.t = t
        if t is not None:
            self.version, self.ptr, self.device = t._version, t.data_ptr(), t.device

    def fresh(self, t):
        return self.t is t and self.version == t._version and self.ptr == t.data_ptr() and self.device == t.device

    def __reduce__(self):
        return (tensor_key, ())


def build_id():
    """What identifies the ARITHMETIC of the LOADED library for a resumable run: its version string, the compiler flags and the hash of ALL the sources it was
    compiled from -- path-tracing stages, material network, shading cache and denoiser included --, both embedded in the binary by the Makefile (a sampler,
    traversal, network or filter change alters bits: maps of two builds must not be mixed by --resume).  Nothing is read from csrc/ on disk: a stale library
    keeps its own id, an installation without sources works.  A library built around the Makefile carries no hash and is refused."""
    h = lib().iris_debug_source_hash().decode()
    if h == "unknown" or len(h) != 16:
        raise IrisError("libiris_hip.so carries no source hash (built without iris_amd/csrc/Makefile): a resumable run cannot be keyed on it")
    return lib().iris_version().decode() + "|" + lib().iris_debug_build_flags().decode() + "|" + h


class StageTimer:
    """Diagnostics (bench.py extras, tools/bench_pt_single.py): HIP events around the stages of a multi-kernel call.  `with L.StageTimer() as t:` makes every
    `L.mark(name)` inside record an event on the stream that is current THERE; `t.ms()` -> {stage: milliseconds between its mark and the previous mark on the
    same stream} (stages on different streams overlap: the figures do not add up to the wall time).  Not active (no events, no cost) otherwise."""
    active = None

    def __enter__(self):
        self.events = []          # (stream id, name, event)
        StageTimer.active = self
        return self

    def __exit__(self, *a):
        StageTimer.active = None

    def ms(self):
        import torch
        torch.cuda.synchronize()
        out, last = {}, {}
        for sid, name, ev in self.events:
            if sid in last and name is not None:
                out[name] = out.get(name, 0.0) + last[sid].elapsed_time(ev)
            last[sid] = ev
        return out


def mark(name=None):
    """StageTimer: end of stage `name` (None: start of a sequence) on the current stream"""
    t = StageTimer.active
    if t is not None:
        import torch
        ev = torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream()
        ev.record(st)
        t.events.append((st.cuda_stream, name, ev))


def debug_set(key, value):
    """iris_debug_set (include/iris_hip_debug.h): process-wide tuning option; value < 0 restores the default."""
    check(lib().iris_debug_set(key.encode(), int(value)))


def check(rc):
    if rc != 0:
        raise IrisError(lib().iris_last_error().decode("utf-8", "replace"))


def require_gpu(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise IrisError(f"{name}: expected a tensor on a HIP device (got {getattr(t, 'device', type(t))}); "
                        "iris_amd has no CPU path")
    if t.dtype != dtype:
        raise IrisError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def no_autograd(fn, *tensors):
    """The entry points behind `fn` are raw HIP kernels writing into fresh buffers: they have no backward pass.  The reference's counterparts
    are differentiable torch ops, so handing them a tensor that requires grad (with grad mode on) would silently train with zero / None
    gradients -- raise instead.  Call under torch.no_grad() or pass .detach()ed tensors to state that no gradient is wanted."""
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise IrisError(f"{fn}: an input requires grad, but this is a HIP kernel without a backward pass (the reference's torch op is differentiable); "
                        "wrap the call in torch.no_grad() or detach() the inputs")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host_f32(a):
    import numpy as np
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)
