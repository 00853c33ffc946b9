"""The intrinsics half of the render stage (reference: render.py:178-220): kd, a_prime, roughness, metallic, emission and the surface light field of a view,
averaged over spp jittered primary rays per pixel.

Three steps per chunk of pixels: `iris_render_primary` (jitter with render.py's un-centred offsets, closest hit, emitter ordinal), the material network at the
hits, `iris_render_intrinsics` (everything after the network as one launch, += into the caller's maps).  The reference's ~100 ATen launches over (B*spp, k)
intermediates for a whole view at once become two kernels and the network over at most CHUNK_SAMPLES samples at a time.
"""
import torch

from .. import _lib as L
from .path_tracing import _mat_tensors

MAPS = (("kd", 3), ("a_prime", 3), ("roughness", 1), ("metallic", 1), ("emission", 3), ("slf", 3))
CHUNK_SAMPLES = 1 << 22        # samples alive at once: SAMPLE_BYTES each = 373 MB per chunk, the material network's own buffers on top
SAMPLE_BYTES = 4 * (3 * 5 + 3 + 2 + 2) + 1     # = 89: wi, wo, pos, nrm, albedo (N,3); roughness, metallic, e0 (N); u2 (N,2); dudv (2,N); valid_next (N) u8


def new_maps(B, device):
    """the six zeroed maps render_intrinsics accumulates into: (B,3) or (B,1) float32, as render.py:165-170 allocates them"""
    return {k: torch.zeros(B, c, device=device, dtype=torch.float32) for k, c in MAPS}


@torch.no_grad()
def render_intrinsics(scene, emitter_net, material_net, rays_o, rays_d, dx_du, dy_dv, spp, out=None, uniforms=None, chunk=None, debug=None):
    """One round of render.py:178-220: `map += mean over spp jittered samples` for the six intrinsic maps.

    rays_o, rays_d, dx_du, dy_dv: (B,3) float32 on the GPU.  out: a dict from `new_maps` (or an earlier call) to accumulate into; None = fresh zeroed maps.
    uniforms: optional [rand(2,B,spp,1), rand(B*spp,2)], the two draws of render.py:179 and :197 (parity mode); otherwise the function draws with torch.rand, one
    generator call per chunk.  chunk: pixels per pass (default: CHUNK_SAMPLES // spp); per-pixel sums are independent, so chunking changes no bit when the draws
    are given.  debug: optional dict that receives the per-sample e0 / valid_next of the call (tests).
    Per pixel: map[b] += (x_0 + ... + x_{spp-1}) * (1.0f / spp), samples added in order in float32 (include/iris_hip.h).  Runs without gradient.
    Returns the dict of maps."""
    spp = int(spp)
    if spp < 1:
        raise L.IrisError(f"render_intrinsics: spp ({spp}) must be at least 1")
    rays_o = L.require_gpu(rays_o, torch.float32, "rays_o").reshape(-1, 3)
    rays_d = L.require_gpu(rays_d, torch.float32, "rays_d").reshape(-1, 3)
    dx_du = L.require_gpu(dx_du, torch.float32, "dx_du").reshape(-1, 3)
    dy_dv = L.require_gpu(dy_dv, torch.float32, "dy_dv").reshape(-1, 3)
    B, dev = rays_o.shape[0], rays_o.device
    if out is None:
        out = new_maps(B, dev)
    maps = {}
    for k, c in MAPS:
        m = L.require_gpu(out[k], torch.float32, f"out[{k!r}]")
        if m.numel() != B * c or m.data_ptr() != out[k].data_ptr():
            raise L.IrisError(f"render_intrinsics: out[{k!r}] must be a contiguous float32 tensor of {B * c} values (got shape {tuple(out[k].shape)})")
        maps[k] = m
    if uniforms is not None:
        if len(uniforms) != 2:
            raise L.IrisError(f"render_intrinsics: uniforms has {len(uniforms)} tensors, a round draws two (rand(2,B,spp,1), rand(B*spp,2))")
        dudv_all = L.require_gpu(uniforms[0], torch.float32, "uniforms[0]")
        u2_all = L.require_gpu(uniforms[1], torch.float32, "uniforms[1]")
        if dudv_all.numel() != 2 * B * spp or u2_all.numel() != 2 * B * spp:
            raise L.IrisError(f"render_intrinsics: uniforms have shapes {tuple(dudv_all.shape)}, {tuple(u2_all.shape)}, expected (2,{B},{spp},1) and ({B * spp},2)")
        dudv_all, u2_all = dudv_all.reshape(2, B, spp), u2_all.reshape(B, spp, 2)
    step = max(1, CHUNK_SAMPLES // spp) if chunk is None else int(chunk)
    if step < 1:
        raise L.IrisError(f"render_intrinsics: chunk ({chunk}) must be at least 1 pixel")
    if debug is not None:
        debug["e0"] = torch.empty(B * spp, device=dev, dtype=torch.int32)
        debug["valid_next"] = torch.empty(B * spp, device=dev, dtype=torch.bool)
    lib = L.lib()
    with torch.cuda.device(dev):
        eh, sh = emitter_net.handle(dev), emitter_net.slf.handle(dev)
        radiance = emitter_net.radiance_on(dev)
        for b0 in range(0, B, step):
            b1 = min(b0 + step, B)
            Bc = b1 - b0
            N = Bc * spp
            L.mark()
            if uniforms is not None:
                dudv = dudv_all[:, b0:b1].contiguous()
                u2 = u2_all[b0:b1].reshape(N, 2).contiguous()
            else:
                pool = torch.rand(4 * N, device=dev)
                dudv, u2 = pool[:2 * N].reshape(2, Bc, spp), pool[2 * N:].reshape(N, 2)
            wi = torch.empty(N, 3, device=dev); wo = torch.empty(N, 3, device=dev); pos = torch.empty(N, 3, device=dev); nrm = torch.empty(N, 3, device=dev)
            e0 = torch.empty(N, device=dev, dtype=torch.int32); valid_next = torch.empty(N, device=dev, dtype=torch.bool)
            # (contiguous row slices of contiguous (B,3) tensors: the pointers of rows b0.. are passed as they are)
            ro, rd, dxu, dyv = rays_o[b0:b1], rays_d[b0:b1], dx_du[b0:b1], dy_dv[b0:b1]
            L.check(lib.iris_render_primary(scene.handle, eh, L.ptr(ro), L.ptr(rd), L.ptr(dxu), L.ptr(dyv), L.ptr(dudv), Bc, spp, L.ptr(wi), L.ptr(wo), L.ptr(pos),
                                            L.ptr(nrm), L.ptr(e0), L.ptr(valid_next), L.stream()))
            L.mark("jitter + primary hit")
            albedo, rough, metal = _mat_tensors(material_net(pos))
            if albedo.shape[0] != N or rough.shape[0] != N or metal.shape[0] != N:
                raise L.IrisError(f"render_intrinsics: material_net returned {albedo.shape[0]} / {rough.shape[0]} / {metal.shape[0]} rows for {N} positions")
            L.mark("material network")
            o = {k: maps[k].reshape(B, c)[b0:b1] for k, c in MAPS}
            L.check(lib.iris_render_intrinsics(eh, sh, L.ptr(radiance), L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(e0), L.ptr(valid_next), L.ptr(albedo), L.ptr(rough),
                                               L.ptr(metal), L.ptr(u2), Bc, spp, L.ptr(o["kd"]), L.ptr(o["a_prime"]), L.ptr(o["roughness"]), L.ptr(o["metallic"]),
                                               L.ptr(o["emission"]), L.ptr(o["slf"]), L.stream()))
            L.mark("intrinsics kernel")
            if debug is not None:
                debug["e0"][b0 * spp:b1 * spp] = e0
                debug["valid_next"][b0 * spp:b1 * spp] = valid_next
    return out
