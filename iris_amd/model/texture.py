"""The exported textures as a material (iris_amd/csrc/iris_texmat.h; the contract: DESIGN.md section 5c-17): what `python -m iris_amd.utils.export` writes
-- albedo.png, rm.png, ft.npy, vt.npy -- read back and evaluated at positions, so that every integrator and render_intrinsics takes the exported asset where
they take NGPBRDF.

The reference's TextureBRDF (model/brdf.py:262) is an unused, trainable uv -> sigmoid(texture) stub; BakedTextureBRDF is not that class: it reads the export's
8-bit files, takes POSITIONS (closest triangle of the mesh -> its UVs -> a bilinear fetch) and has no parameters.  TextureBRDF is the
trainable one: the same fetch over float32 texels, with a backward pass to the texels, which `utils.export --fit_steps` fits to the network.

Not built: mip levels or any filtering by the ray's footprint (every lookup is one bilinear fetch of the full-resolution image), sRGB textures (the export
writes linear values and they are read as linear values), gradients of BakedTextureBRDF and sample_textures (forward only; TextureBRDF has the gradient to its
texels), gradients to UVs, barycentrics or positions, a bitwise-reproducible backward."""
import os

import numpy as np
import torch

from .. import _lib as L
from ..utils.texture import MAX_TEX_RES
from .brdf import BaseBRDF


def _shape_dtype(a):
    if torch.is_tensor(a):
        return tuple(a.shape), ("u1" if a.dtype == torch.uint8 else str(a.dtype))
    a = np.asarray(a)
    return a.shape, ("u1" if a.dtype == np.uint8 else str(a.dtype))


def check_texture_inputs(ft, vt, albedo_img, rm_img, n_faces=None):
    """The host checks of the texture material, before a device is touched -> (H, W).  IrisError on: an image that is not (H, W, 3) uint8, two images of
    different sizes, a side above MAX_TEX_RES; ft not (F, 3) integers, vt not (N, 2) floating point; ft.shape[0] != n_faces (when given: one UV triangle per
    face of the mesh); an index of ft outside vt; a vt that is not finite."""
    from ..utils.texture import _summary
    (s_a, d_a), (s_r, d_r) = _shape_dtype(albedo_img), _shape_dtype(rm_img)
    for name, s, d in (("albedo", s_a, d_a), ("rm", s_r, d_r)):
        if len(s) != 3 or s[2] != 3 or d != "u1" or s[0] < 1 or s[1] < 1:
            raise L.IrisError(f"texture material: the {name} image must be 8-bit RGB, (H, W, 3) uint8 (got {tuple(s)} {d})")
    if s_a != s_r:
        raise L.IrisError(f"texture material: albedo {tuple(s_a[:2])} and rm {tuple(s_r[:2])} differ in size")
    H, W = int(s_a[0]), int(s_a[1])
    if H > MAX_TEX_RES or W > MAX_TEX_RES:
        raise L.IrisError(f"texture material: a {H} x {W} texture: every side must be at most {MAX_TEX_RES}")
    (s_ft, k_ft, _, ft_lo, ft_hi), (s_vt, k_vt, finite, _, _) = _summary(ft), _summary(vt)
    if len(s_ft) != 2 or s_ft[1] != 3 or k_ft != "i":
        raise L.IrisError(f"texture material: ft {tuple(s_ft)} must be an (F, 3) integer array")
    if len(s_vt) != 2 or s_vt[1] != 2 or k_vt != "f":
        raise L.IrisError(f"texture material: vt {tuple(s_vt)} must be an (N, 2) floating-point array")
    if n_faces is not None and s_ft[0] != int(n_faces):
        raise L.IrisError(f"texture material: ft names {s_ft[0]} UV triangles, the mesh has {int(n_faces)} faces (one per face, in the faces' order)")
    if s_ft[0] and (ft_lo < 0 or ft_hi >= s_vt[0]):
        raise L.IrisError(f"texture material: ft indexes [{ft_lo}, {ft_hi}] outside the {s_vt[0]} UV vertices")
    if not finite:
        raise L.IrisError("texture material: vt holds a non-finite UV")
    return H, W


def _to_dev(a, dtype, dev):
    t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


class _Textures:
    """the checked, uploaded tables of one export: ft (F, 3) int32, vt (N, 2) float32, the two (H, W, 3) uint8 images"""

    def __init__(self, ft, vt, albedo_img, rm_img, device, n_faces=None):
        L.no_autograd("texture material", vt)
        self.H, self.W = check_texture_inputs(ft, vt, albedo_img, rm_img, n_faces)
        self.device = torch.device("cuda", L.device_index(device))
        self.ft, self.vt = _to_dev(ft, torch.int32, self.device), _to_dev(vt, torch.float32, self.device)
        self.albedo, self.rm = _to_dev(albedo_img, torch.uint8, self.device), _to_dev(rm_img, torch.uint8, self.device)

    def args(self):
        return (L.ptr(self.ft), self.ft.shape[0], L.ptr(self.vt), self.vt.shape[0], L.ptr(self.albedo), L.ptr(self.rm), self.H, self.W)


def _outputs(B, dev):
    return torch.empty(B, 3, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.float32)


def _sample(tex, tri, bary):
    L.no_autograd("sample_textures", bary)
    tri = L.require_gpu(tri, torch.int64, "tri").reshape(-1)
    bary = L.require_gpu(bary, torch.float32, "bary").detach().reshape(-1, 2)
    B = tri.shape[0]
    if bary.shape[0] != B:
        raise L.IrisError(f"sample_textures: {B} triangles and {bary.shape[0]} barycentric pairs")
    if tri.device != tex.device or bary.device != tex.device:
        raise L.IrisError(f"sample_textures: tri on {tri.device}, bary on {bary.device}, the textures on {tex.device}")
    albedo, rough, metal = _outputs(B, tex.device)
    with torch.cuda.device(tex.device):
        L.check(L.lib().iris_texture_sample(L.ptr(tri), L.ptr(bary), B, *tex.args(), L.ptr(albedo), L.ptr(rough), L.ptr(metal), L.stream()))
    return {"albedo": albedo, "roughness": rough.reshape(B, 1), "metallic": metal.reshape(B, 1)}


def sample_textures(tri, bary, ft, vt, albedo_img, rm_img):
    """The fetch alone, for a caller that already holds a hit's triangle and barycentrics (ray_intersect's idx and uvs, closest_point's tri and bary):
    tri (B,) int64, bary (B, 2) float32 on the GPU; ft (F, 3), vt (N, 2) and the two (H, W, 3) uint8 images as the export wrote them, host arrays or tensors
    -> {'albedo' (B, 3), 'roughness' (B, 1), 'metallic' (B, 1)} float32.
    uv = (1 - b1 - b2) vt[ft[t, 0]] + b1 vt[ft[t, 1]] + b2 vt[ft[t, 2]]; a bilinear fetch in the rasteriser's texel convention (texel (r, c)
    has its centre at u = (c + .5) / W, v = (r + .5) / H), clamped at the borders, bytes as byte / 255, lerp form.  Albedo is read as linear values; roughness
    is channel 0 of rm with the network's floor of 0.02 put back, metallic channel 1.  tri = -1 gives zeros and roughness 0.02.  Uncovered texels are read as
    they are: export with --dilate >= 1, or the taps at a chart's border read black.  Forward only: an input that requires grad raises."""
    dev = tri.device if torch.is_tensor(tri) else None
    if dev is None or dev.type != "cuda":
        raise L.IrisError("sample_textures: tri must be an int64 tensor on a HIP device; iris_amd has no CPU path")
    return _sample(_Textures(ft, vt, albedo_img, rm_img, dev), tri, bary)


class BakedTextureBRDF(BaseBRDF):
    """The exported textures as material_net(position): forward is ONE launch -- the closest triangle of the mesh (utils.closest.closest_point's query), its
    UVs from ft / vt, the bilinear fetch of sample_textures -- and equals sample_textures(*closest_point(scene, x)[:2], ...) bit for bit.  The return
    contract is NGPBRDF.forward's, so path_tracing, path_tracing_single, render_intrinsics and the relighting integrator take it unchanged.

    scene: the Scene of the mesh the atlas belongs to (one UV triangle per face, in the faces' order).  It is the material's own: render_relight traces a scene
    that also holds the inserted lights, and the material keeps looking positions up in the room.  No parameters, forward only."""

    def __init__(self, scene, ft, vt, albedo_img, rm_img):
        super().__init__()
        self.scene = scene
        self.tex = _Textures(ft, vt, albedo_img, rm_img, scene.device, n_faces=scene.n_triangles)

    @classmethod
    def from_export(cls, dir, vertices, faces, device=None):
        """The folder `python -m iris_amd.utils.export --dir_save dir` wrote: ft.npy, vt.npy, albedo.png and rm.png (read with PIL), and the mesh
        (vertices (V, 3), faces (F, 3)) the atlas was made for, of which it builds its own Scene on `device`.  Everything that can be refused is refused
        before the device is touched."""
        from PIL import Image
        from ..utils.path_tracing import Scene
        paths = {n: os.path.join(str(dir), n) for n in ("ft.npy", "vt.npy", "albedo.png", "rm.png")}
        missing = [p for p in paths.values() if not os.path.isfile(p)]
        if missing:
            raise L.IrisError(f"texture material: {missing[0]} not found (the folder must hold ft.npy, vt.npy, albedo.png and rm.png, as utils.export writes them)")
        ft, vt = np.load(paths["ft.npy"]), np.load(paths["vt.npy"])
        images = {}
        for n in ("albedo.png", "rm.png"):
            with Image.open(paths[n]) as im:
                if im.mode != "RGB":
                    raise L.IrisError(f"texture material: {paths[n]} must be 8-bit RGB (its mode is {im.mode})")
                if max(im.size) > MAX_TEX_RES:
                    raise L.IrisError(f"texture material: {paths[n]} is {im.size[1]} x {im.size[0]}: every side must be at most {MAX_TEX_RES}")
                images[n] = np.array(im)
        faces = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        check_texture_inputs(ft, vt, images["albedo.png"], images["rm.png"], n_faces=faces.reshape(-1, 3).shape[0])
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return cls(Scene(vertices, faces, device=device), ft, vt, images["albedo.png"], images["rm.png"])

    def forward(self, position):
        """position (..., 3) float32 on the GPU -> {'albedo': (..., 3), 'roughness': (..., 1) in [0.02, 1], 'metallic': (..., 1)}"""
        L.no_autograd("BakedTextureBRDF.forward", position)
        position = L.require_gpu(position, torch.float32, "position")
        tex = self.tex
        if L.device_index(position.device) != tex.device.index:
            raise L.IrisError(f"BakedTextureBRDF.forward: position is on {position.device}, the textures on {tex.device}")
        shape = position.shape[:-1]
        pos = position.detach().reshape(-1, 3)
        B = pos.shape[0]
        albedo, rough, metal = _outputs(B, tex.device)
        with torch.cuda.device(tex.device):
            L.check(L.lib().iris_texture_material(self.scene.handle, L.ptr(pos), B, *tex.args(), L.ptr(albedo), L.ptr(rough), L.ptr(metal), L.stream()))
        return {"albedo": albedo.reshape(*shape, 3), "roughness": rough.reshape(*shape, 1), "metallic": metal.reshape(*shape, 1)}

    def sample(self, tri, bary):
        """sample_textures on this material's tables (nothing is uploaded again)"""
        return _sample(self.tex, tri, bary)


class _TexelSample(torch.autograd.Function):
    """texels (H, W, 5) -> (albedo, roughness, metallic) at fixed (tri, bary): iris_texture_sample_f32 and its backward, which recomputes the taps and the
    roughness gate from the texels and adds into a zeroed gradient with float atomics (reproducible to rounding, not bit for bit)."""

    @staticmethod
    def forward(ctx, texels, owner, tri, bary):
        ctx.owner, ctx.tri, ctx.bary = owner, tri, bary
        ctx.save_for_backward(texels)
        B = tri.shape[0]
        out = _outputs(B, texels.device)
        with torch.cuda.device(texels.device):
            L.check(L.lib().iris_texture_sample_f32(L.ptr(tri), L.ptr(bary), B, *owner._args(texels), *(L.ptr(o) for o in out), L.stream()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_albedo, g_rough, g_metal):
        (texels,) = ctx.saved_tensors
        B, dev = ctx.tri.shape[0], texels.device
        grad = torch.zeros_like(texels)
        if B > 0:
            def cot(g, shape):
                return torch.zeros(shape, device=dev) if g is None else g.to(torch.float32).contiguous()
            g_albedo, g_rough, g_metal = cot(g_albedo, (B, 3)), cot(g_rough, (B,)), cot(g_metal, (B,))
            with torch.cuda.device(dev):
                L.check(L.lib().iris_texture_sample_f32_bwd(L.ptr(ctx.tri), L.ptr(ctx.bary), B, *ctx.owner._args(texels), L.ptr(g_albedo), L.ptr(g_rough),
                                                            L.ptr(g_metal), L.ptr(grad), L.stream()))
        return grad, None, None, None


class TextureBRDF(BaseBRDF):
    """The exported textures as a TRAINABLE material: one parameter `texels`, (H, W, 5) float32 on the device -- albedo r, g, b,
    roughness, metallic per texel -- read by BakedTextureBRDF's fetch with the taps taken as they are (iris_texture_sample_f32), and differentiable with respect
    to the texels (iris_texture_sample_f32_bwd).  It starts from the export's 8-bit images, texels = byte / 255 (a float32 division: sample() then equals
    BakedTextureBRDF.sample() bit for bit), is fitted to the network by utils.texture.fit_textures, and goes back to 8 bits with to_images().
    (The reference's unused TextureBRDF, model/brdf.py:262, is uv -> sigmoid(texture); this one takes positions or (tri, bary) and stores the values themselves.)

    scene, ft, vt, the images: as BakedTextureBRDF.  position, bary and vt get no gradient, and a position or bary that requires grad raises.  FusedAdam steps
    `texels` as any contiguous float32 device tensor.  The gradient is summed with float atomics: reproducible to rounding, not bit for bit."""

    def __init__(self, scene, ft, vt, albedo_img, rm_img):
        super().__init__()
        self.scene = scene
        tex = _Textures(ft, vt, albedo_img, rm_img, scene.device, n_faces=scene.n_triangles)
        self.H, self.W, self.ft, self.vt = tex.H, tex.W, tex.ft, tex.vt
        bytes5 = torch.cat([tex.albedo, tex.rm[..., :2]], dim=-1).to(torch.float32)
        # (a tensor divisor: torch turns a division by a Python scalar into a multiplication by its reciprocal, which is not the fetch's byte / 255)
        self.texels = torch.nn.Parameter((bytes5 / torch.tensor(255.0, device=tex.device)).contiguous())

    from_export = classmethod(BakedTextureBRDF.from_export.__func__)

    def _args(self, texels):
        return (L.ptr(self.ft), self.ft.shape[0], L.ptr(self.vt), self.vt.shape[0], L.ptr(texels), self.H, self.W)

    def sample(self, tri, bary):
        """tri (B,) int64, bary (B, 2) float32 on the device -> {'albedo' (B, 3), 'roughness' (B, 1), 'metallic' (B, 1)}, differentiable w.r.t. texels"""
        L.no_autograd("TextureBRDF.sample", bary)
        texels = self.texels
        if not texels.is_cuda or texels.dtype != torch.float32 or not texels.is_contiguous() or tuple(texels.shape) != (self.H, self.W, 5):
            raise L.IrisError(f"TextureBRDF: texels must stay a contiguous ({self.H}, {self.W}, 5) float32 tensor on the device "
                              f"(it is {tuple(texels.shape)} {texels.dtype} on {texels.device})")
        tri = L.require_gpu(tri, torch.int64, "tri").reshape(-1)
        bary = L.require_gpu(bary, torch.float32, "bary").detach().reshape(-1, 2)
        B = tri.shape[0]
        if bary.shape[0] != B:
            raise L.IrisError(f"TextureBRDF.sample: {B} triangles and {bary.shape[0]} barycentric pairs")
        if tri.device != texels.device or bary.device != texels.device:
            raise L.IrisError(f"TextureBRDF.sample: tri on {tri.device}, bary on {bary.device}, the texels on {texels.device}")
        albedo, rough, metal = _TexelSample.apply(texels, self, tri, bary)
        return {"albedo": albedo, "roughness": rough.reshape(B, 1), "metallic": metal.reshape(B, 1)}

    def forward(self, position):
        """position (..., 3) float32 on the GPU -> NGPBRDF.forward's dict: closest_point, then sample at its (tri, bary) (two launches: the query dominates)"""
        from ..utils.closest import closest_point
        L.no_autograd("TextureBRDF.forward", position)
        position = L.require_gpu(position, torch.float32, "position")
        shape = position.shape[:-1]
        tri, bary, _, _ = closest_point(self.scene, position.detach().reshape(-1, 3))
        out = self.sample(tri, bary)
        return {"albedo": out["albedo"].reshape(*shape, 3), "roughness": out["roughness"].reshape(*shape, 1), "metallic": out["metallic"].reshape(*shape, 1)}

    @torch.no_grad()
    def to_images(self):
        """-> (albedo_img, rm_img), (H, W, 3) uint8 on the device: floor(clamp(x, 0, 1) * 255 + 0.5) in float32, a NaN as 0; rm = (roughness, metallic, 0).
        Rounds to nearest where the bake truncates: a fitted value has no reason to be truncated."""
        return quantize_texels(self.texels)


def quantize_texels(texels):
    """to_images' rule on an (H, W, 5) float32 tensor, wherever it lives -> (albedo (H, W, 3), rm (H, W, 3)) uint8"""
    t = texels.detach().to(torch.float32)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t).clamp(0.0, 1.0)
    q = torch.floor(t * 255.0 + 0.5).to(torch.uint8)
    return q[..., :3].contiguous(), torch.cat([q[..., 3:5], torch.zeros_like(q[..., :1])], dim=-1).contiguous()
