"""Texture export on the device (reference: utils/export.py): UV rasteriser, material bake into albedo / roughness-metallic images, and the small host
pieces the stage needs (an atlas stand-in, a PNG writer, a textured OBJ writer).

The reference unwraps with xatlas and rasterises with nvdiffrast; both are third-party CUDA / GL packages without a ROCm build and neither is a dependency
here.  The rasteriser is this project's own HIP (iris_amd/csrc/iris_texture.h) with an exact contract: texel (r, c) of an H x W
texture has its centre at u = (c + .5) / W, v = (r + .5) / H, row 0 at v ~ 0; UVs snapped to 1 / 256 texel; int64 edge functions with a top-left rule; the
lowest face index wins an overlap; barycentrics from a float64 division, positions interpolated in float32 in one stated order.  tests/uv_raster_ref.py is
the same contract in numpy, and the kernels equal it bit for bit.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import torch

from .. import _lib as L

MAX_TEX_RES = 8192
RASTER_AUTO, RASTER_ALL_SMALL, RASTER_ALL_LARGE = 0, 1, 2        # include/iris_hip_debug.h IRIS_UV_RASTER_*


def _hw(tex_res):
    if isinstance(tex_res, (tuple, list)):
        if len(tex_res) != 2:
            raise L.IrisError(f"tex_res = {tex_res!r}: an integer or (H, W)")
        H, W = tex_res
    else:
        H = W = tex_res
    for n in (H, W):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_TEX_RES:
            raise L.IrisError(f"tex_res = {tex_res!r}: every side must be an integer in [1, {MAX_TEX_RES}]")
    return int(H), int(W)


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _summary(a):
    """(shape, kind 'f' / 'i' / other, all finite, min, max) of a host array or of a tensor WHERE IT LIVES: a device tensor is reduced on its device and three
    scalars are read back, the array itself is not copied"""
    if torch.is_tensor(a):
        a = a.detach()
        kind = "f" if a.is_floating_point() else "i" if a.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) else "?"
        if a.numel() == 0 or kind == "?":
            return tuple(a.shape), kind, True, 0, 0
        lo, hi = torch.aminmax(a)
        finite = bool(torch.isfinite(a).all()) if kind == "f" else True
        return tuple(a.shape), kind, finite, lo.item(), hi.item()
    a = np.asarray(a)
    kind = "f" if a.dtype.kind == "f" else "i" if a.dtype.kind in "iu" else "?"
    if a.size == 0 or kind == "?":
        return a.shape, kind, True, 0, 0
    return a.shape, kind, bool(np.isfinite(a).all()) if kind == "f" else True, a.min(), a.max()


def check_inputs(vt, ft, v, f, tex_res):
    """The host checks of the contract, before anything is uploaded -> (H, W).  Raises IrisError on: a tex_res outside [1, 8192]; vt not (N, 2), v not (V, 3),
    ft / f not (F, 3) integers or of different shapes; UVs that are not finite or lie outside [-1, 2]; an index of ft outside vt or of f outside v.
    Under these limits every edge value of the rasteriser stays far below 2^53.  (An input that already is a device tensor is reduced there.)"""
    H, W = _hw(tex_res)
    (s_vt, k_vt, finite, vt_lo, vt_hi), (s_ft, k_ft, _, ft_lo, ft_hi) = _summary(vt), _summary(ft)
    (s_v, k_v, _, _, _), (s_f, k_f, _, f_lo, f_hi) = _summary(v), _summary(f)
    if len(s_vt) != 2 or s_vt[1] != 2 or len(s_v) != 2 or s_v[1] != 3:
        raise L.IrisError(f"rasterize_uv: vt {s_vt} must be (N, 2) and v {s_v} must be (V, 3)")
    if s_ft != s_f:
        raise L.IrisError(f"rasterize_uv: ft {s_ft} and f {s_f} differ in shape (one UV triangle per face)")
    if len(s_ft) != 2 or s_ft[1] != 3 or k_ft != "i" or k_f != "i":
        raise L.IrisError(f"rasterize_uv: ft {s_ft} and f {s_f} must be (F, 3) integer arrays")
    if s_ft[0] > 2 ** 31 - 1:
        raise L.IrisError("rasterize_uv: more than 2^31 - 1 faces")
    if k_vt != "f" or k_v != "f":
        raise L.IrisError("rasterize_uv: vt and v must be floating point")
    if not finite:
        raise L.IrisError("rasterize_uv: vt holds a non-finite UV")
    if vt_lo < -1.0 or vt_hi > 2.0:
        raise L.IrisError(f"rasterize_uv: UVs must lie in [-1, 2] (got [{vt_lo}, {vt_hi}])")
    if s_ft[0] and (ft_lo < 0 or ft_hi >= s_vt[0]):
        raise L.IrisError(f"rasterize_uv: ft indexes [{ft_lo}, {ft_hi}] outside the {s_vt[0]} UV vertices")
    if s_f[0] and (f_lo < 0 or f_hi >= s_v[0]):
        raise L.IrisError(f"rasterize_uv: f indexes [{f_lo}, {f_hi}] outside the {s_v[0]} vertices")
    return H, W


def _upload(a, dtype, dev):
    t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


class UVMesh:
    """The checked, uploaded inputs of one export: vt (N, 2) f32, ft (F, 3) i32, v (V, 3) f32, f (F, 3) i32 on the device, and the texture size."""

    def __init__(self, vt, ft, v, f, tex_res, device=None):
        L.no_autograd("rasterize_uv", vt, v)
        self.H, self.W = check_inputs(vt, ft, v, f, tex_res)
        if device is None:
            device = next((a.device for a in (vt, ft, v, f) if torch.is_tensor(a) and a.is_cuda), "cuda")
        self.device = torch.device("cuda", L.device_index(device))
        self.vt, self.v = _upload(vt, torch.float32, self.device), _upload(v, torch.float32, self.device)
        self.ft, self.f = _upload(ft, torch.int32, self.device), _upload(f, torch.int32, self.device)
        self.F = int(self.ft.shape[0])

    def raster(self, mode=None):
        """ids (H, W) int32: the face per texel, -1 where uncovered.  mode: None = iris_uv_raster, else IRIS_UV_RASTER_* through iris_debug_uv_raster."""
        lib = L.lib()
        ids = torch.empty(self.H, self.W, dtype=torch.int32, device=self.device)
        need = int(lib.iris_uv_raster_workspace_bytes(self.F))
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            if mode is None:
                L.check(lib.iris_uv_raster(L.ptr(self.vt), self.vt.shape[0], L.ptr(self.ft), self.F, self.H, self.W, L.ptr(ids), L.ptr(ws), need, L.stream()))
            else:
                L.check(lib.iris_debug_uv_raster(L.ptr(self.vt), self.vt.shape[0], L.ptr(self.ft), self.F, self.H, self.W, L.ptr(ids), L.ptr(ws), need, int(mode),
                                                 L.stream()))
        return ids

    def resolve(self, ids, texel0=0, n=None, bary=True):
        """(bary (n, 2) or None, xyz (n, 3)) of the texels [texel0, texel0 + n) of the texture rasterised into ids."""
        n = self.H * self.W - texel0 if n is None else int(n)
        b = torch.empty(n, 2, device=self.device) if bary else None
        xyz = torch.empty(n, 3, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().iris_uv_resolve(L.ptr(self.vt), self.vt.shape[0], L.ptr(self.ft), L.ptr(self.v), self.v.shape[0], L.ptr(self.f), self.F, self.H, self.W,
                                            L.ptr(ids), int(texel0), n, L.ptr(b), L.ptr(xyz), L.stream()))
        return b, xyz


def rasterize_uv(vt, ft, v, f, tex_res, device=None):
    """Rasterise the UV triangles (vt (N, 2), ft (F, 3)) into a texture of tex_res (an integer, or (H, W)) and interpolate the mesh (v (V, 3), f (F, 3)) there:
    what `dr.rasterize` + `dr.interpolate` give the reference (utils/export.py:83-92), under this project's exact contract.  Inputs: GPU tensors or host arrays.
    -> {'ids' (H, W) int32, -1 uncovered; 'mask' (H, W) bool; 'bary' (H, W, 2) f32, weights of vertices 0 and 1; 'xyz' (H, W, 3) f32}, device tensors
    (zeros where uncovered).  No backward pass: an input that requires grad raises."""
    m = UVMesh(vt, ft, v, f, tex_res, device)
    ids = m.raster()
    bary, xyz = m.resolve(ids)
    return {"ids": ids, "mask": ids >= 0, "bary": bary.reshape(m.H, m.W, 2), "xyz": xyz.reshape(m.H, m.W, 3)}


def quantize_into(albedo, roughness, metallic, ids, texel0, albedo_img, rm_img):
    """iris_texture_quantize: float32 albedo (n, 3), roughness (n[, 1]), metallic (n[, 1]) of the texels [texel0, texel0 + n) -> their bytes of the two
    (H, W, 3) uint8 images; 0 where ids < 0."""
    albedo = L.require_gpu(albedo, torch.float32, "albedo").detach().reshape(-1, 3)
    roughness = L.require_gpu(roughness, torch.float32, "roughness").detach().reshape(-1)
    metallic = L.require_gpu(metallic, torch.float32, "metallic").detach().reshape(-1)
    n = albedo.shape[0]
    if roughness.shape[0] != n or metallic.shape[0] != n:
        raise L.IrisError(f"quantize: albedo {n}, roughness {roughness.shape[0]} and metallic {metallic.shape[0]} texels differ")
    ids = L.require_gpu(ids, torch.int32, "ids")
    for img in (albedo_img, rm_img):
        if img.dtype != torch.uint8 or not img.is_contiguous() or img.numel() != ids.numel() * 3 or img.device != ids.device:
            raise L.IrisError("quantize: the images must be contiguous (H, W, 3) uint8 tensors on the device of ids")
    with torch.cuda.device(ids.device):
        L.check(L.lib().iris_texture_quantize(L.ptr(albedo), L.ptr(roughness), L.ptr(metallic), L.ptr(ids), int(texel0), n, ids.numel(), L.ptr(albedo_img),
                                              L.ptr(rm_img), L.stream()))


MAX_DILATE = 4


def check_dilate(n):
    """-> n as an int; IrisError unless it is an integer in [0, 4]"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= MAX_DILATE:
        raise L.IrisError(f"dilate = {n!r}: an integer in [0, {MAX_DILATE}]")
    return int(n)


def dilate_into(ids, albedo_img, rm_img, n):
    """iris_texture_dilate, seam dilation in place: every uncovered texel (ids < 0) of the two (H, W, 3) uint8 images takes the bytes of the covered texel
    within Chebyshev distance n (0 <= n <= 4) that has the smallest squared Euclidean distance, then the smallest row, then the smallest column; it is left as it
    is when there is none.  Covered texels and ids are not changed; n = 0 launches nothing."""
    n = check_dilate(n)
    ids = L.require_gpu(ids, torch.int32, "ids")
    if ids.dim() != 2 or ids.numel() == 0:
        raise L.IrisError(f"dilate: ids {tuple(ids.shape)} must be (H, W)")
    H, W = ids.shape
    for img in (albedo_img, rm_img):
        if not torch.is_tensor(img) or img.dtype != torch.uint8 or not img.is_contiguous() or tuple(img.shape) != (H, W, 3) or img.device != ids.device:
            raise L.IrisError("dilate: the images must be contiguous (H, W, 3) uint8 tensors on the device of ids")
    if albedo_img.data_ptr() == rm_img.data_ptr():
        raise L.IrisError("dilate: albedo and rm are the same image")
    with torch.cuda.device(ids.device):
        L.check(L.lib().iris_texture_dilate(L.ptr(ids), H, W, n, L.ptr(albedo_img), L.ptr(rm_img), L.stream()))


@torch.no_grad()
def bake_textures(material_net, vt, ft, v, f, tex_res, chunk_size=160000, device=None, dilate=0):
    """The material network baked into the UV atlas (utils/export.py:77-135) -> (albedo, rm): two (H, W, 3) uint8 device tensors, rm = (roughness, metallic, 0).
    The ids are rasterised once; then, per chunk of `chunk_size` consecutive texels: resolve, material_net(xyz), quantise.  The network runs on EVERY texel of
    a chunk, covered or not (uncovered ones sit at the origin and are masked by the quantiser): no compaction pass, no host round trip.
    material_net: any callable with NGPBRDF.forward's contract.  dilate = n > 0: dilate_into after the last chunk (seam dilation; the reference has none)."""
    chunk_size = int(chunk_size)
    if chunk_size < 1:
        raise L.IrisError(f"bake_textures: chunk_size = {chunk_size}")
    dilate = check_dilate(dilate)
    m = UVMesh(vt, ft, v, f, tex_res, device)
    ids = m.raster()
    albedo = torch.empty(m.H, m.W, 3, dtype=torch.uint8, device=m.device)
    rm = torch.empty(m.H, m.W, 3, dtype=torch.uint8, device=m.device)
    for texel0 in range(0, m.H * m.W, chunk_size):
        _, xyz = m.resolve(ids, texel0, min(chunk_size, m.H * m.W - texel0), bary=False)
        mat = material_net(xyz)
        quantize_into(mat["albedo"], mat["roughness"], mat["metallic"], ids, texel0, albedo, rm)
    if dilate:
        dilate_into(ids, albedo, rm, dilate)
    return albedo, rm


def check_fit_options(steps, points, lr):
    """The host checks of the fit, before a device is touched -> (steps, points, lr).  IrisError on steps < 0, points < 1, lr <= 0 (or not a number)."""
    for name, n, lo in (("steps", steps, 0), ("points", points, 1)):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < lo:
            raise L.IrisError(f"fit_textures: {name} = {n!r}: an integer >= {lo}")
    if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not float(lr) > 0.0 or not np.isfinite(float(lr)):
        raise L.IrisError(f"fit_textures: lr = {lr!r}: a finite number > 0")
    return int(steps), int(points), float(lr)


def surface_draw(v, f, points, seed, device):
    """The fit's default draw(step) -> (face (points,) int64, bary (points, 2) float32) on the device: 2 * points uniform pairs of iris_philox_u2 with the key
    (seed, stream = step); the first component of pair i < points picks the face by searchsorted on the float64 cumulative face areas (area-proportional),
    pair points + i is the barycentrics, folded into the triangle as export.verify_points folds them (b1 + b2 > 1 -> (1 - b1, 1 - b2))."""
    v64 = torch.as_tensor(_host(v), dtype=torch.float64).reshape(-1, 3)
    f64 = torch.as_tensor(_host(f).astype(np.int64)).reshape(-1, 3)
    p0, p1, p2 = (v64[f64[:, k]] for k in range(3))
    area = 0.5 * torch.linalg.cross(p1 - p0, p2 - p0).norm(dim=-1)
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area))
    cum = torch.cumsum(area, 0)
    if not float(cum[-1]) > 0.0:
        raise L.IrisError("fit_textures: the mesh has no face of finite positive area to draw points on")
    cum_d, total, n_faces = cum.to(device), float(cum[-1]), f64.shape[0]

    def draw(step):
        u = torch.empty(2 * points, 2, device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            L.check(L.lib().iris_philox_u2(int(seed) & (2 ** 64 - 1), 0, int(step) & 0xFFFFFFFF, 2 * points, L.ptr(u), L.stream()))
        face = torch.searchsorted(cum_d, u[:points, 0].double() * total, right=True).clamp_(max=n_faces - 1)
        b = u[points:]
        return face, torch.where((b[:, :1] + b[:, 1:]) > 1.0, 1.0 - b, b).contiguous()
    return draw


def fit_step(material_net, texture_brdf, optimizer, v_d, f_d, face, bary):
    """One step of fit_textures on the points (face, bary); v_d (V, 3) float32 and f_d (F, 3) int64 on the device -> the loss, a 0-d device tensor"""
    b1, b2 = bary[:, :1], bary[:, 1:]
    p0, p1, p2 = (v_d[f_d[face, k]] for k in range(3))
    with torch.no_grad():
        want = material_net(((1.0 - b1 - b2) * p0 + b1 * p1) + b2 * p2)
        want = torch.cat([want["albedo"].reshape(-1, 3), want["roughness"].reshape(-1, 1), want["metallic"].reshape(-1, 1)], dim=1)
    got = texture_brdf.sample(face, bary)
    loss = ((torch.cat([got["albedo"], got["roughness"], got["metallic"]], dim=1) - want) ** 2).mean()
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach()


def fit_textures(material_net, texture_brdf, v, f, steps, points, lr, seed=0, draw=None):
    """Least-squares fit of a model.texture.TextureBRDF to the network it was baked from: what the bake's point sampling at texel centres
    and its truncation to 8 bits lose against the bilinear read-back is won back, the texels just outside a chart -- which dilation only copies -- included.
    Per step: (face, bary) = draw(step); position = ((1 - b1 - b2) p0 + b1 p1) + b2 p2 in float32 (verify_points' order); target = material_net(position) under
    no_grad; prediction = texture_brdf.sample(face, bary); loss = the mean over the points and the 5 channels of the squared difference; one FusedAdam step at lr.
    draw: None = surface_draw(v, f, points, seed, device), area-proportional; or a callable step -> (face int64 (M,), bary float32 (M, 2)) on the device.
    -> {'steps', 'first_loss', 'last_loss'} (the losses are None for steps = 0; they are read back once, after the last step)."""
    from .optim import FusedAdam
    steps, points, lr = check_fit_options(steps, points, lr)
    dev = texture_brdf.texels.device
    report = {"steps": steps, "first_loss": None, "last_loss": None}
    if steps == 0:
        return report
    v_d, f_d = _upload(v, torch.float32, dev).reshape(-1, 3), _upload(f, torch.int64, dev).reshape(-1, 3)
    if draw is None:
        draw = surface_draw(v, f, points, seed, dev)
    optimizer = FusedAdam([texture_brdf.texels], lr=lr)
    first = last = None
    for step in range(steps):
        last = fit_step(material_net, texture_brdf, optimizer, v_d, f_d, *draw(step))
        if step == 0:
            first = last
    report["first_loss"], report["last_loss"] = float(first), float(last)
    return report


def grid_atlas(n_faces, tex_res):
    """The stand-in for xatlas, which is not a dependency: (vt (3F, 2) float32, ft = arange(3F).reshape(F, 3) int32), host numpy.
    Every face gets its own three UV vertices.  Two faces share a cell of a G x G grid, G = ceil(sqrt(ceil(F / 2))), as the two halves on either side of the
    cell's diagonal; each is inset by a quarter texel from the cell and from the diagonal, so that no texel centre is covered by two faces, and at a tex_res
    that gives cells of 4 texels or more every face covers a texel centre.
    It IGNORES the triangles' shape and area: every face gets the same right triangle.  Valid (a bijection onto disjoint charts), but not a good atlas: no
    chart shares an edge with its neighbour in 3-D, texel density is unrelated to surface area.  An atlas made elsewhere drops in as vt.npy / ft.npy."""
    F = int(n_faces)
    if F < 1:
        raise L.IrisError(f"grid_atlas: n_faces = {n_faces}")
    H, W = _hw(tex_res)
    G = int(np.ceil(np.sqrt((F + 1) // 2)))
    while G * G < (F + 1) // 2:
        G += 1
    m = g = 0.25                                                   # texels: margin to the cell's border, half gap along the diagonal
    cell = np.arange((F + 1) // 2)
    x0, y0 = (cell % G) * (W / G), (cell // G) * (H / G)           # the cell's corner, texels (float64)
    x1, y1 = x0 + W / G, y0 + H / G
    lower = np.stack([np.stack([x0 + m, y0 + m], -1), np.stack([x1 - m - g, y0 + m], -1), np.stack([x0 + m, y1 - m - g], -1)], 1)       # (cells, 3, 2)
    upper = np.stack([np.stack([x1 - m, y1 - m], -1), np.stack([x0 + m + g, y1 - m], -1), np.stack([x1 - m, y0 + m + g], -1)], 1)
    tri = np.stack([lower, upper], 1).reshape(-1, 3, 2)[:F]        # faces 2 k and 2 k + 1 share cell k
    vt = (tri / np.array([W, H], np.float64)).reshape(-1, 2).astype(np.float32)
    return vt, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


ATLAS_KMIN, ATLAS_JMIN, ATLAS_JMAX = 2, -800, 800              # iris_amd/csrc/iris_atlas.h kAtlasKMin, kAtlasJMin, kAtlasJMax


def atlas_min_res(n_faces):
    """the smallest power of two R whose R x R texels hold ceil(F / 2) cells of 4 x 4 (it may exceed MAX_TEX_RES)"""
    R = 4
    while (int(n_faces) + 1) // 2 * 16 > R * R:
        R *= 2
    return R


def check_atlas_inputs(v, f, tex_res):
    """The host checks of area_atlas, before a device is touched -> (R, KMAX, V, F).  IrisError on: a tex_res that is not a square power of two in [4, 8192];
    v not (V, 3) floating point, f not (F, 3) integers, F < 1; more faces than R x R texels hold at two per 4 x 4 cell.  The VALUES of v and f are not looked at:
    a face that names a vertex out of range or has no finite positive area is part of the contract (it gets the smallest chart)."""
    if isinstance(tex_res, (tuple, list)):
        if len(tex_res) != 2 or tex_res[0] != tex_res[1]:
            raise L.IrisError(f"area_atlas: tex_res = {tex_res!r}: the atlas is built for a square texture (an integer, or (R, R))")
        tex_res = tex_res[0]
    if isinstance(tex_res, bool) or not isinstance(tex_res, (int, np.integer)) or not 4 <= int(tex_res) <= MAX_TEX_RES or int(tex_res) & (int(tex_res) - 1):
        raise L.IrisError(f"area_atlas: tex_res = {tex_res!r}: a power of two in [4, {MAX_TEX_RES}]")
    R = int(tex_res)

    def shape_kind(a):
        if torch.is_tensor(a):
            return tuple(a.shape), "f" if a.is_floating_point() else "i" if a.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) else "?"
        a = np.asarray(a)
        return a.shape, "f" if a.dtype.kind == "f" else "i" if a.dtype.kind in "iu" else "?"
    (s_v, k_v), (s_f, k_f) = shape_kind(v), shape_kind(f)
    if len(s_v) != 2 or s_v[1] != 3 or k_v != "f":
        raise L.IrisError(f"area_atlas: v {s_v} must be a floating-point (V, 3) array")
    if len(s_f) != 2 or s_f[1] != 3 or k_f != "i" or s_f[0] < 1:
        raise L.IrisError(f"area_atlas: f {s_f} must be an integer (F, 3) array with F >= 1")
    F = int(s_f[0])
    if s_v[0] > 2 ** 31 - 1:
        raise L.IrisError("area_atlas: more than 2^31 - 1 vertices")
    if (F + 1) // 2 * 16 > R * R:
        need = atlas_min_res(F)
        raise L.IrisError(f"area_atlas: {F} faces need {(F + 1) // 2} cells of 4 x 4 texels and tex_res = {R} holds {R * R // 16}: the smallest tex_res that holds "
                          f"them is {need}" + ("" if need <= MAX_TEX_RES else f", above the limit of {MAX_TEX_RES}"))
    return R, R.bit_length() - 1, int(s_v[0]), F


def _faces_i32(f, n_v, dev):
    """f as (F, 3) int32 on the device; an index that int32 could not hold (or any other outside [0, n_v)) arrives as -1 instead of wrapping into range"""
    if torch.is_tensor(f):
        t = f.detach()
    else:
        a = np.asarray(f)
        t = torch.from_numpy(np.ascontiguousarray(a if a.dtype.kind == "i" else a.astype(np.int64)))          # (torch has no unsigned types beyond uint8)
    if t.dtype != torch.int32:
        t = t.to(torch.int64)
        t = t.masked_fill((t < 0) | (t >= n_v), -1)
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _atlas_texels(hist):
    return sum((int(n) + 1) // 2 * 4 ** k for k, n in enumerate(hist))


def area_atlas(v, f, tex_res, device=None):
    """The built-in atlas that respects surface area (the kernels and the contract are in iris_amd/csrc/iris_atlas.h, the numpy
    restatement in tests/atlas_ref.py): v (V, 3) float, f (F, 3) integer, host arrays or device tensors; tex_res = R, a square power of two in [4, 8192]
    -> (vt (3 F, 2) float32, ft = arange(3 F).reshape(F, 3) int32, report), vt and ft DEVICE tensors that UVMesh / bake_textures take as they are.
    Every face is a chart of its own, as in grid_atlas, but its cell is a 2^k x 2^k square with 4 16^k >= S_f D_j > 4 16^(k - 1), S_f four times the squared
    area in float64 and D_j = M[j mod 2] 2^floor(j / 2) the density of the ladder that a bisection over j in [-800, 800] ends at: all cells fit the texture at
    step j and not at j + 1 (the texel sum is monotone in j except where a face moves into the free half of a cell, so this is the bisection's j, stated in
    DESIGN.md, and not in every case the largest that fits).  An unclamped face gets between
    1 / 2 and 2 times sqrt(D_j) area texels.  Cells are placed without a search, by class (largest first), face index and Morton order; the longest edge lies
    on the cell's diagonal.  Integers and float64 in one stated order: bit for bit the restatement's result.
    report: j, D_j, histogram (faces per class 0 .. KMAX), used (share of the texels inside cells), clamped_min / clamped_max (faces whose class the limits
    KMIN = 2 and 2^KMAX = R changed; faces without a finite positive area count as clamped_min).
    Refused (IrisError, before anything is launched): the sizes check_atlas_inputs lists.  Refused after the first probe: areas so large (beyond about 1e60,
    coordinates beyond 1e30) that even the ladder's lowest density does not fit.
    Still per-face charts: no chart of several faces, no shape preservation (every chart is the same right isosceles triangle), no non-square texture."""
    L.no_autograd("area_atlas", v)
    R, kmax, V, F = check_atlas_inputs(v, f, tex_res)
    if device is None:
        device = next((a.device for a in (v, f) if torch.is_tensor(a) and a.is_cuda), "cuda")
    dev = torch.device("cuda", L.device_index(device))
    lib = L.lib()
    v_d, f_d = _upload(v, torch.float32, dev), _faces_i32(f, V, dev)
    S = torch.empty(F, dtype=torch.float64, device=dev)
    corner = torch.empty(F, dtype=torch.uint8, device=dev)
    k = torch.empty(F, dtype=torch.uint8, device=dev)
    hist = torch.empty(16, dtype=torch.int64, device=dev)
    vt = torch.empty(3 * F, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.mark()
        L.check(lib.iris_atlas_measure(L.ptr(v_d), V, L.ptr(f_d), F, L.ptr(S), L.ptr(corner), L.stream()))
        L.mark("measure")

        def probe(j):
            L.check(lib.iris_atlas_classes(L.ptr(S), F, j, R, L.ptr(k), L.ptr(hist), L.stream()))
            h = hist.cpu().tolist()                         # (the one small read per probe)
            L.mark("classes")
            return h
        h = probe(ATLAS_JMIN)
        if _atlas_texels(h[:14]) > R * R:
            raise L.IrisError(f"area_atlas: the faces do not fit {R} x {R} texels even at the lowest density of the ladder (j = {ATLAS_JMIN}): "
                              "some face's area is beyond about 1e60")
        lo, hi, probed = ATLAS_JMIN, ATLAS_JMAX + 1, ATLAS_JMIN          # lo fits, hi does not: the contract's bisection, step for step
        while hi - lo > 1:
            mid = (lo + hi) // 2
            h_mid = probe(mid)
            probed = mid
            if _atlas_texels(h_mid[:14]) <= R * R:
                lo, h = mid, h_mid
            else:
                hi = mid
        j = lo
        if probed != j:
            h = probe(j)                                    # k of the chosen step
        order = torch.sort(k, stable=True)[1]               # by class, the face index breaking ties: position - class start is the rank within the class
        L.mark("rank")
        L.check(lib.iris_atlas_place(L.ptr(k), L.ptr(corner), L.ptr(order), F, R, (C.c_int64 * 14)(*h[:14]), L.ptr(vt), L.stream()))
        L.mark("place")
        ft = torch.arange(3 * F, dtype=torch.int32, device=dev).reshape(F, 3)
    report = {"j": j, "D_j": float(lib.iris_atlas_density(j)), "histogram": [int(n) for n in h[:kmax + 1]], "used": _atlas_texels(h[:14]) / (R * R),
              "clamped_min": int(h[14]), "clamped_max": int(h[15])}
    return vt, ft, report


def write_png(path, rgb_uint8):
    """8-bit RGB PNG of an (H, W, 3) uint8 array (host array or tensor) with the standard library alone: every scanline with filter 0, one IDAT chunk."""
    a = _host(rgb_uint8)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise L.IrisError(f"write_png: expected an (H, W, 3) uint8 image, got {a.shape} {a.dtype}")
    H, W = a.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(a).reshape(H, W * 3)], 1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_textured_obj(dir_save, v, f, vt, ft):
    """<dir>/mesh.obj (v, vt, f a/ta b/tb c/tc; floats with 9 significant digits: float32 round-trips) and <dir>/mesh.mtl with map_Kd albedo.png: what makes
    the export folder loadable (the reference leaves that to the user).  vt is written as it is: image row 0 is v ~ 0, the reference's layout."""
    v, f, vt, ft = _host(v), _host(f), _host(vt), _host(ft)
    with open(os.path.join(dir_save, "mesh.mtl"), "w") as fh:
        fh.write("newmtl material_0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nmap_Kd albedo.png\n")
    with open(os.path.join(dir_save, "mesh.obj"), "w") as fh:
        fh.write("mtllib mesh.mtl\nusemtl material_0\n")
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p) for p in v))
        fh.write("".join("vt %.9g %.9g\n" % tuple(float(x) for x in p) for p in vt))
        fh.write("".join("f %d/%d %d/%d %d/%d\n" % (a[0] + 1, b[0] + 1, a[1] + 1, b[1] + 1, a[2] + 1, b[2] + 1) for a, b in zip(f.tolist(), ft.tolist())))
