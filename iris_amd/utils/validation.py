"""The trainers' validation (reference: train_brdf_crf.py:331-499, the same lines in train_emitter.py and initialize.py): `val/loss` and `val/psnr` of the
diffuse reflectance albedo * (1 - metallic) over the validation views, and the images validation() writes every val_step steps.

  kd_validation_loss      validation_step after the material network, for a stack of views: one fused HIP reduction (iris_amd/csrc/iris_validate.h,
                          `iris_val_kd_loss`) without atomics -- val/loss decides which checkpoint is kept, so equal parameters give equal bits, on every call
                          and for a view alone or in a stack.
  validation_intrinsics   validation()'s material maps: `iris_render_primary`, the material network, `iris_val_intrinsics`, per chunk of pixels, as
                          utils.render.render_intrinsics.
  ValidationSet           the validation views of a scene resident on the device; evaluate() -> what Lightning logs (the mean of the per-view values).
  validation_images       validation() for one view: the eight PNGs, through the device PNG encoder.  Not built: crfs.png and crfs_weight.png (matplotlib).

The gamma table of the real layouts' stand-in ground truth (`rgb.pow(1 / 2.2).clamp(0, 1)`, :486) is built on the host in float64, once: torch's CPU pow gives
position-dependent last bits for equal inputs (vector lanes and the scalar tail differ), a table does not.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib as L

GAMMA = 2.2
MAPS = (("albedo", 3), ("roughness", 1), ("metallic", 1), ("emission", 3))
IMAGE_NAMES = ("L_train", "L_full", "L_gt", "mat_albedo", "mat_roughness", "mat_metallic", "emission", "mask")
MODES = ("none", "metric", "images", "all")

_lut = None


def gamma_table():
    """(256,) float32: lut[c] = float32(clip(float64(float32(c / 255)) ** (1 / 2.2), 0, 1)), what `rgb.pow(1 / GAMMA).clamp(0, 1)` is of the photograph's code c
    (the datasets hold float32(c / 255)), evaluated in float64 and rounded once.  Within 2^-24 of torch's float32 pow on all 256 codes."""
    global _lut
    if _lut is None:
        x = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64)
        _lut = np.clip(x ** (1.0 / GAMMA), 0.0, 1.0).astype(np.float32)
    return _lut.copy()


_lut_dev = {}


def _gamma_table_on(dev):
    key = (dev.type, L.device_index(dev))
    if key not in _lut_dev:
        _lut_dev[key] = torch.from_numpy(gamma_table()).to(dev)
    return _lut_dev[key]


def _flat(t, dtypes, name, numel):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.IrisError(f"kd_validation_loss: {name}: expected a tensor on a HIP device (got {getattr(t, 'device', type(t))}); iris_amd has no CPU path")
    if t.dtype not in dtypes:
        raise L.IrisError(f"kd_validation_loss: {name} has dtype {t.dtype}; expected {' or '.join(str(d) for d in dtypes)}")
    if t.numel() != numel:
        raise L.IrisError(f"kd_validation_loss: {name} has shape {tuple(t.shape)}: {numel} values expected")
    return t.detach().contiguous()


def kd_validation_loss(albedo, metallic, valid, *, gt=None, emit=None, codes=None, img_hw):
    """validation_step (:456-499) after the material network, for N views of img_hw = (H, W) pixels in one launch pair.
    albedo (N*HW, 3), metallic (N*HW) or (N*HW, 1) float32: the network's outputs at the pixel-centre primary hits of ALL pixels; valid (N*HW) bool or uint8.
    Ground truth, exactly one of:  gt and emit, (N*HW, 3) float32 -- a synthetic scene's DiffCol and Emit maps (pixels whose emission sums to 0 count);
                                   codes, (N*HW, 3) uint8 -- the photograph, scored against gamma_table()[codes] at every pixel.
    (Leading dimensions may be split, (N, H, W, 3): only the element count and the order matter.)
    -> {'S' (N,) float64: the sum of squared differences of a view, 'loss' = S / (3 H W), 'psnr' = -10 log10(max(loss, 1e-5))}, device tensors, float64;
    nothing synchronises with the host.  The per-element contract: include/iris_hip.h, iris_val_kd_loss."""
    H, W = int(img_hw[0]), int(img_hw[1])
    if H < 1 or W < 1:
        raise L.IrisError(f"kd_validation_loss: img_hw {tuple(img_hw)}: positive sizes expected")
    synthetic = gt is not None or emit is not None
    if synthetic == (codes is not None):
        raise L.IrisError("kd_validation_loss: pass either gt and emit (float32, a synthetic scene's maps) or codes (uint8, the photograph), not both and not neither")
    if synthetic and (gt is None or emit is None):
        raise L.IrisError("kd_validation_loss: the synthetic mode takes both gt and emit")
    if not isinstance(valid, torch.Tensor):
        raise L.IrisError(f"kd_validation_loss: valid: expected a tensor on a HIP device (got {type(valid)})")
    n = valid.numel()
    if n == 0 or n % (H * W):
        raise L.IrisError(f"kd_validation_loss: valid has {n} elements, not a positive multiple of H W = {H * W}")
    N = n // (H * W)
    f32 = (torch.float32,)
    valid = _flat(valid, (torch.bool, torch.uint8), "valid", n)
    albedo = _flat(albedo, f32, "albedo", 3 * n)
    metallic = _flat(metallic, f32, "metallic", n)
    dev = valid.device
    if synthetic:
        gt_t, emit_t, lut = _flat(gt, f32, "gt", 3 * n), _flat(emit, f32, "emit", 3 * n), None
    else:
        gt_t, emit_t, lut = _flat(codes, (torch.uint8,), "codes", 3 * n), None, _gamma_table_on(dev)
    for name, t in (("albedo", albedo), ("metallic", metallic), ("gt" if synthetic else "codes", gt_t), ("emit", emit_t)):
        if t is not None and t.device != dev:
            raise L.IrisError(f"kd_validation_loss: {name} is on {t.device}, valid on {dev}")
    lib = L.lib()
    need = int(lib.iris_val_kd_loss_workspace_bytes(N, H, W))
    if need == 0:
        raise L.IrisError(f"kd_validation_loss: size (N, H, W) = {(N, H, W)} is not supported: N, H, W >= 1, H W <= 2^30, N ceil(H W / 512) < 2^31")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    S = torch.empty(N, dtype=torch.float64, device=dev)
    a = L.ValKdLossArgs(albedo=L.ptr(albedo), metallic=L.ptr(metallic), valid=L.ptr(valid), gt=L.ptr(gt_t), emit=L.ptr(emit_t), lut=L.ptr(lut), sums=L.ptr(S),
                        workspace=L.ptr(ws), workspace_bytes=need, gt_is_u8=int(not synthetic), N=N, H=H, W=W)
    with torch.cuda.device(dev):
        L.check(lib.iris_val_kd_loss(C.byref(a), L.stream()))
    # (tensor / tensor: a correctly rounded float64 division; torch divides a device tensor by a Python scalar as a product with the reciprocal)
    loss = S / torch.full_like(S, float(3 * H * W))
    psnr = -10.0 * torch.log10(torch.clamp_min(loss, 1e-5))
    return {"S": S, "loss": loss, "psnr": psnr}


def new_maps(B, device):
    """the four zeroed maps validation_intrinsics accumulates into, as validation() allocates them (:356-359): albedo, emission (B,3), roughness, metallic (B,1)"""
    return {k: torch.zeros(B, c, device=device, dtype=torch.float32) for k, c in MAPS}


@torch.no_grad()
def validation_intrinsics(scene, emitter_net, material_net, rays_o, rays_d, dx_du, dy_dv, spp, out=None, uniforms=None, chunk=None, debug=None):
    """One round of validation()'s intrinsics (:372-396): `map += mean over spp jittered samples` of albedo, roughness and metallic -- a sample that misses the
    mesh, or hits an emitter whose radiance row does not sum to zero, counts as 0 -- and of the emission, unmasked.

    rays_o, rays_d, dx_du, dy_dv: (B,3) float32 on the GPU.  out: a dict from `new_maps` (or an earlier call) to accumulate into; None = fresh zeroed maps.
    uniforms: optional [rand(2,B,spp,1)], the draw of :373 (parity mode); otherwise the function draws with torch.rand, one generator call per chunk.
    chunk: pixels per pass (default: utils.render.CHUNK_SAMPLES // spp); per-pixel sums are independent, so chunking changes no bit when the draw is given.
    debug: optional dict that receives the per-sample e0, valid_next and network outputs (albedo, roughness, metallic) of the call (tests).
    Per pixel: map[b] += (x_0 + ... + x_{spp-1}) * (1.0f / spp), samples added in order in float32 (include/iris_hip.h).  Returns the dict of maps."""
    from .path_tracing import _mat_tensors
    from .render import CHUNK_SAMPLES
    spp = int(spp)
    if spp < 1:
        raise L.IrisError(f"validation_intrinsics: spp ({spp}) must be at least 1")
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
            raise L.IrisError(f"validation_intrinsics: out[{k!r}] must be a contiguous float32 tensor of {B * c} values (got shape {tuple(out[k].shape)})")
        maps[k] = m
    if uniforms is not None:
        if len(uniforms) != 1:
            raise L.IrisError(f"validation_intrinsics: uniforms has {len(uniforms)} tensors, a round draws one (rand(2,B,spp,1))")
        dudv_all = L.require_gpu(uniforms[0], torch.float32, "uniforms[0]")
        if dudv_all.numel() != 2 * B * spp:
            raise L.IrisError(f"validation_intrinsics: uniforms[0] has shape {tuple(dudv_all.shape)}, expected (2,{B},{spp},1)")
        dudv_all = dudv_all.reshape(2, B, spp)
    step = max(1, CHUNK_SAMPLES // spp) if chunk is None else int(chunk)
    if step < 1:
        raise L.IrisError(f"validation_intrinsics: chunk ({chunk}) must be at least 1 pixel")
    lib = L.lib()
    rows = {"e0": [], "valid_next": [], "albedo": [], "roughness": [], "metallic": []}
    with torch.cuda.device(dev):
        eh = emitter_net.handle(dev)
        radiance = emitter_net.radiance_on(dev)
        for b0 in range(0, B, step):
            b1 = min(b0 + step, B)
            Bc = b1 - b0
            N = Bc * spp
            L.mark()
            dudv = dudv_all[:, b0:b1].contiguous() if uniforms is not None else torch.rand(2, Bc, spp, device=dev)
            wi = torch.empty(N, 3, device=dev); wo = torch.empty(N, 3, device=dev); pos = torch.empty(N, 3, device=dev); nrm = torch.empty(N, 3, device=dev)
            e0 = torch.empty(N, device=dev, dtype=torch.int32); valid_next = torch.empty(N, device=dev, dtype=torch.bool)
            ro, rd, dxu, dyv = rays_o[b0:b1], rays_d[b0:b1], dx_du[b0:b1], dy_dv[b0:b1]
            L.check(lib.iris_render_primary(scene.handle, eh, L.ptr(ro), L.ptr(rd), L.ptr(dxu), L.ptr(dyv), L.ptr(dudv), Bc, spp, L.ptr(wi), L.ptr(wo), L.ptr(pos),
                                            L.ptr(nrm), L.ptr(e0), L.ptr(valid_next), L.stream()))
            L.mark("jitter + primary hit")
            albedo, rough, metal = _mat_tensors(material_net(pos))
            if albedo.shape[0] != N or rough.shape[0] != N or metal.shape[0] != N:
                raise L.IrisError(f"validation_intrinsics: material_net returned {albedo.shape[0]} / {rough.shape[0]} / {metal.shape[0]} rows for {N} positions")
            L.mark("material network")
            o = {k: maps[k].reshape(B, c)[b0:b1] for k, c in MAPS}
            L.check(lib.iris_val_intrinsics(eh, L.ptr(radiance), L.ptr(e0), L.ptr(valid_next), L.ptr(albedo), L.ptr(rough), L.ptr(metal), Bc, spp,
                                            L.ptr(o["albedo"]), L.ptr(o["roughness"]), L.ptr(o["metallic"]), L.ptr(o["emission"]), L.stream()))
            L.mark("intrinsics kernel")
            if debug is not None:
                for k, t in zip(rows, (e0, valid_next, albedo, rough, metal)):
                    rows[k].append(t)
    if debug is not None:
        debug.update({k: torch.cat(v) for k, v in rows.items()})
    return out


# ---- the files of the validation split (host only)
def _header_size(path):
    """(H, W) of an image file from its header; IrisError when there is no such file"""
    if not os.path.isfile(path):
        raise L.IrisError(f"{path}: no such file (a file of the validation split)")
    if path.lower().endswith(".exr"):
        from .exr import read_exr_header
        h = read_exr_header(path)
        return int(h["height"]), int(h["width"])
    from PIL import Image
    from .dataset.files import _check_eight_bit
    with Image.open(path) as im:
        _check_eight_bit(path, im)
        return int(im.size[1]), int(im.size[0])


def validation_files(dataset, root, scene=None, ldr_img_dir=None, res_scale=1.0):
    """What a ValidationSet is loaded from, found and checked on the host (headers only: nothing is decoded, no device is opened) ->
    dict(dataset, img_hw, views, photographs [paths], exposure (V,) float32, synthetic, resize, diffcol [paths] or None, emit [paths] or None).
        real       the 'val' split (views 0, 10, .. 150 of the capture): <root>/<ldr_img_dir>/{id:03d}_0001.png, <ldr_img_dir>/cam/exposure.npy[id]
        synthetic  <root>/val: transforms.json, <ldr_img_dir>/{i:03d}_0001.png, <ldr_img_dir>/cam/exposure.npy, DiffCol/{i:03d}_0001.exr, Emit/{i:03d}_0001.exr
        scannetpp  the 'test' list: psdf/images/<name>, exposure 1; the 8-bit files may have any size (resized on the device, as the training photographs)
    IrisError for every file that is missing or of the wrong size, and for a split without views."""
    from . import cameras
    from .dataset.files import _image_size
    from .stage import layout_resizes
    if dataset not in ("real", "synthetic", "scannetpp"):
        raise L.IrisError(f"--dataset {dataset}: expected real, synthetic or scannetpp")
    resize = layout_resizes(dataset)
    diffcol = emit = None
    if dataset == "scannetpp":
        psdf = os.path.join(root, "data", scene or "", "psdf")
        for name in ("train_test_lists.json", "transforms_all.json"):
            if not os.path.isfile(os.path.join(psdf, name)):
                raise L.IrisError(f"validation: {os.path.join(psdf, name)} is missing")
        img_hw, views = cameras.load_scannetpp(root, scene or "", res_scale, split="test")
        photos = [os.path.join(psdf, "images", v["name"]) for v in views]
        exposure = np.ones(len(views), np.float32)
        where = f"{psdf}: the test list"
    else:
        if float(res_scale) != 1.0:
            raise L.IrisError(f"--res_scale {res_scale}: resizing the validation images is built for the scannetpp layout only")
        if not ldr_img_dir:
            raise L.IrisError("--ldr_img_dir is needed: the validation views' photographs and exposures lie there")
        synthetic = dataset == "synthetic"
        data_root = os.path.join(root, "val") if synthetic else root
        img_dir = os.path.join(data_root, ldr_img_dir)
        if synthetic:
            if not os.path.isfile(os.path.join(data_root, "transforms.json")):
                raise L.IrisError(f"validation: {os.path.join(data_root, 'transforms.json')} is missing (the synthetic layout's val split)")
            ids, n_total = None, None
        else:
            if not os.path.isfile(os.path.join(root, "cam.txt")):
                raise L.IrisError(f"validation: {os.path.join(root, 'cam.txt')} is missing")
            with open(os.path.join(root, "cam.txt")) as fh:
                n_total = int(fh.readline())
            ids = cameras.real_split_ids(n_total, "val")
        first = os.path.join(img_dir, "%03d_0001.png" % (ids[0] if ids else 0))
        if not os.path.isfile(os.path.join(data_root, "Image", "000_0001.exr")) and not os.path.isfile(first):
            raise L.IrisError(f"{first}: no such file (the first photograph of the validation split)")
        img_hw = _image_size(data_root, first)
        # the training views' size, by load_training_files' rule: the validation views are rendered and scored at the size the stage trains at
        train_root = os.path.join(root, "train") if synthetic else root
        train_first = os.path.join(train_root, ldr_img_dir, "%03d_0001.png" % (0 if synthetic else (cameras.real_split_ids(n_total, "train") or [0])[0]))
        if os.path.isfile(os.path.join(train_root, "Image", "000_0001.exr")) or os.path.isfile(train_first):
            train_hw = _image_size(train_root, train_first)
            if tuple(train_hw) != tuple(img_hw):
                raise L.IrisError(f"{first}: the validation views are {img_hw[0]} x {img_hw[1]}, the training views {train_hw[0]} x {train_hw[1]}")
        img_hw, views = (cameras.load_synthetic(root, img_hw=img_hw, split="val") if synthetic else cameras.load_real(root, img_hw=img_hw, split="val"))
        ids = list(range(len(views))) if ids is None else ids
        if len(ids) != len(views):
            raise L.IrisError(f"{root}: {len(views)} cameras for {len(ids)} validation views")
        photos = [os.path.join(img_dir, "%03d_0001.png" % i) for i in ids]
        table_path = os.path.join(img_dir, "cam", "exposure.npy")
        if not os.path.isfile(table_path):
            raise L.IrisError(f"{table_path}: no such file (the validation views' exposures)")
        table = np.load(table_path).astype(np.float32).reshape(-1)
        if ids and table.shape[0] <= max(ids):
            raise L.IrisError(f"{table_path} holds {table.shape[0]} values, the validation views reach id {max(ids)}")
        exposure = table[ids] if ids else np.zeros(0, np.float32)
        if synthetic:
            diffcol = [os.path.join(data_root, "DiffCol", "%03d_0001.exr" % i) for i in ids]
            emit = [os.path.join(data_root, "Emit", "%03d_0001.exr" % i) for i in ids]
        where = f"{data_root}: the val split"
    if not views:
        raise L.IrisError(f"{where} has no views: nothing to validate on")
    if min(img_hw) < 1:
        raise L.IrisError(f"validation: --res_scale {res_scale} leaves views of {img_hw[0]} x {img_hw[1]} pixels")
    for p in photos:
        size = _header_size(p)
        if size != tuple(img_hw) and not resize:
            raise L.IrisError(f"{p}: the photograph is {size[0]} x {size[1]}, the validation views {img_hw[0]} x {img_hw[1]}")
    for p in (diffcol or []) + (emit or []):
        size = _header_size(p)
        if size != tuple(img_hw):
            raise L.IrisError(f"{p}: the map is {size[0]} x {size[1]}, the validation views {img_hw[0]} x {img_hw[1]}")
    return dict(dataset=dataset, img_hw=tuple(int(s) for s in img_hw), views=views, photographs=photos, exposure=np.asarray(exposure, np.float32),
                synthetic=dataset == "synthetic", resize=resize, diffcol=diffcol, emit=emit)


def check_validation_args(args):
    """the host-side refusals of a trainer's --validate (stage.refuse_unbuilt_training calls it): the mode's name, the validation split's files
    (validation_files), --val_frame inside the split and --val_step, SPP // spp positive where images are written -> validation_files' dict, or None for
    'none'.  Nothing touches a device."""
    mode = getattr(args, "validate", "none") or "none"
    if mode not in MODES:
        raise L.IrisError(f"--validate {mode}: expected one of {', '.join(MODES)}")
    if mode == "none":
        return None
    dataset, root = args.dataset
    files = validation_files(dataset, root, args.scene, args.ldr_img_dir, args.res_scale)
    if mode in ("images", "all"):
        if not 0 <= int(args.val_frame) < len(files["views"]):
            raise L.IrisError(f"--val_frame {args.val_frame}: the validation split has {len(files['views'])} views")
        if int(args.val_step) < 1:
            raise L.IrisError(f"--val_step {args.val_step}: a positive number of steps is expected")
        if int(args.spp) < 1 or int(args.SPP) // int(args.spp) < 1:
            raise L.IrisError(f"--SPP {args.SPP} --spp {args.spp}: expected 1 <= spp <= SPP (the validation images take SPP // spp rounds of spp samples)")
    return files


def _rgb_codes(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _rgb_exr(path):
    from .exr import read_exr
    a = read_exr(path)
    if a.ndim != 3 or a.shape[-1] < 3:
        raise L.IrisError(f"{path}: three colour channels expected")
    return np.ascontiguousarray(a[..., :3], dtype=np.float32)


class ValidationSet:
    """The validation views of a scene, resident on the device: per view the camera, the photograph's 8-bit codes (V, H W, 3), the exposure and, for a
    synthetic scene, DiffCol and Emit (V, H W, 3) float32.  Every view's pixel-centre rays are traced ONCE, here (the geometry never changes): `positions`
    (V, H W, 3) and `valid` (V, H W) stay on the device, the rays do not.

    views, img_hw: as stage.load_views gives them; codes: (V, H, W, 3) uint8, array or tensor; exposure: (V,); diffcol, emit: (V, H, W, 3) float32 or None.
    scene: the Scene the rays are traced in; emitter: the emitter the validation images are rendered under (None: the caller passes one to write_images).
    stack: views per network call and kernel launch (default: as many as fit utils.render.CHUNK_SAMPLES positions, at least one)."""

    def __init__(self, views, img_hw, codes, exposure, scene, *, diffcol=None, emit=None, emitter=None, device=None, stack=None):
        from . import cameras
        from .path_tracing import ray_intersect
        from .render import CHUNK_SAMPLES
        self.views, self.img_hw = list(views), (int(img_hw[0]), int(img_hw[1]))
        H, W = self.img_hw
        V, hw = len(self.views), H * W
        if V < 1:
            raise L.IrisError("ValidationSet: no views")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise L.IrisError(f"ValidationSet: {dev}: the validation set lives on a HIP device (there is no CPU path)")
        self.device = dev = torch.device("cuda", L.device_index(dev))
        if (diffcol is None) != (emit is None):
            raise L.IrisError("ValidationSet: a synthetic scene's ground truth is both diffcol and emit")

        def stack_of(a, dtype, name):
            t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
            if t.dtype != dtype or t.numel() != V * hw * 3:
                raise L.IrisError(f"ValidationSet: {name}: expected {V} x {H} x {W} x 3 values of {dtype}, got {tuple(t.shape)} of {t.dtype}")
            return t.to(dev).reshape(V, hw, 3).contiguous()
        self.codes = stack_of(codes, torch.uint8, "codes")
        self.diffcol = None if diffcol is None else stack_of(diffcol, torch.float32, "diffcol")
        self.emit = None if emit is None else stack_of(emit, torch.float32, "emit")
        self.exposure = np.asarray(exposure, np.float32).reshape(-1)
        if self.exposure.shape[0] != V:
            raise L.IrisError(f"ValidationSet: {self.exposure.shape[0]} exposures for {V} views")
        self.scene, self.emitter = scene, emitter
        self.stack = max(1, CHUNK_SAMPLES // hw) if stack is None else max(1, int(stack))
        self.positions = torch.empty(V, hw, 3, device=dev)
        self.valid = torch.empty(V, hw, dtype=torch.bool, device=dev)
        for i, view in enumerate(self.views):
            o, d = cameras.view_rays(view, self.img_hw, dev)[:2]
            pos, _, _, _, valid = ray_intersect(scene, o, torch.nn.functional.normalize(d, dim=-1))           # (:465-467)
            self.positions[i], self.valid[i] = pos, valid

    def __len__(self):
        return len(self.views)

    @classmethod
    def load(cls, files, scene, device, emitter=None, stack=None):
        """validation_files' dict -> the set: the photographs decoded on the host and uploaded as 8-bit codes (a scannetpp photograph of another size is
        resized on the device, utils.resize.resize_u8, linear: as the training photographs), DiffCol and Emit as float32"""
        from .resize import resize_u8
        dev = torch.device(device)
        codes = []
        for p in files["photographs"]:
            c = torch.from_numpy(_rgb_codes(p)).to(dev)
            if tuple(c.shape[:2]) != tuple(files["img_hw"]):
                if not files["resize"]:
                    raise L.IrisError(f"{p}: the photograph is {c.shape[0]} x {c.shape[1]}, the validation views {files['img_hw'][0]} x {files['img_hw'][1]}")
                c = resize_u8(c, files["img_hw"], "linear")
            codes.append(c)
        diffcol = emit = None
        if files["synthetic"]:
            diffcol = np.stack([_rgb_exr(p) for p in files["diffcol"]])
            emit = np.stack([_rgb_exr(p) for p in files["emit"]])
        return cls(files["views"], files["img_hw"], torch.stack(codes), files["exposure"], scene, diffcol=diffcol, emit=emit, emitter=emitter, device=dev, stack=stack)

    @torch.no_grad()
    def per_view(self, material, scene=None):
        """-> kd_validation_loss's dict over ALL views ((V,) float64 device tensors): the network on a stack of views, one kd_validation_loss call per stack"""
        from .path_tracing import _mat_tensors
        if scene is not None and scene is not self.scene:
            raise L.IrisError("ValidationSet: the views were traced in another scene than the one passed to evaluate()")
        parts = []
        for v0 in range(0, len(self), self.stack):
            v1 = min(v0 + self.stack, len(self))
            n = (v1 - v0) * self.img_hw[0] * self.img_hw[1]
            albedo, _, metal = _mat_tensors(material(self.positions[v0:v1].reshape(n, 3)))
            if albedo.shape[0] != n or metal.shape[0] != n:
                raise L.IrisError(f"ValidationSet: the material network returned {albedo.shape[0]} / {metal.shape[0]} rows for {n} positions")
            truth = dict(codes=self.codes[v0:v1]) if self.diffcol is None else dict(gt=self.diffcol[v0:v1], emit=self.emit[v0:v1])
            parts.append(kd_validation_loss(albedo, metal, self.valid[v0:v1], img_hw=self.img_hw, **truth))
        return {k: torch.cat([p[k] for p in parts]) for k in ("S", "loss", "psnr")}

    def evaluate(self, scene, material):
        """-> {'val/loss', 'val/psnr'}: 0-d float64 device tensors, the mean over the views of the per-view loss and of the per-view psnr -- Lightning logs
        the mean of validation_step's per-batch values, and a batch is a view.  The means are torch's float64 sum of the (V,) per-view values on the
        device -- one reduction without atomics, its order fixed by V -- and one division: the same bits for the same parameters.  scene: the set's own
        (None), checked when given."""
        out = self.per_view(material, scene)
        n = torch.full((), float(len(self)), dtype=torch.float64, device=self.device)
        return {"val/loss": out["loss"].sum() / n, "val/psnr": out["psnr"].sum() / n}

    def write_images(self, folder, step, frame, material, model_crf, SPP, spp, emitter=None):
        """validation_images of view `frame` into `folder`, as {step:05d}_<name>.png -> the files' paths"""
        from . import cameras
        emitter = emitter if emitter is not None else self.emitter
        if emitter is None:
            raise L.IrisError("ValidationSet.write_images: no emitter to render the validation images under")
        if not 0 <= int(frame) < len(self):
            raise L.IrisError(f"ValidationSet.write_images: view {frame} of {len(self)}")
        rays = cameras.view_rays(self.views[int(frame)], self.img_hw, self.device, ray_diff=True)
        return validation_images(self.scene, emitter, material, model_crf, rays, self.img_hw, self.codes[int(frame)], float(self.exposure[int(frame)]), SPP, spp,
                                 folder, step)


@torch.no_grad()
def validation_images(scene, emitter_net, material_net, model_crf, rays, img_hw, codes, exposure, SPP, spp, folder, step, denoiser=None):
    """validation() (:339-444) for one view.  rays: the tuple (origins, directions, dxdu, dydv) of (H W, 3) float32 device tensors; codes: the photograph,
    (H W, 3) or (H, W, 3) uint8 on the device; exposure: the view's.  SPP // spp rounds of path_tracing_single, path_tracing(indir_depth=5) and
    validation_intrinsics; both radiance images / rounds through the denoiser (the project's a-trous filter, guided by the pixel-centre hits, where the
    reference has OptiX) and model_crf(., exposure); mask = (denoised L_train > 1) & (photograph > 0.99).  Writes
    <folder>/{step:05d}_{L_train,L_full,L_gt,mat_albedo,mat_roughness,mat_metallic,emission,mask}.png through ONE encode_frames_device call (the maps'
    `/ rounds` and the emission's `/ rounds / 20` are the encoder's divisors; roughness and metallic through the magma table) -> the eight paths."""
    from .denoise import Denoiser
    from .path_tracing import path_tracing, path_tracing_single, ray_intersect
    from .png import encode_frames_device
    H, W = int(img_hw[0]), int(img_hw[1])
    rays_x, rays_d, dxdu, dydv = (L.require_gpu(r, torch.float32, "rays").reshape(-1, 3) for r in rays)
    rays_d = torch.nn.functional.normalize(rays_d, dim=-1)                       # (:351)
    B, dev = rays_x.shape[0], rays_x.device
    if B != H * W:
        raise L.IrisError(f"validation_images: {B} rays for an image of {H} x {W}")
    codes = L.require_gpu(codes, torch.uint8, "codes").reshape(H, W, 3)
    rounds = int(SPP) // int(spp)
    if rounds < 1:
        raise L.IrisError(f"validation_images: SPP ({SPP}) // spp ({spp}) is zero: nothing would be rendered")
    L_train, L_full = torch.zeros(B, 3, device=dev), torch.zeros(B, 3, device=dev)
    maps = new_maps(B, dev)

    def pixels(L_round):      # (no path continues after the primary hit: the integrator returns the un-reduced samples, as the reference's does)
        L_round = L_round.detach()
        return L_round if L_round.shape[0] == B else L_round.reshape(B, int(spp), 3).mean(1)
    for _ in range(rounds):
        L_train += pixels(path_tracing_single(scene, emitter_net, material_net, rays_x, rays_d, dxdu, dydv, spp))
        L_full += pixels(path_tracing(scene, emitter_net, material_net, rays_x, rays_d, dxdu, dydv, spp, 5))
        validation_intrinsics(scene, emitter_net, material_net, rays_x, rays_d, dxdu, dydv, spp, out=maps)
    if denoiser is None:
        denoiser = Denoiser((W, H), dev)
    pos, nrm, _, _, valid = ray_intersect(scene, rays_x, rays_d)
    denoiser.set_guides(nrm, pos, valid)
    hdr_train, hdr_full = denoiser.denoise_maps([(L_train / rounds).reshape(H, W, 3), (L_full / rounds).reshape(H, W, 3)])
    ldr_train = model_crf(hdr_train.reshape(B, 3).contiguous(), exposure).detach().reshape(H, W, 3)
    ldr_full = model_crf(hdr_full.reshape(B, 3).contiguous(), exposure).detach().reshape(H, W, 3)
    mask = ((hdr_train > 1.0) & (codes.to(torch.float32) / 255.0 > 0.99)).to(torch.float32)                  # (:440-442)
    images = [ldr_train.contiguous(), ldr_full.contiguous(), codes, maps["albedo"].reshape(H, W, 3), maps["roughness"].reshape(H, W, 1),
              maps["metallic"].reshape(H, W, 1), maps["emission"].reshape(H, W, 3), mask]
    divisors = [1.0, 1.0, 1.0, float(rounds), float(rounds), float(rounds), float(rounds) * 20.0, 1.0]
    magma = [False, False, False, False, True, True, False, False]
    files = encode_frames_device(images, divisors=divisors, magma=magma)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for name, data in zip(IMAGE_NAMES, files):
        paths.append(os.path.join(folder, "{:0>5d}_{}.png".format(int(step), name)))
        with open(paths[-1], "wb") as fh:
            fh.write(data)
    return paths
