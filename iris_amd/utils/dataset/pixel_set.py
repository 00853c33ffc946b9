"""The trainers' training set resident in HBM: pixel batches in one launch (iris_amd/csrc/iris_batch.h).

Reference: ``Inv*DatasetLDR(pixel=True)`` (utils/dataset/real_ldr.py:334-427, synthetic_ldr.py, scannetpp/dataset.py) keeps one float row per training
pixel on the host -- 12 ray floats, segmentation, rgb, 3 albedo floats, exposure, 39 cached shading floats: 59 floats, 236 B per pixel -- and
``__getitem__`` slices a ``randperm`` of the rows; the trainer then traces the batch and filters eight tensors by ``valid`` in every step
(train_brdf_crf.py:165-190, train_emitter.py:166-174), each boolean index a host synchronisation.

Here the rays of a pixel are computed from its camera (96 B per VIEW), 8-bit images stay 8-bit (3 + 3 B per pixel, 4 B for the segment id), the
shading cache is the ``ShadingCache`` already in HBM, and ``iris_pixel_batch`` turns a list of global pixel ids ``view * H*W + y*W + x`` into the
reference's batch dict.  ``restrict_to_hits`` traces every view ONCE and keeps the ids of the pixels that hit the mesh: afterwards every batch is
all-valid and of a fixed size, and a step needs neither the per-step trace (with ``store_positions``) nor the ``valid`` filtering.  That is a
deliberate deviation from the reference, which draws from all pixels and drops the invalid ones in the step; without the call the
batches are the reference's and the caller filters.

    ps = PixelSet(views, img_hw, rgb=images_u8, segmentation=seg, int_albedo=albedo_u8, exposure=exposures, batch_size=8192, device="cuda")
    ps.attach_cache(cache)
    ps.restrict_to_hits(scene, store_positions=True)
    for epoch in ...:
        ps.resample()
        for i in range(len(ps)):
            batch = ps[i]           # rays, rgbs, segmentation, int_albedo, exposure, idx, positions: device tensors, no synchronisation
"""
import numpy as np
import torch
import torch.nn.functional as NF

from ... import _lib as L

CAM_FLOATS = 24          # iris_batch.h kCamFloats: K[9] | c2w[12] | focal | 2 pad


def batch_count(n, batch_size):
    """ceil(n / batch_size): the reference's ``batch_num`` (real_ldr.py:382)"""
    n, batch_size = int(n), int(batch_size)
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    return -(-n // batch_size)


def check_ids(ids, n_pixels):
    """ids as a 1-d int64 tensor (where it lives), after checking ON THE HOST that every id lies in [0, n_pixels): ValueError otherwise.
    (A device tensor costs one synchronisation: its minimum and maximum come to the host.)"""
    t = torch.from_numpy(np.ascontiguousarray(ids)) if isinstance(ids, np.ndarray) else ids
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype not in (torch.int64, torch.int32) or t.dim() != 1:
        raise ValueError("ids: expected a 1-d integer array or tensor")
    t = t.to(torch.int64)
    if t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= n_pixels:
            raise ValueError(f"ids: values in [{lo}, {hi}] leave the pixel range [0, {n_pixels})")
    return t


def check_cache_length(cache, n_pixels):
    """the cache's row index is the global pixel id (views in the same order): its length must be the set's"""
    if len(cache) != n_pixels:
        raise ValueError(f"the cache has {len(cache)} rows, the pixel set {n_pixels} pixels (same views, same order?)")


def camera_table(cameras, synthetic):
    """(V,24) float32 host table of the views of utils/cameras.py's loaders ({'kind', 'K' | 'focal', 'c2w'})"""
    if len(cameras) == 0:
        raise ValueError("cameras: no views")
    table = np.zeros((len(cameras), CAM_FLOATS), np.float32)
    for v, cam in enumerate(cameras):
        if (cam["kind"] == "synthetic") != bool(synthetic):
            raise ValueError(f"view {v} is of kind {cam['kind']!r} but synthetic={bool(synthetic)}")
        table[v, 9:21] = L.host_f32(cam["c2w"]).reshape(-1)[:12]
        if synthetic:
            table[v, 21] = np.float32(cam["focal"])
        else:
            table[v, :9] = L.host_f32(cam["K"]).reshape(9)
            table[v, 21] = 1.0
    return table


def _pieces(x, name):
    """x (one array / tensor, or one per view) as a list of tensors: numpy arrays are host data to be uploaded, torch tensors must be on a HIP device"""
    out = []
    for p in (x if isinstance(x, (list, tuple)) else [x]):
        if isinstance(p, np.ndarray):
            p = torch.from_numpy(np.ascontiguousarray(p))
        elif not isinstance(p, torch.Tensor) or not p.is_cuda:
            raise L.IrisError(f"{name}: expected numpy arrays or tensors on a HIP device (got {getattr(p, 'device', type(p))}); iris_amd has no CPU path")
        out.append(p)
    return out


def _store(x, name, cols, n, dtypes, device):
    """the per-pixel store (n, cols) on the device, its dtype one of `dtypes` kept as given"""
    pieces = _pieces(x, name)
    if any(p.dtype != pieces[0].dtype for p in pieces) or pieces[0].dtype not in dtypes:
        raise ValueError(f"{name}: expected dtype {' or '.join(str(d) for d in dtypes)}, got {sorted({str(p.dtype) for p in pieces})}")
    if sum(p.numel() for p in pieces) != n * cols:
        raise ValueError(f"{name}: expected {n} x {cols} values over all views, got {sum(p.numel() for p in pieces)}")
    return lambda: torch.cat([p.reshape(-1).to(device) for p in pieces]).reshape(n, cols).contiguous()


class PixelSet:
    """The reference loader's call surface -- ``resample()``, ``len``, ``[i]`` -> batch dict -- on device-resident stores.

    cameras: the views of iris_amd/utils/cameras.py's loaders; img_hw: (H, W); rgb / int_albedo: (N,3) uint8 (decoded as ``np.float32(u / 255.0)``, what
    open_png and the albedo loader produce) or float32 (stored and returned as given, e.g. gamma-linearised images), N = V*H*W, one array or tensor or
    one per view; segmentation: (N) integer ids (int32 on the device, int64 in the batch); exposure: (V) per view.  numpy arrays are uploaded, tensors
    must already be on a HIP device.  ray_diff: the loaders' ``self.ray_diff = True`` (un-normalised directions and differentials)."""

    def __init__(self, cameras, img_hw, rgb, segmentation=None, int_albedo=None, exposure=None, *, synthetic=False, batch_size, device, ray_diff=True,
                 materialise_cache=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.IrisError(f"{device}: PixelSet needs a HIP device (there is no CPU fallback)")
        self.H, self.W = int(img_hw[0]), int(img_hw[1])
        if self.H <= 0 or self.W <= 0:
            raise ValueError("img_hw must be positive")
        self.batch_size = int(batch_size)
        batch_count(0, self.batch_size)
        self.synthetic, self.ray_diff, self.materialise_cache = bool(synthetic), bool(ray_diff), bool(materialise_cache)
        self.views = list(cameras)
        table = camera_table(self.views, self.synthetic)
        self.n_views = table.shape[0]
        self.n_pixels = n = self.n_views * self.H * self.W
        u8f = (torch.uint8, torch.float32)
        ints = (torch.int32, torch.int64, torch.uint8, torch.int16, torch.float32)       # (the reference reads the ids from an EXR channel as floats)
        up = dict(rgb=_store(rgb, "rgb", 3, n, u8f, device))
        if int_albedo is not None:
            up["int_albedo"] = _store(int_albedo, "int_albedo", 3, n, u8f, device)
        if segmentation is not None:
            up["segmentation"] = _store(segmentation, "segmentation", 1, n, ints, device)
        if exposure is not None:
            up["exposure"] = _store(exposure, "exposure", 1, self.n_views, (torch.float32, torch.float64), device)
        # everything above ran on the host; from here on the device is touched
        self.device = torch.device("cuda", L.device_index(device))
        self.cameras = torch.from_numpy(table).to(self.device)
        self.rgb = up["rgb"]()
        self.int_albedo = up["int_albedo"]() if "int_albedo" in up else None
        self.segmentation = up["segmentation"]().reshape(n).to(torch.int32) if "segmentation" in up else None
        self.exposure = up["exposure"]().reshape(self.n_views).to(torch.float32) if "exposure" in up else None
        self.positions = None          # (N,3) hit positions, restrict_to_hits(store_positions=True)
        self.kept = None               # sorted ids of the pixels that hit the mesh, restrict_to_hits
        self.cache = None
        self.resample()

    # ---- what the batches are drawn from
    def attach_cache(self, cache):
        """cache: the ShadingCache of the same views in the same order: its row index is the global pixel id, so ``batch['idx']`` addresses both"""
        check_cache_length(cache, self.n_pixels)
        if cache.rows.device != self.device:
            raise L.IrisError(f"the cache lives on {cache.rows.device}, the pixel set on {self.device}")
        self.cache = cache

    def view_rays(self, v):
        """the whole-view rays of view v as the batches carry them: (o, d) or, with ray_diff, (o, d, dxdu, dydv)"""
        from . import real_ldr, synthetic_ldr
        cam = self.views[v]
        if self.synthetic:
            return synthetic_ldr.get_rays(synthetic_ldr.get_ray_directions(self.H, self.W, cam["focal"]), cam["c2w"],
                                          focal=cam["focal"] if self.ray_diff else None, device=self.device)
        return real_ldr.to_world(real_ldr.get_direction(cam["K"], (self.H, self.W)), cam["c2w"], self.ray_diff, device=self.device)

    def restrict_to_hits(self, scene, store_positions=False):
        """Trace every view once -- ``ray_intersect(scene, o, normalize(d))``, the trainers' first lines (train_brdf_crf.py:165-178) -- and keep the ids
        of the pixels that hit the mesh (one ``nonzero`` per view: construction time, not step time); with store_positions also the hit positions,
        12 B per pixel, returned as ``batch['positions']``.  Draws a new order over the kept ids.  Returns their number."""
        from ..path_tracing import ray_intersect
        hw = self.H * self.W
        kept, positions = [], torch.empty(self.n_pixels, 3, device=self.device, dtype=torch.float32) if store_positions else None
        for v in range(self.n_views):
            rays = self.view_rays(v)
            pos, _, _, _, valid = ray_intersect(scene, rays[0], NF.normalize(rays[1], dim=-1))
            kept.append(valid.nonzero().reshape(-1) + v * hw)
            if store_positions:
                positions[v * hw:(v + 1) * hw] = pos
        self.kept, self.positions = torch.cat(kept), positions
        self.resample()
        return self.kept.shape[0]

    def resample(self, generator=None):
        """a new random order of the kept ids (all pixels before restrict_to_hits): ``torch.randperm`` on the device (real_ldr.py:388-390)"""
        n = self.n_pixels if self.kept is None else self.kept.shape[0]
        perm = torch.randperm(n, device=self.device, generator=generator)
        self.order = perm if self.kept is None else self.kept[perm]

    def set_order(self, ids, check=True):
        """The order of the coming batches, given (tests, resume).  check: every id is bounded on the host first (ValueError); pass check=False only
        for ids that were bounded before, such as a saved ``order``: the kernel is never to see an id the host has not bounded."""
        if check:
            ids = check_ids(ids, self.n_pixels)
        elif not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError("ids: expected a 1-d int64 tensor")
        self.order = ids.to(self.device).contiguous()

    # ---- the batches
    def __len__(self):
        return batch_count(self.order.shape[0], self.batch_size)

    def gather(self, idx):
        """the batch of the pixels idx ((B) int64 on the device, bounded by the caller): the dict of __getitem__"""
        idx = L.require_gpu(idx, torch.int64, "idx")
        B, dev, f32 = idx.shape[0], self.device, torch.float32
        new = lambda store, *shape, dtype=f32: None if store is None else torch.empty(*shape, device=dev, dtype=dtype)
        rays = torch.empty(B, 12, device=dev, dtype=f32)
        rgbs, albedo = new(self.rgb, B, 3), new(self.int_albedo, B, 3)
        seg, exposure, positions = new(self.segmentation, B, dtype=torch.int64), new(self.exposure, B, 1), new(self.positions, B, 3)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_pixel_batch(L.ptr(idx), B, L.ptr(self.cameras), self.n_views, self.H, self.W, int(self.ray_diff), int(self.synthetic),
                                             L.ptr(self.rgb), int(self.rgb.dtype == torch.uint8), L.ptr(self.int_albedo),
                                             int(self.int_albedo is not None and self.int_albedo.dtype == torch.uint8), L.ptr(self.segmentation),
                                             L.ptr(self.positions), L.ptr(self.exposure), L.ptr(rays), L.ptr(rgbs), L.ptr(albedo), L.ptr(seg),
                                             L.ptr(exposure), L.ptr(positions), L.stream()))
        batch = dict(rays=rays, rgbs=rgbs, segmentation=seg, int_albedo=albedo, exposure=exposure, idx=idx)
        if positions is not None:
            batch["positions"] = positions
        if self.materialise_cache:
            if self.cache is None:
                raise L.IrisError("materialise_cache: no cache attached (attach_cache)")
            batch["diffuse"], batch["specular0"], batch["specular1"] = self.cache.gather(idx)
        return batch

    def __getitem__(self, i):
        """Batch i of the current order: the reference's dict (real_ldr.py:418-427) -- rays (B,12) = [o | d | dxdu | dydv], rgbs (B,3), segmentation (B)
        int64, int_albedo (B,3), exposure (B,1); None for a store that was not given -- plus idx (B) int64, the global pixel ids (``cache.shade(idx, ...)``),
        positions (B,3) when stored, and diffuse / specular0 / specular1 with materialise_cache.  The last batch is short.  Nothing here synchronises."""
        n = len(self)
        if not -n <= i < n:
            raise IndexError(i)
        i = i % n if n else 0
        return self.gather(self.order[i * self.batch_size:(i + 1) * self.batch_size])
