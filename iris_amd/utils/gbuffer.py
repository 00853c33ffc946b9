"""Pooling primitives of the stages that produce the bake's inputs: the voxel occupancy
histogram of slf_bake.py:96-114 and the per-triangle radiance sums of extract_emitter_ldr.py:82-98.  (VoxelSLF.scatter_add is a
method of iris_amd.model.slf.VoxelSLF.)  Atomic accumulation on the GPU; float sums agree with the reference's sequential
scatter_add up to summation order.  pool_view is what the pre-bake stages (iris_amd/slf_bake.py) call: a view's ray generation, closest hit, radiance
decode and any of these sinks as ONE launch; the two primitives below stay for callers that hold positions or triangle indices already."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L


def view_rays_args(fn, a, keep, scene, camera, img_hw, rays):
    """Fills a (an L.ViewRays: the `rays` member of the argument structure of fn -- pool_view, vote_view, label_view) from camera= and img_hw=, or from
    rays=; what a points at is appended to keep, to stay alive until the call returns -> (number of rays, the device the call runs under)"""
    if (camera is None) == (rays is None):
        raise L.IrisError(f"{fn}: pass either camera= (with img_hw=) or rays=")
    if camera is not None:
        from .dataset.pixel_set import camera_table
        if img_hw is None:
            raise L.IrisError(f"{fn}: camera= needs img_hw=(H, W)")
        synthetic = camera["kind"] == "synthetic"
        row = np.ascontiguousarray(camera_table([camera], synthetic)[0])
        keep.append(row)
        a.camera, a.H, a.W, a.synthetic = row.ctypes.data_as(C.c_void_p), int(img_hw[0]), int(img_hw[1]), int(synthetic)
        return a.H * a.W, scene.device
    rays = L.require_gpu(rays, torch.float32, "rays")
    if rays.dim() < 2 or rays.shape[-1] < 6:
        raise L.IrisError(f"rays: expected (N, 6) [origin, direction], got {tuple(rays.shape)}")
    rays = rays.reshape(-1, rays.shape[-1])              # (rows wider than 6 -- a dataset's ray differentials -- are stepped over)
    keep.append(rays)
    a.rays_o, a.rays_d, a.ray_stride, a.B = rays.data_ptr(), rays.data_ptr() + 12, rays.shape[1], rays.shape[0]
    return rays.shape[0], rays.device


def pool_view(scene, *, camera=None, img_hw=None, rays=None, image=None, crf_tables=None, exposure=1.0, bounds=None, hist=None, voxel_range=None, vslf=None,
              tri_sum=None, tri_count=None):
    """One view's primary hits pooled where they land, in ONE launch (iris_amd/csrc/iris_prebake.h): per pixel the ray, its closest hit (ray_intersect's,
    bit for bit) and, for a hit, every sink that was given.  Nothing is allocated and nothing comes back to the host; the call writes into the tensors
    it was given and returns None.

      rays      camera = a view dict of utils/cameras.py with img_hw = (H, W): the pixel-centre rays of cameras.view_rays; or rays = an (N,6) float32
                tensor [origin, direction] on the device, read in place
      image     the radiance of every ray, (N,3) or (H,W,3), uint8 (decoded as u / 255) or float32, on the device; needed by the two pools only
      crf_tables, exposure   (grid, inverse table) of an EmorCRF -- model.grid, model.get_inv_crf() --: the radiance is model.inverse(image, exposure);
                exposure as EmorCRF.inverse takes it (a number, one value, or one per ray)
      bounds    (2,) float32 [min, max], updated with the min / max over the coordinates of the hit positions (exact)
      hist      (H,H,H) float32 occupancy [z,y,x] of the grid voxel_range = (voxel_min, voxel_max): voxel_histogram of the hit positions
      vslf      a VoxelSLF with its buffers on the device: VoxelSLF.scatter_add(hit positions, radiance)
      tri_sum, tri_count   (F,3) and (F,) float32: scatter_add_rows(radiance, hit triangle)
    With no sink the launch only traces."""
    for name, t in (("bounds", bounds), ("hist", hist), ("tri_sum", tri_sum), ("tri_count", tri_count)):
        if isinstance(t, torch.Tensor) and not t.is_contiguous():      # (require_gpu copies what is not contiguous: a sink must be written in place)
            raise L.IrisError(f"{name}: a sink must be contiguous")
    a = L.PoolViewArgs()
    keep = []                                             # what the struct points at, alive until the call returns
    n, device = view_rays_args("pool_view", a.rays, keep, scene, camera, img_hw, rays)
    if vslf is not None or tri_sum is not None:
        if image is None:
            raise L.IrisError("pool_view: the voxel and triangle pools need image=")
        if not isinstance(image, torch.Tensor) or image.dtype not in (torch.uint8, torch.float32):
            raise L.IrisError("image: expected a uint8 or float32 tensor")
        image = L.require_gpu(image, image.dtype, "image")
        if image.numel() != 3 * n:
            raise L.IrisError(f"image: {tuple(image.shape)} for {n} rays")
        keep.append(image)
        a.rgb, a.rgb_is_u8 = image.data_ptr(), int(image.dtype == torch.uint8)
        if crf_tables is not None:
            from ..model.crf import _check_tables, _exposure_args
            grid, inv = crf_tables
            inv, grid = _check_tables(inv, grid)
            e, ne, ev = _exposure_args(exposure, n, device)
            keep += [grid, inv, e]
            a.crf_grid, a.crf_inv_table, a.crf_n = grid.data_ptr(), inv.data_ptr(), inv.shape[1]
            a.exposure, a.n_exposure, a.exposure_value = (e.data_ptr() if e is not None else None), ne, ev
    if bounds is not None:
        bounds = L.require_gpu(bounds, torch.float32, "bounds")
        if bounds.numel() != 2:
            raise L.IrisError("bounds: expected 2 values [min, max]")
        a.bounds = bounds.data_ptr()
    if hist is not None:
        hist = L.require_gpu(hist, torch.float32, "hist")
        if hist.dim() != 3 or len(set(hist.shape)) != 1 or voxel_range is None:
            raise L.IrisError("hist: expected (H, H, H) and voxel_range=(voxel_min, voxel_max)")
        a.hist, a.hist_H, a.voxel_min, a.voxel_max = hist.data_ptr(), hist.shape[0], float(voxel_range[0]), float(voxel_range[1])
    if vslf is not None:
        acc = L.require_gpu(vslf.radiance, torch.float32, "VoxelSLF.radiance buffer")
        cnt = L.require_gpu(vslf.count, torch.int64, "VoxelSLF.count buffer")
        a.slf, a.slf_acc, a.slf_count = vslf.handle(device, need_radiance=False), acc.data_ptr(), cnt.data_ptr()
    if tri_sum is not None:
        tri_sum = L.require_gpu(tri_sum, torch.float32, "tri_sum")
        if tri_sum.dim() != 2 or tri_sum.shape[1] != 3:
            raise L.IrisError(f"tri_sum: expected (F, 3), got {tuple(tri_sum.shape)}")
        a.tri_sum, a.n_tri = tri_sum.data_ptr(), tri_sum.shape[0]
        if tri_count is not None:
            tri_count = L.require_gpu(tri_count, torch.float32, "tri_count")
            if tri_count.numel() != tri_sum.shape[0]:
                raise L.IrisError("tri_count: expected one value per row of tri_sum")
            a.tri_count = tri_count.data_ptr()
    with torch.cuda.device(device):
        L.check(L.lib().iris_pool_view(scene.handle, C.byref(a), L.stream()))
    if vslf is not None:                                  # the kernel wrote the buffers behind torch's back (as VoxelSLF.scatter_add)
        vslf.radiance.add_(0); vslf.count.add_(0)


def voxel_histogram(position, voxel_min, voxel_max, res_spatial, hist=None):
    """SpatialHist of slf_bake.py:104-110: counts of positions per voxel, shape (H,H,H) indexed [z,y,x]; pass `hist` to
    accumulate over views."""
    position = L.require_gpu(position, torch.float32, "position").reshape(-1, 3)
    H = int(res_spatial)
    if hist is None:
        hist = torch.zeros(H, H, H, device=position.device, dtype=torch.float32)
    hist = L.require_gpu(hist, torch.float32, "hist")
    with torch.cuda.device(position.device):
        L.check(L.lib().iris_voxel_histogram(L.ptr(position), position.shape[0], float(voxel_min), float(voxel_max), H, L.ptr(hist), L.stream()))
    return hist


def scatter_add_rows(values, index, out, count=None):
    """out[index[i]] += values[i] (rows of 3), count[index[i]] += 1: torch_scatter.scatter(values, index, 0, out, reduce='sum')
    of extract_emitter_ldr.py:90-95."""
    values = L.require_gpu(values, torch.float32, "values").reshape(-1, 3)
    index = L.require_gpu(index, torch.int64, "index").reshape(-1)
    out = L.require_gpu(out, torch.float32, "out")
    if count is not None:
        count = L.require_gpu(count, torch.float32, "count")
    with torch.cuda.device(values.device):
        L.check(L.lib().iris_scatter_add_rows(L.ptr(values), L.ptr(index), values.shape[0], out.shape[0], L.ptr(out), L.ptr(count), L.stream()))
    return out, count
