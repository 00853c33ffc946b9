"""Segmentation fusion (the reference's utils/fuse_segmentation.py:62-102; iris_amd/csrc/iris_labels.h): the per-view part segmentations of a scene made
consistent across views by a vote per triangle.

  vote_view        one view's pixels vote for their id at the triangle they see: ONE launch (ray, closest hit -- ray_intersect's, bit for bit -- and the
                   add), instead of ray_intersect + boolean mask + scatter_add_
  triangle_labels  per triangle the id with the most votes (the LOWER id among equal counts, as numpy's and torch-CPU's argmax), 0 without a vote
  label_view       a view painted from a per-triangle table: ONE launch, no atomics; with dtype=torch.uint8 and miss=-1 it is the hot path of the
                   reference's utils/dataset/scannetpp/render_semantic.py
  fuse             the loop python -m iris_amd.fuse_segmentation runs
Everything is an integer count or a copy: exact, and the same bits from run to run.  vote_view writes into the histogram it is given and returns None;
the other three return tensors they allocate."""
import ctypes as C

import torch

from .. import _lib as L
from .gbuffer import view_rays_args

_HIST_DTYPES = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())


def _check_hist(hist, name="hist"):
    if not isinstance(hist, torch.Tensor) or not hist.is_cuda:
        raise L.IrisError(f"{name}: expected a tensor on a HIP device (got {getattr(hist, 'device', type(hist))}); iris_amd has no CPU path")
    if hist.dtype not in _HIST_DTYPES or hist.dim() != 2 or hist.shape[1] < 1:
        raise L.IrisError(f"{name}: expected (F, n_labels) int32 or uint32, got {tuple(hist.shape)} {hist.dtype}")
    if not hist.is_contiguous():
        raise L.IrisError(f"{name}: must be contiguous (it is read and written in place)")
    if hist.numel() >= 1 << 62:
        raise L.IrisError(f"{name}: too large")
    return hist


def vote_view(scene, hist, labels, *, camera=None, img_hw=None, rays=None):
    """hist[tri, id] += 1 for every pixel whose ray hits triangle tri and whose id satisfies 1 <= id < n_labels.  Ids that are 0, negative, NaN or
    >= n_labels are dropped, and so are misses; column 0 is never written.

      hist      (F, n_labels) int32 or uint32 (counts are unsigned 32-bit either way), F the scene's triangle count, contiguous, on the device, written in place
      labels    the pixels' ids, (N,) or (H, W), float32 (truncated toward zero, as .long()) or uint8, on the device
      rays      camera = a view dict of utils/cameras.py with img_hw = (H, W); or rays = an (N, 6+) float32 tensor [origin, direction, ...] read in place
    Returns None; nothing is allocated and nothing comes back to the host."""
    hist = _check_hist(hist)
    if hist.shape[0] != scene.n_triangles:
        raise L.IrisError(f"hist: {hist.shape[0]} rows for a scene of {scene.n_triangles} triangles")
    a, keep = L.LabelViewArgs(), []
    n, device = view_rays_args("vote_view", a.rays, keep, scene, camera, img_hw, rays)
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.float32, torch.uint8):
        raise L.IrisError("labels: expected a float32 or uint8 tensor")
    labels = L.require_gpu(labels, labels.dtype, "labels")
    if labels.numel() != n:
        raise L.IrisError(f"labels: {tuple(labels.shape)} for {n} rays")
    if hist.device != device or labels.device != device:
        raise L.IrisError(f"vote_view: hist on {hist.device}, labels on {labels.device}, the rays on {device}")
    a.n_tri, a.ids, a.ids_is_u8, a.hist, a.n_labels = hist.shape[0], labels.data_ptr(), int(labels.dtype == torch.uint8), hist.data_ptr(), hist.shape[1]
    with torch.cuda.device(device):
        L.check(L.lib().iris_label_vote(scene.handle, C.byref(a), L.stream()))


def triangle_labels(hist):
    """-> (F,) int32: per row of hist (F, n_labels) the column in [1, n_labels) with the highest count (unsigned), the lower column among equal counts,
    0 where no such column has a vote: 1 + argmax(hist[:, 1:], 1), zeroed where that maximum is 0."""
    hist = _check_hist(hist)
    out = torch.empty(hist.shape[0], dtype=torch.int32, device=hist.device)
    with torch.cuda.device(hist.device):
        L.check(L.lib().iris_label_argmax(L.ptr(hist), hist.shape[0], hist.shape[1], L.ptr(out), L.stream()))
    return out


def label_view(scene, table, *, camera=None, img_hw=None, rays=None, miss=0, dtype=torch.float32):
    """-> (N,) tensor of dtype float32 or uint8: table[tri] where the pixel's ray hits triangle tri, `miss` where it hits nothing.  uint8 keeps the value's
    low byte (miss=-1 -> 255), as numpy's astype(uint8).  table: (F,) int32 on the device, F the scene's triangle count."""
    table = L.require_gpu(table, torch.int32, "table")
    if table.dim() != 1 or table.shape[0] != scene.n_triangles:
        raise L.IrisError(f"table: expected ({scene.n_triangles},) -- one entry per triangle --, got {tuple(table.shape)}")
    if dtype not in (torch.float32, torch.uint8):
        raise L.IrisError(f"label_view: dtype {dtype}: float32 or uint8")
    if not -(1 << 31) <= int(miss) < (1 << 31):
        raise L.IrisError(f"label_view: miss={miss} is not a 32-bit integer")
    a, keep = L.LabelViewArgs(), [table]
    n, device = view_rays_args("label_view", a.rays, keep, scene, camera, img_hw, rays)
    if table.device != device:
        raise L.IrisError(f"label_view: table on {table.device}, the rays on {device}")
    out = torch.empty(n, dtype=dtype, device=device)
    a.n_tri, a.table, a.out, a.out_is_u8, a.miss_value = table.shape[0], table.data_ptr(), out.data_ptr(), int(dtype == torch.uint8), int(miss)
    with torch.cuda.device(device):
        L.check(L.lib().iris_label_view(scene.handle, C.byref(a), L.stream()))
    return out


def fuse(scene, views, img_hw, label_maps, n_labels):
    """The whole fusion: a zeroed (F, n_labels) histogram, one vote_view per view, triangle_labels, one label_view per view.
    views: view dicts of utils/cameras.py; label_maps: one (H, W) or (H*W,) float32 / uint8 device tensor per view; n_labels: the histogram's row width
    (ids 1 .. n_labels - 1 can win).  -> (tri_label (F,) int32, [one (H*W,) float32 map per view]).  No host synchronisation inside the loops."""
    if len(views) != len(label_maps):
        raise L.IrisError(f"fuse: {len(views)} views, {len(label_maps)} label maps")
    if int(n_labels) < 1:
        raise L.IrisError(f"fuse: n_labels = {n_labels}")
    hist = torch.zeros(scene.n_triangles, int(n_labels), dtype=torch.int32, device=scene.device)
    for view, labels in zip(views, label_maps):
        vote_view(scene, hist, labels, camera=view, img_hw=img_hw)
    tri_label = triangle_labels(hist)
    return tri_label, [label_view(scene, tri_label, camera=view, img_hw=img_hw) for view in views]
