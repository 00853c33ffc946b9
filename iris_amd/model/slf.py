"""VoxelSLF: sparse voxel radiance cache (reference: model/slf.py:16-70)."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L


class VoxelSLF(nn.Module):
    """voxel grid based surface light field; same constructor, buffers and state_dict keys as the reference."""

    def __init__(self, mask, voxel_min, voxel_max):
        super().__init__()
        H = mask.shape[0]
        self.H = H
        self.voxel_min = float(voxel_min)
        self.voxel_max = float(voxel_max)
        # (the buffers are built where the mask lives: a mask counted on the GPU -- slf_bake -- never visits the host; the reference builds on the CPU)
        mask = torch.as_tensor(mask)
        dev = mask.device
        kk, jj, ii = torch.where(mask)
        inds = -torch.ones(H, H, H, dtype=torch.long, device=dev)
        inds[kk, jj, ii] = torch.arange(len(ii), device=dev)
        self.register_buffer("inds", inds)
        self.register_buffer("radiance", torch.zeros(len(ii), 3, device=dev))
        self.register_buffer("count", torch.zeros(len(ii), dtype=torch.long, device=dev))
        self._native = L.Native()

    # -- device handle ---------------------------------------------------------------------------------
    def refresh(self):
        """Drop the device-side tables; they are rebuilt from the buffers at the next lookup."""
        self._native.free()

    def handle(self, device, need_radiance=True):
        """Device-side tables (int32 index grid + padded radiance rows).  They follow the module (L.tensor_key): the tables are rebuilt when `inds`
        changed since the upload (load_state_dict, in-place edits, rebinding, .to()), and the radiance rows alone are re-uploaded when only
        `radiance` did (scatter_add, mean pooling) -- lazily, the next time a lookup needs them."""
        # the device ordinal resolved ONCE ('cuda' without an index = torch's current device): the same ordinal decides whether the handle is for this device,
        # whether the tensors are already there, which device torch makes current around the call, and which device the C side creates the tables on
        idx = L.device_index(device)
        n = self._native
        if n.ptr is None or n.device != idx or not n.keys[0].fresh(self.inds):
            n.free()
            h = C.c_void_p()
            on_dev = lambda t: t.is_cuda and t.device.index == idx
            if on_dev(self.inds) and on_dev(self.radiance):
                inds = self.inds.detach().to(torch.int64).contiguous()
                rad = self.radiance.detach().to(torch.float32).contiguous().reshape(-1, 3)
                with torch.cuda.device(idx):
                    L.check(L.lib().iris_slf_create_dev(L.ptr(inds), self.H, L.ptr(rad), rad.shape[0], self.voxel_min, self.voxel_max, idx, C.byref(h), L.stream()))
            else:
                inds = np.ascontiguousarray(self.inds.detach().cpu().numpy(), dtype=np.int64)
                rad = L.host_f32(self.radiance).reshape(-1, 3)
                L.check(L.lib().iris_slf_create(inds.ctypes.data_as(C.c_void_p), self.H, rad.ctypes.data_as(C.c_void_p), rad.shape[0],
                                                self.voxel_min, self.voxel_max, idx, C.byref(h)))
            n = self._native = L.Native(h, L.lib().iris_slf_destroy, idx, (L.tensor_key(self.inds), L.tensor_key(self.radiance)))
        elif need_radiance and not n.keys[1].fresh(self.radiance):
            rr = self.radiance.detach().to(device=torch.device("cuda", idx), dtype=torch.float32).contiguous()
            with torch.cuda.device(idx):
                L.check(L.lib().iris_slf_set_radiance(n.ptr, L.ptr(rr), rr.shape[0], L.stream()))
            n.keys[1] = L.tensor_key(self.radiance)
        return n.ptr

    # -- reference API ---------------------------------------------------------------------------------
    def _lookup(self, x, want_idx, want_rgb):
        x = L.require_gpu(x, torch.float32, "x").reshape(-1, 3)
        B = x.shape[0]
        idx = torch.empty(B, device=x.device, dtype=torch.int64) if want_idx else None
        rgb = torch.empty(B, 3, device=x.device, dtype=torch.float32) if want_rgb else None
        with torch.cuda.device(x.device):
            L.check(L.lib().iris_slf_lookup(self.handle(x.device), L.ptr(x), B, L.ptr(idx), L.ptr(rgb), L.stream()))
        return idx, rgb

    def spatial_idx(self, x):
        """voxel entry index for Bx3 positions, -1 = empty (model/slf.py:41-54)"""
        return self._lookup(x, True, False)[0]

    def forward(self, x):
        """query surface light field; zero radiance in empty space (model/slf.py:63-70)"""
        return {"rgb": self._lookup(x, False, True)[1]}

    def scatter_add(self, x, radiance):
        """scatter add radiance into the voxel grid and count the entries (model/slf.py:56-61); the caller divides by
        count afterwards for mean pooling (slf_bake.py:138).  x, radiance: Bx3 on the GPU; the module's `radiance` / `count`
        buffers must live on the same device."""
        x = L.require_gpu(x, torch.float32, "x").reshape(-1, 3)
        radiance = L.require_gpu(radiance, torch.float32, "radiance").reshape(-1, 3)
        acc = L.require_gpu(self.radiance, torch.float32, "VoxelSLF.radiance buffer")
        cnt = L.require_gpu(self.count, torch.int64, "VoxelSLF.count buffer")
        with torch.cuda.device(x.device):
            L.check(L.lib().iris_slf_scatter_add(self.handle(x.device, need_radiance=False), L.ptr(x), L.ptr(radiance), x.shape[0], L.ptr(acc), L.ptr(cnt), L.stream()))
        # the kernel wrote the buffers behind torch's back: bump their version counters so that handle() re-uploads them
        self.radiance.add_(0); self.count.add_(0)
