"""8-bit image resize on the device: what the scannetpp layout's --res_scale does to a photograph, an albedo prior (linear) and a segment-id image (nearest).

    linear   the reference's open_png: cv2.resize(img, (Wt, Ht)) on the decoded 8-bit image -- OpenCV's INTER_LINEAR on its 8-bit fixed-point path, and its
             rounded 2 x 2 mean when both axes shrink by exactly 2
    nearest  the reference's sample_nearest: PIL's Image.NEAREST

The full-size image is uploaded once and the resized one is made where its consumer (pool_view, PixelSet) reads it: iris_resize_u8, one launch per 16
images (iris_amd/csrc/iris_resize.h).  The per-axis tables come from the library (iris_resize_tables, a host function), are uploaded once and kept per
(mode, source samples, destination samples, device).  The contract is DESIGN.md 5c-15; tests/resize_ref.py restates it in numpy.  The call creates no native
object (the tables are torch tensors), so _lib.Native owns nothing here.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L

MODES = {"linear": 0, "nearest": 1}          # IRIS_RESIZE_LINEAR, IRIS_RESIZE_NEAREST (include/iris_hip.h)
_tables = {}                                 # (mode, ns, nd, device index) -> (ofs int32 (nd), coef int16 (nd, 2) or None) on that device


def axis_tables(mode, ns, nd):
    """-> (ofs (nd) int32, coef (nd, 2) int16 or None for nearest) of one axis on the HOST, as iris_resize_tables fills them; needs no device"""
    if mode not in MODES:
        raise L.IrisError(f"resize: mode {mode!r}: linear | nearest")
    ns, nd = int(ns), int(nd)
    ofs = np.zeros(max(nd, 0), np.int32)
    coef = np.zeros((max(nd, 0), 2), np.int16) if mode == "linear" else None
    L.check(L.lib().iris_resize_tables(MODES[mode], ns, nd, ofs.ctypes.data_as(C.c_void_p), None if coef is None else coef.ctypes.data_as(C.c_void_p)))
    return ofs, coef


def _device_tables(mode, ns, nd, device):
    key = (mode, int(ns), int(nd), L.device_index(device))
    if key not in _tables:
        ofs, coef = axis_tables(mode, ns, nd)
        _tables[key] = (torch.from_numpy(ofs).to(device), None if coef is None else torch.from_numpy(coef).to(device))
    return _tables[key]


def resize_u8(images, hw, mode="linear"):
    """images: a uint8 tensor on a HIP device, (H, W), (H, W, 3) or (N, H, W, 3), or a list of equal-size (H, W) / (H, W, 3) ones; hw: (Ht, Wt) -> the same
    rank (a list: a list) at hw.  The same size in gives the input back untouched.  IrisError on a CPU tensor, another dtype, a channel count other than 1
    or 3, or an unknown mode; nothing is launched then."""
    if mode not in MODES:
        raise L.IrisError(f"resize_u8: mode {mode!r}: linear | nearest")
    Ht, Wt = int(hw[0]), int(hw[1])
    is_list = isinstance(images, (list, tuple))
    pieces = list(images) if is_list else [images]
    if not pieces:
        raise L.IrisError("resize_u8: no image")
    pieces = [L.require_gpu(t, torch.uint8, f"resize_u8: image {i}") for i, t in enumerate(pieces)]
    first = pieces[0]
    if any(t.shape != first.shape or t.device != first.device for t in pieces):
        raise L.IrisError("resize_u8: the images of one call have one size and lie on one device")
    if first.dim() not in ((2, 3) if is_list else (2, 3, 4)):
        raise L.IrisError(f"resize_u8: expected (H, W), (H, W, 3){'' if is_list else ' or (N, H, W, 3)'}, got {tuple(first.shape)}")
    batched = first.dim() == 4
    channels = 1 if first.dim() == 2 else int(first.shape[-1])
    if channels not in (1, 3):
        raise L.IrisError(f"resize_u8: images have 1 or 3 channels, got {channels}")
    Hs, Ws = (int(s) for s in (first.shape[1:3] if batched else first.shape[:2]))
    if min(Hs, Ws, Ht, Wt) < 1 or max(Hs, Ws, Ht, Wt) > 65535:
        raise L.IrisError(f"resize_u8: {Hs} x {Ws} -> {Ht} x {Wt}: a side has 1..65535 pixels")
    if (Hs, Ws) == (Ht, Wt):
        return images
    n = int(first.shape[0]) if batched else len(pieces)
    if n == 0:
        raise L.IrisError("resize_u8: no image")
    tail = () if first.dim() == 2 else (channels,)
    dev = first.device
    out = torch.empty((n, Ht, Wt) + tail, dtype=torch.uint8, device=dev)
    block = Hs * Ws * channels
    ptrs = (C.c_void_p * n)(*([first.data_ptr() + i * block for i in range(n)] if batched else [t.data_ptr() for t in pieces]))
    half = mode == "linear" and Hs == 2 * Ht and Ws == 2 * Wt                   # the library takes the exact-2 path itself: no tables
    with torch.cuda.device(dev):
        (xofs, xcoef), (yofs, ycoef) = ((None, None), (None, None)) if half else (_device_tables(mode, Ws, Wt, dev), _device_tables(mode, Hs, Ht, dev))
        L.check(L.lib().iris_resize_u8(ptrs, n, Hs, Ws, channels, MODES[mode], L.ptr(xofs), L.ptr(xcoef), L.ptr(yofs), L.ptr(ycoef), L.ptr(out), Ht, Wt, L.stream()))
    if is_list:
        return list(out.unbind(0))
    return out if batched else out[0]
