"""Image-quality metrics on the device: SSIM and PSNR of image stacks (reference: render.py:236-239, skimage.metrics).

The reference calls ``skimage.metrics.structural_similarity(gt, ldr, data_range=1, channel_axis=-1)`` and ``peak_signal_noise_ratio``.
skimage is not a dependency of this project: the contract is its defaults restated (uniform 7 x 7 window, K1 0.01, K2 0.03, sample
covariance, only windows fully inside the image), evaluated by one fused HIP kernel (iris_amd/csrc/iris_metrics.h) whose window moments are
taken of the window shifted by its own centre pixel -- skimage's E[x^2] - E[x]^2 in float32 loses 2e-4 of SSIM on a bright, nearly flat
pair.  Tests pin the kernel to a float64 restatement (tests/ssim_ref64.py) and the restatement to skimage's literal formula.
"""
import torch

from .. import _lib as L


def _as_stack(t, name):
    t = L.require_gpu(t, torch.float32, name)
    if t.dim() == 2:
        return t[None, :, :, None]
    if t.dim() == 3:
        return t[None]
    if t.dim() == 4:
        return t
    raise L.IrisError(f"image_metrics: {name} has shape {tuple(t.shape)}; expected (H,W), (H,W,C) or (N,H,W,C)")


def image_metrics(a, b, data_range=1.0, full=False):
    """a, b: GPU float32 tensors (H,W), (H,W,C) or (N,H,W,C) of equal shape, C 1 or 3, H and W >= 7.
    -> {'psnr': (N,) float64, 'ssim': (N,) float64, 'sums': (N,C,2) float64} on the device (+ 'ssim_map' (N,H-6,W-6,C) float32 with full=True):
    psnr = 10 log10(R^2 / mse) (inf at mse == 0), ssim = mean over the channels of the mean of S over the windows, both derived in float64 from 'sums', the
    kernel's double sums (per image and channel: squared error over the pixels, S over the windows; bitwise reproducible for a shape).  Nothing synchronises
    with the host.  No backward pass (the reference never trains on SSIM): an input that requires grad raises."""
    if tuple(getattr(a, "shape", ())) != tuple(getattr(b, "shape", ())):
        raise L.IrisError(f"image_metrics: a {tuple(getattr(a, 'shape', ()))} and b {tuple(getattr(b, 'shape', ()))} differ in shape")
    a, b = _as_stack(a, "a"), _as_stack(b, "b")
    if a.device != b.device:
        raise L.IrisError(f"image_metrics: a is on {a.device}, b on {b.device}")
    L.no_autograd("image_metrics", a, b)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    N, H, W, C = (int(s) for s in a.shape)
    R = float(data_range)
    lib = L.lib()
    need = int(lib.iris_image_metrics_workspace_bytes(N, H, W, C))
    if need == 0:
        raise L.IrisError(f"image_metrics: shape (N, H, W, C) = {(N, H, W, C)} is not supported: N >= 1, H >= 7, W >= 7, C 1 or 3")
    ws = torch.empty(need, dtype=torch.uint8, device=a.device)
    sums = torch.empty(N, C, 2, dtype=torch.float64, device=a.device)
    smap = torch.empty(N, H - 6, W - 6, C, dtype=torch.float32, device=a.device) if full else None
    with torch.cuda.device(a.device):
        L.check(lib.iris_image_metrics(L.ptr(a), L.ptr(b), N, H, W, C, R, L.ptr(sums), L.ptr(smap), L.ptr(ws), need, L.stream()))
    mse = sums[:, :, 0].sum(1) / float(H * W * C)
    out = {"psnr": 10.0 * torch.log10((R * R) / mse), "ssim": (sums[:, :, 1] / float((H - 6) * (W - 6))).mean(1), "sums": sums}
    if full:
        out["ssim_map"] = smap
    return out


def _single(a, b, data_range, key, who):
    m = image_metrics(a, b, data_range)[key]
    if m.numel() != 1:
        raise L.IrisError(f"{who}: one image expected, got a stack of {m.numel()} (use image_metrics)")
    return float(m.item())


def ssim(a, b, data_range=1.0):
    """SSIM of one image pair as a Python float (synchronises)."""
    return _single(a, b, data_range, "ssim", "ssim")


def psnr_device(a, b, data_range=1.0):
    """PSNR of one image pair as a Python float (synchronises); inf for identical images."""
    return _single(a, b, data_range, "psnr", "psnr_device")
