"""Float64 restatement of the photometric step loss (iris_loss_photometric, include/iris_hip.h), for the tests.

    L = L_sum / n_calls,  rgb = crf(L, e),  d = rgb - gt
    loss = sum d^2 / (3 B),  psnr = -10 log10(max(loss, 1e-5)),  dL_sum = ((2 d) / (3 B)) * (slope e) / n_calls

`restatement` works wholly in float64 through tools/crf_restatement.py (the interpolation contract) and takes the gradient from autograd: it shares no line
with the kernel's closed form.  `from_pieces` is the yardstick of the GPU tests: the same formulas in float64 over the float32 `rgb` and `slope e` that
the existing entry points (EmorCRF.forward, iris_crf_bwd on a cotangent of ones) return, so that what is compared is this call's own arithmetic."""
import math

import numpy as np
import torch

from tools import crf_restatement as R


def _exposure(exposure, B):
    if torch.is_tensor(exposure):
        e = exposure.detach().double().reshape(-1)
        return e.reshape(B, 1) if e.numel() == B and B != 1 else e.reshape(1, 1)
    return float(exposure)


def psnr_of(loss):
    return -10.0 * math.log10(max(float(loss), 1e-5))


def restatement(L_sum, n_calls, table, exposure, gt):
    """-> (loss, psnr, dL_sum) as python floats and a (B, 3) float64 tensor; every input is converted to float64"""
    x = L_sum.detach().double().clone().requires_grad_(True)
    B = x.shape[0]
    rgb = R.forward(table.detach().double(), x / float(n_calls), _exposure(exposure, B))
    loss = ((rgb - gt.detach().double()) ** 2).sum() / (3.0 * B)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), psnr_of(loss.detach()), g


def closed_form(L_sum, n_calls, table, exposure, gt):
    """the gradient as the header states it, in float64: ((2 d) / (3 B)) * (slope e) / n_calls with the contract's slope, 0 where L e leaves [0, 1]"""
    x = L_sum.detach().double() / float(n_calls)
    B = x.shape[0]
    e = _exposure(exposure, B)
    tab = table.detach().double()
    xe = x * e
    q = torch.clip(xe, 0, 1)
    p = R.linspace(tab.shape[1], tab)
    out = torch.empty_like(x)
    for c in range(3):
        l, r, dl, dr, flat = R.segment(p, q[:, c])
        v = tab[c]
        rgb = (v[l] * dr + v[r] * dl) / (dl + dr)
        slope = torch.where(flat, torch.zeros_like(dl), (v[r] - v[l]) / (dl + dr))
        inside = (xe[:, c] >= 0) & (xe[:, c] <= 1)
        se = torch.where(inside, slope * (e if isinstance(e, float) else e.expand(B, 1)[:, 0]), torch.zeros_like(slope))
        out[:, c] = (2.0 * (rgb - gt.detach().double()[:, c])) / (3.0 * B) * se / float(n_calls)
    return out


def from_pieces(rgb32, gt32, slope_e32, n_calls):
    """rgb32, gt32, slope_e32: (B, 3) float32 arrays or tensors.  -> (loss64 of the float32 d, psnr of float32(loss64), dL_sum64)"""
    rgb, gt, se = (np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, np.float32) for t in (rgb32, gt32, slope_e32))
    B = rgb.shape[0]
    d = (rgb - gt).astype(np.float32).astype(np.float64)                  # the float32 difference, exactly
    loss = float((d * d).sum() / (3.0 * B))
    g = (2.0 * d) / (3.0 * B) * se.astype(np.float64) / float(n_calls)
    return loss, psnr_of(np.float32(loss)), g
