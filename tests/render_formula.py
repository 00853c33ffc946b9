"""The documented per-sample formula of iris_render_intrinsics (include/iris_hip.h, iris_amd/csrc/iris_render.h) in plain torch, in any dtype: what
tests/test_render.py holds the kernel to on synthetic inputs, and where the bound's `max |x|` comes from.  Shared by the GPU and the CPU test file."""
import math

import numpy as np
import torch

from conftest import golden

MAPS = (("kd", 3), ("a_prime", 3), ("roughness", 1), ("metallic", 1), ("emission", 3), ("slf", 3))
U = 2.0 ** -24


def fixture():
    g = golden("render_intrinsics.npz")
    return {k: g[k] for k in g.files}


def _normalize(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def voxel_rows(pos, inds, vmin, vmax):
    """the VoxelSLF row of every position, with the kernel's float32 coordinate arithmetic: int((p - vmin) / (vmax - vmin) * H) clamped"""
    H = inds.shape[0]
    p = pos.to(torch.float32)
    f = (p - np.float32(vmin)) / np.float32(vmax - vmin) * np.float32(H)
    c = torch.nan_to_num(f, nan=0.0, posinf=0.0).to(torch.int64).clamp(0, H - 1)
    return torch.as_tensor(inds).long()[c[:, 2], c[:, 1], c[:, 0]]


def sample_terms(dtype, pos, nrm, wo, e0, valid_next, albedo, rough, metal, u2, radiance, slf_inds, slf_radiance, vmin, vmax):
    """-> {map: (N, c)} per-sample terms x in `dtype`, and the keep mask.  Inputs: float32 / int tensors on the CPU."""
    T = lambda a: torch.as_tensor(a).to(dtype)
    n, o, alb, r, m, u = T(nrm), T(wo), T(albedo), T(rough).reshape(-1, 1), T(metal).reshape(-1, 1), T(u2)
    kd = alb * (1 - m)
    ks = 0.04 * (1 - m) + alb * m
    # get_normal_space / specular_sampler / sample_specular's weights (model/brdf.py:36-59, :112-136; utils/ops.py:12-30)
    z = torch.zeros_like(n[:, 0])
    t = torch.where((n[:, :1].abs() <= 0.1), torch.stack([z, -n[:, 2], n[:, 1]], -1), torch.stack([n[:, 2], z, -n[:, 0]], -1))
    t = _normalize(t)
    b = torch.cross(n, t, dim=-1)
    alpha = r * r
    c2 = (1 - u[:, :1]) / (u[:, :1] * (alpha * alpha - 1) + 1)
    theta, phi = torch.acos(torch.sqrt(c2).clamp(max=1)), 2 * math.pi * u[:, 1:2]
    l = _normalize(torch.cat([torch.sin(theta) * torch.cos(phi), torch.sin(theta) * torch.sin(phi), torch.cos(theta)], -1))
    wh = l[:, :1] * t + l[:, 1:2] * b + l[:, 2:3] * n
    wi = _normalize(2 * (o * wh).sum(-1, keepdim=True) * wh - o)
    h = _normalize(wi + o)
    NoL, NoV = (wi * n).sum(-1, keepdim=True).relu(), (o * n).sum(-1, keepdim=True).relu()
    VoH, NoH = (o * h).sum(-1, keepdim=True).relu(), (n * h).sum(-1, keepdim=True).relu()
    k = (r + 1) ** 2 / 8
    G = 1 / (NoL * (1 - k) + k) * (1 / (NoV * (1 - k) + k))
    x5 = (1 - VoH) ** 5
    fac = G * VoH * NoL / NoH.clamp_min(1e-4)
    a_prime = (1 - x5) * fac * ks + x5 * fac + kd
    e0 = torch.as_tensor(e0).long()
    rad = T(radiance)
    emission = torch.where((e0 >= 0)[:, None], rad[e0.clamp_min(0)], torch.zeros_like(alb))
    vis = torch.as_tensor(valid_next).bool() | (e0 >= 0)
    keep = vis & ((emission[:, 0] + emission[:, 1]) + emission[:, 2] == 0)
    rows = voxel_rows(torch.as_tensor(pos), slf_inds, vmin, vmax)
    slf = torch.where((rows >= 0)[:, None], T(slf_radiance)[rows.clamp_min(0)], torch.zeros_like(alb))
    one, zero, K = torch.ones_like(alb), torch.zeros_like(r), keep[:, None]
    return {"kd": torch.where(K, kd, one), "a_prime": torch.where(K, a_prime, one), "roughness": torch.where(K, r, one[:, :1]), "metallic": torch.where(K, m, zero),
            "emission": emission, "slf": slf}, keep


def pixel_means(x, spp):
    """(N, c) per-sample terms -> (B, c): the sequential sum over s times 1 / spp, in x's dtype"""
    B = x.shape[0] // spp
    x = x.reshape(B, spp, -1)
    acc = torch.zeros_like(x[:, 0])
    for s in range(spp):
        acc = acc + x[:, s]
    return acc * (torch.ones((), dtype=x.dtype) / spp)


def bound(d32, spp, xmax):
    """max(8 d32, spp 2^-24 max|x|): tests/test_propagation.py's and tests/test_crf.py's rule"""
    return max(8 * d32, spp * U * xmax)
