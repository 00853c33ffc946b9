"""The fetch contract of the texture material (iris_amd/csrc/iris_texmat.h) in numpy, no project import.

The contract states the texel COORDINATES in float32, in one order: they decide which four texels are read and the two weights, and a float64 coordinate
would name other weights (at W = 256 a last-bit difference in u moves fx by 3e-5).  They are therefore computed in float32 here too, operation for operation
(IEEE: numpy's float32 and the device agree).  Everything the bound of tests/test_texture_material.py is about -- byte / 255 and the three-deep lerps -- is in
float64."""
import numpy as np

ROUGHNESS_MIN = 0.02
F32 = np.float32


def texel_coords(tri, bary, ft, vt, H, W):
    """-> (x0, x1, fx, y0, y1, fy): the four taps' columns and rows (int64) and the weights (float32, exactly the contract's)"""
    ft, vt = np.asarray(ft, np.int64), np.asarray(vt, F32)
    b1, b2 = np.asarray(bary, F32)[:, 0], np.asarray(bary, F32)[:, 1]
    b0 = (F32(1.0) - b1) - b2
    i0, i1, i2 = ft[tri, 0], ft[tri, 1], ft[tri, 2]
    u = ((b0 * vt[i0, 0]) + (b1 * vt[i1, 0])) + (b2 * vt[i2, 0])
    v = ((b0 * vt[i0, 1]) + (b1 * vt[i1, 1])) + (b2 * vt[i2, 1])
    x = np.clip(u * F32(W) - F32(0.5), F32(0.0), F32(W - 1)).astype(F32)
    y = np.clip(v * F32(H) - F32(0.5), F32(0.0), F32(H - 1)).astype(F32)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0).astype(F32), (y - y0).astype(F32)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    return x0, np.minimum(x0 + 1, W - 1), fx, y0, np.minimum(y0 + 1, H - 1), fy


def fetch(tri, bary, ft, vt, albedo_img, rm_img):
    """tri (B,) int, bary (B, 2), ft (F, 3), vt (N, 2), the two (H, W, 3) uint8 images -> {'albedo' (B, 3), 'roughness' (B, 1), 'metallic' (B, 1)} float64.
    tri < 0: zeros, roughness 0.02."""
    tri = np.asarray(tri, np.int64).reshape(-1)
    albedo_img, rm_img = np.asarray(albedo_img), np.asarray(rm_img)
    H, W = albedo_img.shape[:2]
    ok = tri >= 0
    t = np.where(ok, tri, 0)
    x0, x1, fx, y0, y1, fy = texel_coords(t, bary, ft, vt, H, W)
    fx, fy = fx.astype(np.float64)[:, None], fy.astype(np.float64)[:, None]

    def bilinear(img):
        a = img.astype(np.float64) / 255.0
        t00, t01, t10, t11 = a[y0, x0], a[y0, x1], a[y1, x0], a[y1, x1]
        top, bot = t00 + fx * (t01 - t00), t10 + fx * (t11 - t10)
        return top + fy * (bot - top)
    alb, rm = bilinear(albedo_img), bilinear(rm_img)
    rough = np.maximum(rm[:, :1], ROUGHNESS_MIN)
    z = ~ok[:, None]
    return {"albedo": np.where(z, 0.0, alb), "roughness": np.where(z, ROUGHNESS_MIN, rough), "metallic": np.where(z, 0.0, rm[:, 1:2])}
