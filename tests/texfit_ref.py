"""The trainable texture (iris_amd/csrc/iris_texmat.h, iris_amd/model/texture.py TextureBRDF, iris_amd/utils/texture.py fit_textures)
in numpy, no project import.

  fetch       the float fetch in FLOAT32, operation for operation in the kernel's order (the coordinates are tests/texmat_ref.py's): what the device must equal
              bit for bit.
  gradient    the transpose of that fetch in FLOAT64, taken from the float32 x0, y0, fx, fy of the fetch (they decide which texels are read and with which
              weights, so they are part of the contract); it also returns, per texel channel, the number of contributions n and S = sum |w_i g_i|, which the
              tolerance (n + 4) 2^-24 S of tests/test_texture_fit.py is made of.
  fit         fit_textures' loop in float64, Adam as tests/adam_ref.py states it (bias corrections folded into step_size and bc2), the recorded draws handed in.
"""
import math

import numpy as np

ROUGHNESS_MIN = np.float32(0.02)
F32 = np.float32


def _taps(tri, bary, ft, vt, H, W):
    """-> (ok, x0, x1, fx, y0, y1, fy): tests/texmat_ref.py's texel_coords in the kernel's own form of the clamp (a NaN coordinate becomes 0), and which rows
    have a triangle"""
    tri = np.asarray(tri, np.int64).reshape(-1)
    ft, vt = np.asarray(ft, np.int64), np.asarray(vt, F32)
    ok = (tri >= 0) & (tri < ft.shape[0])
    t = np.where(ok, tri, 0)
    b1, b2 = np.asarray(bary, F32).reshape(-1, 2)[:, 0], np.asarray(bary, F32).reshape(-1, 2)[:, 1]
    with np.errstate(all="ignore"):
        b0 = (F32(1.0) - b1) - b2
        i0, i1, i2 = ft[t, 0], ft[t, 1], ft[t, 2]
        u = ((b0 * vt[i0, 0]) + (b1 * vt[i1, 0])) + (b2 * vt[i2, 0])
        v = ((b0 * vt[i0, 1]) + (b1 * vt[i1, 1])) + (b2 * vt[i2, 1])
        x, y = u * F32(W) - F32(0.5), v * F32(H) - F32(0.5)
        x = np.where(x > 0, np.where(x < F32(W - 1), x, F32(W - 1)), F32(0)).astype(F32)
        y = np.where(y > 0, np.where(y < F32(H - 1), y, F32(H - 1)), F32(0)).astype(F32)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf).astype(F32), (y - yf).astype(F32)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    return ok, x0, np.minimum(x0 + 1, W - 1), fx, y0, np.minimum(y0 + 1, H - 1), fy


def _lerp(t00, t01, t10, t11, fx, fy):
    top, bot = t00 + fx * (t01 - t00), t10 + fx * (t11 - t10)
    return top + fy * (bot - top)


def fetch(tri, bary, ft, vt, texels):
    """tri (B,), bary (B, 2), ft (F, 3), vt (N, 2), texels (H, W, 5) float32 -> {'albedo' (B, 3), 'roughness' (B, 1), 'metallic' (B, 1)} FLOAT32, every operation a
    float32 operation in the kernel's order.  tri outside [0, F): zeros, roughness 0.02."""
    texels = np.asarray(texels, F32)
    H, W = texels.shape[:2]
    ok, x0, x1, fx, y0, y1, fy = _taps(tri, bary, ft, vt, H, W)
    with np.errstate(all="ignore"):
        out = _lerp(texels[y0, x0], texels[y0, x1], texels[y1, x0], texels[y1, x1], fx[:, None], fy[:, None])
    assert out.dtype == F32
    rough = np.where(out[:, 3] > ROUGHNESS_MIN, out[:, 3], ROUGHNESS_MIN)           # fmaxf: a NaN gives the floor
    z = ~ok
    return {"albedo": np.where(z[:, None], F32(0), out[:, :3]), "roughness": np.where(z, ROUGHNESS_MIN, rough)[:, None].astype(F32),
            "metallic": np.where(z, F32(0), out[:, 4])[:, None]}


def fetch64(tri, bary, ft, vt, texels):
    """the same fetch with the taps and lerps in float64 (the coordinates stay the contract's float32) -> (B, 5) float64 and the rows' validity"""
    texels = np.asarray(texels, np.float64)
    H, W = texels.shape[:2]
    ok, x0, x1, fx, y0, y1, fy = _taps(tri, bary, ft, vt, H, W)
    out = _lerp(texels[y0, x0], texels[y0, x1], texels[y1, x0], texels[y1, x1], fx.astype(np.float64)[:, None], fy.astype(np.float64)[:, None])
    out[:, 3] = np.maximum(out[:, 3], float(ROUGHNESS_MIN))
    out[~ok] = [0.0, 0.0, 0.0, float(ROUGHNESS_MIN), 0.0]
    return out, ok


def gradient(tri, bary, ft, vt, texels, g_albedo, g_rough, g_metal, gate="float32"):
    """-> (g_texels, n, S), each (H, W, 5): the float64 gradient of sum(out * g) with respect to the texels, the number of contributions per texel channel and
    S = sum |w g| over them.  Weights w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy), w10 = (1 - fx) fy, w11 = fx fy from the float32 fx, fy, in float64; taps that the
    clamp merges land on one texel and are counted once each.  The roughness gradient passes where the interpolated roughness is > 0.02 -- gate = 'float32': the
    float32 fetch's value (the kernel's decision), 'float64': the float64 fetch's (for central differences) -- and a blocked row contributes nothing."""
    texels = np.asarray(texels)
    H, W = texels.shape[:2]
    ok, x0, x1, fx, y0, y1, fy = _taps(tri, bary, ft, vt, H, W)
    if gate == "float32":
        t = texels.astype(F32)
        with np.errstate(all="ignore"):
            r = _lerp(t[y0, x0, 3], t[y0, x1, 3], t[y1, x0, 3], t[y1, x1, 3], fx, fy)
        passes = r > ROUGHNESS_MIN
    else:
        t = texels.astype(np.float64)
        passes = _lerp(t[y0, x0, 3], t[y0, x1, 3], t[y1, x0, 3], t[y1, x1, 3], fx.astype(np.float64), fy.astype(np.float64)) > float(ROUGHNESS_MIN)
    B = ok.shape[0]
    g = np.concatenate([np.asarray(g_albedo, np.float64).reshape(B, 3), np.asarray(g_rough, np.float64).reshape(B, 1), np.asarray(g_metal, np.float64).reshape(B, 1)], 1)
    live = np.repeat(ok[:, None], 5, 1)
    live[:, 3] &= passes
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    grad, n, S = np.zeros((H * W, 5)), np.zeros((H * W, 5), np.int64), np.zeros((H * W, 5))
    for ys, xs, w in ((y0, x0, (1 - fx) * (1 - fy)), (y0, x1, fx * (1 - fy)), (y1, x0, (1 - fx) * fy), (y1, x1, fx * fy)):
        flat = ys * W + xs
        for ch in range(5):
            m = live[:, ch]
            term = w[m] * g[m, ch]
            grad[:, ch] += np.bincount(flat[m], weights=term, minlength=H * W)
            S[:, ch] += np.bincount(flat[m], weights=np.abs(term), minlength=H * W)
            n[:, ch] += np.bincount(flat[m], minlength=H * W)
    grad, n, S = grad.reshape(H, W, 5), n.reshape(H, W, 5), S.reshape(H, W, 5)
    return grad, n, S


def quantize(texels):
    """TextureBRDF.to_images' rule: floor(clamp(x, 0, 1) * 255 + 0.5) in float32, a NaN as 0 -> (H, W, 5) uint8"""
    t = np.asarray(texels, F32)
    t = np.clip(np.where(np.isnan(t), F32(0), t), F32(0), F32(1))
    return np.floor(t * F32(255) + F32(0.5)).astype(np.uint8)


# ---- the fit's test case: the identity quad (two faces over the whole UV square), a material of wavelength 4 texels at 16 x 16
QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
QUAD_VT = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
WAVE_PHASE = (0.0, 0.7, 1.4, 2.1, 2.8)             # albedo r, g, b, roughness, metallic


def wave(x, y):
    """the test material at positions (x, y) -> (N, 5) float64: 0.5 + 0.35 sin(2 pi 4 x + phase) cos(2 pi 4 y) per channel, inside [0.15, 0.85]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([0.5 + 0.35 * np.sin(2 * np.pi * 4 * x + ph) * np.cos(2 * np.pi * 4 * y) for ph in WAVE_PHASE], 1)


def quad_draw(rng, n):
    """n uniform points of the identity quad -> (face (n,) int64, bary (n, 2) float32, position (n, 3) float32 in verify_points' order of operations)"""
    face = rng.integers(0, 2, n).astype(np.int64)
    b = rng.random((n, 2)).astype(F32)
    b = np.where((b[:, :1] + b[:, 1:]) > 1.0, F32(1.0) - b, b).astype(F32)
    b1, b2 = b[:, :1], b[:, 1:]
    p0, p1, p2 = (QUAD_V[QUAD_F[face, k]] for k in range(3))
    pos = ((F32(1.0) - b1 - b2) * p0 + b1 * p1) + b2 * p2
    assert pos.dtype == F32
    return face, b, pos


def held_out_mse(texels, face, bary, want):
    """the mean squared difference of the float64 fetch of `texels` (H, W, 5) at (face, bary) on the identity quad from `want` (N, 5)"""
    got, _ = fetch64(face, bary, QUAD_F, QUAD_VT, texels)
    return float(((got - want) ** 2).mean())


def adam_step64(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """tests/adam_ref.py's step (no weight decay) in float64 -> (p', m', v'); step counts from 1"""
    step_size, bc2 = lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step)
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + ((1.0 - beta2) * g) * g
    return p - step_size * (m / (np.sqrt(v) / bc2 + eps)), m, v


def fit(texels0, ft, vt, draws, targets, lr):
    """fit_textures in float64: texels0 (H, W, 5); draws[k] = (face, bary) of step k, targets[k] = the material's (M, 5) values there -> (texels, [loss per step]).
    loss = the mean over the points and the 5 channels of the squared difference; the roughness gate is the float64 fetch's."""
    p = np.asarray(texels0, np.float64).copy()
    m, v, losses = np.zeros_like(p), np.zeros_like(p), []
    for k, ((face, bary), want) in enumerate(zip(draws, targets)):
        got, _ = fetch64(face, bary, ft, vt, p)
        d = got - np.asarray(want, np.float64)
        losses.append(float((d ** 2).mean()))
        g = 2.0 * d / d.size
        grad, _, _ = gradient(face, bary, ft, vt, p, g[:, :3], g[:, 3], g[:, 4], gate="float64")
        p, m, v = adam_step64(p, grad, m, v, k + 1, lr)
    return p, losses
