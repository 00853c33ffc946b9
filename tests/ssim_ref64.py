"""Helper (not a test): the SSIM / PSNR contract of iris_amd/csrc/iris_metrics.h in numpy.

The contract is skimage.metrics.structural_similarity's defaults restated: uniform 7 x 7 window, K1 0.01, K2 0.03, sample covariance (cov_norm 49/48),
C1 = (K1 R)^2, C2 = (K2 R)^2, per channel and per window that lies fully inside the image
    S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),     mssim = mean over channels of the mean of S over the (H-6)(W-6) windows.

ssim_ref64   the contract in float64 with explicit windows and centred moments (v = mean((x - ux)(y - uy)): nothing cancels).
ssim_f32     the kernel's documented operation order in float32 (window shifted by its centre pixel, taps row-major, one rounding per operation): exists only
             to measure d32, the float32 / float64 deviation of that order on a given input.
psnr_ref64   10 log10(R^2 / mean((a - b)^2)) in float64.
Images are (H, W), (H, W, C) or (N, H, W, C); the maps come back as (N, H-6, W-6, C), the mssim as (N,)."""
import numpy as np

WIN = 7


def _stack(x, dtype):
    x = np.asarray(x, dtype)
    if x.ndim == 2:
        return x[None, :, :, None]
    if x.ndim == 3:
        return x[None]
    assert x.ndim == 4, x.shape
    return x


def _windows(x):
    """(N, H, W, C) -> (N, H-6, W-6, C, 7, 7): window [.., i, j] = pixel (y + i, x + j), i.e. taps in row-major order"""
    return np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN), axis=(1, 2))


def ssim_ref64(a, b, R=1.0):
    a, b = _stack(a, np.float64), _stack(b, np.float64)
    assert a.shape == b.shape and a.shape[1] >= WIN and a.shape[2] >= WIN
    R = float(R)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    cov_norm = 49.0 / 48.0
    wa, wb = _windows(a), _windows(b)
    ux, uy = wa.mean((-1, -2)), wb.mean((-1, -2))
    da, db = wa - ux[..., None, None], wb - uy[..., None, None]
    vx, vy, vxy = cov_norm * (da * da).mean((-1, -2)), cov_norm * (db * db).mean((-1, -2)), cov_norm * (da * db).mean((-1, -2))
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return S, S.mean((1, 2)).mean(-1)


def ssim_f32(a, b, R=1.0):
    f = np.float32
    a, b = _stack(a, f), _stack(b, f)
    assert a.shape == b.shape and a.shape[1] >= WIN and a.shape[2] >= WIN
    k1r, k2r = f(0.01) * f(R), f(0.03) * f(R)
    c1, c2 = k1r * k1r, k2r * k2r
    cov_norm = f(49) / f(48)
    wa, wb = _windows(a), _windows(b)
    xc, yc = wa[..., 3, 3], wb[..., 3, 3]
    sx, sy, sxx, syy, sxy = (np.zeros(xc.shape, f) for _ in range(5))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(WIN):
            for j in range(WIN):
                dx, dy = wa[..., i, j] - xc, wb[..., i, j] - yc
                sx = sx + dx; sy = sy + dy; sxx = sxx + dx * dx; syy = syy + dy * dy; sxy = sxy + dx * dy
        n = f(49)
        mx, my = sx / n, sy / n
        ux, uy = xc + mx, yc + my
        vx, vy, vxy = cov_norm * (sxx / n - mx * mx), cov_norm * (syy / n - my * my), cov_norm * (sxy / n - mx * my)
        S = ((f(2) * ux * uy + c1) * (f(2) * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    assert S.dtype == f
    return S, S.astype(np.float64).mean((1, 2)).mean(-1)


def psnr_ref64(a, b, R=1.0):
    a, b = _stack(a, np.float64), _stack(b, np.float64)
    mse = ((a - b) ** 2).mean((1, 2, 3))
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(float(R) ** 2 / mse)


# ---- the inputs the tests share (seeded; shapes (H, W, C))
def case_pairs(H, W, C, seed=0):
    """name -> (a, b, data_range), float32 (H, W, C)"""
    g = np.random.default_rng(seed)
    f = np.float32
    yy, xx = np.mgrid[0:H, 0:W]
    noise = g.random((H, W, C))
    smooth = 0.5 + 0.4 * np.sin(0.31 * xx + 0.17 * yy)[..., None] * np.cos(0.05 * xx[..., None] * np.arange(1, C + 1))
    flat = 0.9 + 1e-3 * g.standard_normal((H, W, C))
    flat_b = flat + 1e-3 * g.standard_normal((H, W, C))
    half = flat.copy(); half[:, :W // 2] = 0.0
    half_b = half + 1e-3 * g.standard_normal((H, W, C)); half_b[:, :W // 2] = np.abs(half_b[:, :W // 2])
    step = np.zeros((H, W, C)); step[:, W // 2:] = 0.8; step += 0.1
    step_b = np.zeros((H, W, C)); step_b[:, W // 2 + 2:] = 0.8; step_b += 0.1
    hdr = 2.5 * g.random((H, W, C)) ** 2
    cases = {
        "noise": (noise, np.clip(noise + 0.1 * g.standard_normal((H, W, C)), 0, 1), 1.0),
        "smooth": (smooth, smooth + 0.02 * g.standard_normal((H, W, C)), 1.0),
        "bright_flat": (flat, flat_b, 1.0),
        "half_dark": (half, half_b, 1.0),
        "step": (step, step_b, 1.0),
        "constant": (np.full((H, W, C), 0.7), np.full((H, W, C), 0.5), 1.0),
        "hdr": (hdr, np.clip(hdr + 0.05 * g.standard_normal((H, W, C)), 0, 2.5), 2.5),
    }
    return {k: (np.ascontiguousarray(a, f), np.ascontiguousarray(b, f), R) for k, (a, b, R) in cases.items()}
