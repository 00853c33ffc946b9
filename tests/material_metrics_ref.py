"""Helper (not a test): the material metrics' contract (iris_amd/csrc/iris_matmetrics.h, iris_amd/utils/material_metrics.py) in numpy, twice, and the
adversarial inputs the tests share.  Written from the contract; the restatements import nothing of the package.

  exact(gt, est)     (a) the contract in code values: int64 sums and counts, S_emit in float64.
  literal(gt, est)   (b) the reference's utils/metric_brdf.py:32-80 line by line in float32: x / 255, clamp(0.2, 1), `== 1`, mean squared errors.
                     torch's .long() is truncation toward zero; of a NaN it is whatever the machine's conversion gives (the contract says NaN -> code 0), so
                     (a) and (b) are compared on inputs whose albedo / kd ground truth holds no NaN (make_inputs(colour_nan=False)).
"""
import math

import numpy as np

F = np.float32
KEYS = ("emit", "albedo", "kd", "rough")


def _stack(d):
    out = {}
    for k in KEYS:
        a = np.asarray(d[k])
        want = 3 if k == "rough" else 4
        out[k] = a[None] if a.ndim == want - 1 else a
    return out


def q(x):
    """save_png's quantisation of a float32 array: trunc(min(max(x, 0), 1) * 255f), NaN -> 0 (fmax / fmin drop the NaN), one float32 multiply"""
    x = np.asarray(x, F)
    return np.trunc(np.fmin(np.fmax(x, F(0)), F(1)) * F(255)).astype(np.int64)


def codes(x):
    """an estimate map as code values: uint8 as it is, float32 through q"""
    x = np.asarray(x)
    return x.astype(np.int64) if x.dtype == np.uint8 else q(x)


def emitter_mask(e):
    e = np.asarray(e, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((e[..., 0] + e[..., 1]) + e[..., 2]) > F(0)


def rough_gt_code(x):
    """clamp(T(x * 255f), 51, 255), T saturating truncation, NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(x, F) * F(255)
    p = np.where(np.isnan(p), F(0), p)
    return np.trunc(np.clip(p, F(51), F(255))).astype(np.int64)       # clamping to [51, 255] first commutes with the truncation: both bounds are integers


def exact(gt, est):
    """-> {'sums': (N,7) int64 [S_albedo, S_kd, S_rough, n_gt, n_est, n_and, n_or], 's_emit': (N,) float64, 'bound_log', 'bound_sq': (N,) float64, the two
    sums of the S_emit tolerance: sum 2|d|(|la| + |lb|) and sum d^2}"""
    gt, est = _stack(gt), _stack(est)
    N, H, W = gt["rough"].shape
    m = emitter_mask(gt["emit"])
    m_est = emitter_mask(est["emit"])
    keep = ~m
    a_gt = q(gt["albedo"]) * keep[..., None]
    a = codes(est["albedo"]) * keep[..., None]
    r_gt = rough_gt_code(gt["rough"]) * keep
    r = np.clip(codes(est["rough"]), 51, 255) * keep
    diff = (r_gt == 255)[..., None]
    k_gt = q(gt["kd"]) * diff
    k = codes(est["kd"]) * diff
    ax = (1, 2)
    sums = np.stack([((a - a_gt) ** 2).sum((1, 2, 3)), ((k - k_gt) ** 2).sum((1, 2, 3)), ((r - r_gt) ** 2).sum(ax), m.sum(ax), m_est.sum(ax), (m & m_est).sum(ax),
                     (m | m_est).sum(ax)], 1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        la = np.log(est["emit"].astype(np.float64) + 1.0)
        lb = np.log(gt["emit"].astype(np.float64) + 1.0)
        d = la - lb
        s_emit, b_log, b_sq = [], [], []
        for n in range(N):
            dd = (d[n] * d[n]).reshape(-1)
            finite = bool(np.all(np.isfinite(dd)))
            s_emit.append(math.fsum(dd) if finite else float(np.sum(dd)))
            b_log.append(math.fsum((2.0 * np.abs(d[n]) * (np.abs(la[n]) + np.abs(lb[n]))).reshape(-1)) if finite else float("nan"))
            b_sq.append(s_emit[-1])
    return {"sums": sums, "s_emit": np.array(s_emit, np.float64), "bound_log": np.array(b_log, np.float64), "bound_sq": np.array(b_sq, np.float64)}


def s_emit_tolerance(ref, n, H, W, c=2.0):
    """the S_emit assertion's bound for view n: 2^-53 (c sum 2|d|(|la| + |lb|) + (ceil(log2(3 H W)) + 2) sum d^2) -- a c-half-ulp logarithm and the tree's roundings"""
    return 2.0 ** -53 * (c * ref["bound_log"][n] + (math.ceil(math.log2(3 * H * W)) + 2) * ref["bound_sq"][n])


def per_view(sums, s_emit, H, W):
    """the contract's per-view values from (a)'s sums, float64: the MSEs, emit_iou = n_and / n_or and emit_log_mse = S_emit / (3 H W), the last two NaN for a
    view with n_gt == 0"""
    s = np.asarray(sums, np.float64)
    hw = float(H * W)
    has = np.asarray(sums)[:, 3] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"mse_albedo": s[:, 0] / (255.0 ** 2 * 3 * hw), "mse_kd": s[:, 1] / (255.0 ** 2 * 3 * hw), "mse_roughness": s[:, 2] / (255.0 ** 2 * hw),
                "emit_iou": np.where(has, s[:, 5] / s[:, 6], np.nan), "emit_log_mse": np.where(has, np.asarray(s_emit, np.float64) / (3 * hw), np.nan)}


def summary(pv):
    """metric_brdf.py:88-92 in float64 from per_view()'s values"""
    psnr = lambda mse: float(np.mean(-10.0 * np.log10(np.maximum(mse, 1e-10))))
    some = lambda v: float(np.mean(v[~np.isnan(v)])) if np.any(~np.isnan(v)) else float("nan")
    return {"kd": psnr(pv["mse_kd"]), "albedo": psnr(pv["mse_albedo"]), "roughness": psnr(pv["mse_roughness"]), "emit_iou": some(pv["emit_iou"]),
            "emit_log_mse": some(pv["emit_log_mse"])}


def _long(x):
    """torch's .long() of a float32 array (truncation toward zero)"""
    with np.errstate(invalid="ignore"):
        return np.trunc(x).astype(np.int64)


def literal(gt, est_u8):
    """(b): metric_brdf.py:32-80 for ONE view in float32.  gt: (H,W,3) / (H,W) float32 maps as the EXR files hold them; est_u8: 'emit' float32, the others uint8
    as cv2 reads the PNGs.  -> {'mse_roughness', 'mse_albedo', 'mse_kd', 'emit_iou', 'emit_log_mse'} (the last two None for a view without an emitter): float32
    means as numpy takes them (torch's mse_loss adds in another order: the comparison allows float32 summation rounding)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        emission_gt = np.asarray(gt["emit"], F)
        emission_mask = emitter_mask(emission_gt)
        albedo_gt = _long(np.clip(np.asarray(gt["albedo"], F), F(0), F(1)) * F(255)).astype(F) / F(255)
        albedo_gt[emission_mask] = 0
        kd_gt = _long(np.clip(np.asarray(gt["kd"], F), F(0), F(1)) * F(255)).astype(F) / F(255)
        kd_gt[emission_mask] = 0
        roughness_gt = np.clip(_long(np.asarray(gt["rough"], F) * F(255)).astype(F) / F(255), F(0.2), F(1))
        roughness_gt[emission_mask] = 0
        diff_mask = roughness_gt == 1
        kd_gt[~diff_mask] = 0
        emission = np.asarray(est_u8["emit"], F)
        albedo = est_u8["albedo"].astype(F) / F(255)
        albedo[emission_mask] = 0
        kd = est_u8["kd"].astype(F) / F(255)
        kd[emission_mask] = 0
        kd[~diff_mask] = 0
        roughness = np.clip(est_u8["rough"].astype(F) / F(255), F(0.2), F(1))
        roughness[emission_mask] = 0
        emission_mask_est = emitter_mask(emission)
        mse = lambda a, b: F(np.mean((a - b) ** 2, dtype=F))
        out = {"emit_iou": None, "emit_log_mse": None}
        if emission_mask.any():
            out["emit_iou"] = float((emission_mask & emission_mask_est).sum() * 1.0 / (emission_mask | emission_mask_est).sum())
            out["emit_log_mse"] = mse(np.log(emission + F(1)), np.log(emission_gt + F(1)))
        out["mse_roughness"] = mse(roughness, roughness_gt)
        out["mse_albedo"] = mse(albedo, albedo_gt)
        out["mse_kd"] = mse(kd, kd_gt)
    return out


def log_mse_f32_scale(emit_gt, emit):
    """The size of the float32 evaluation's error of ONE view's emission log-MSE, u = 2^-24: x + 1 rounds (the logarithm moves by <= u), the logarithm rounds
    (u |l|), the difference rounds (u |d|): |error of d| <= u t with t = 2 + |la| + |lb| + |d|; a squared term is off by 2 |d| u t + (u t)^2 + u d^2, and a
    pairwise float32 mean of n terms adds u ceil(log2 n) of the sum.  -> the mean over the terms of that."""
    la = np.log(np.asarray(emit, np.float64) + 1.0).reshape(-1)
    lb = np.log(np.asarray(emit_gt, np.float64) + 1.0).reshape(-1)
    d = la - lb
    u = 2.0 ** -24
    t = 2.0 + np.abs(la) + np.abs(lb) + np.abs(d)
    return float(np.mean(2.0 * np.abs(d) * u * t + (u * t) ** 2 + u * d * d * (1 + math.ceil(math.log2(max(d.size, 2))))))


# ---- the adversarial inputs
def _code_neighbours():
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(F)          # float32(k / 255)
    return np.concatenate([k, np.nextafter(k, F(-1)), np.nextafter(k, F(2))]).astype(F)


def _plant(rng, flat, specials):
    """writes the special values over random places of `flat` (all of them where they fit in half of it, else a random sample)"""
    n = min(len(specials), flat.size // 2)
    if n:
        flat[rng.choice(flat.size, n, replace=False)] = rng.permutation(specials)[:n]


def make_inputs(N, H, W, seed, emitter_views=None, colour_nan=True):
    """-> (gt, est_u8, est_f32): dicts of numpy arrays, (N,H,W,3) / (N,H,W).  gt float32 as the EXR maps; est_u8: 'emit' float32, the others uint8;
    est_f32: the same estimate as float32 maps whose quantisation is NOT est_u8 everywhere (they are two estimates, each covering all 256 codes).
    In rough_gt, albedo_gt and kd_gt: every float32(k / 255) with both neighbours, values < 0, > 1, 1e10, -0.0 and NaN (albedo / kd: only with colour_nan);
    rough_gt rows exactly 1.0 and rows just below; emission rows that cancel, (1e-8, -1e-8, 0), and negative sums; every emission value finite and > -1.
    emitter_views: per view, whether its ground truth has an emitter (default: all have)."""
    rng = np.random.default_rng(seed)
    P = N * H * W
    odd = np.array([-0.5, -1e-3, 1.0 + 2.0 ** -23, 1.5, 1e10, -0.0, 0.0, 1.0, float("nan"), 0.2, 0.19999999], F)
    near = _code_neighbours()

    def colour():
        a = rng.random(P * 3).astype(F)
        _plant(rng, a, np.concatenate([near, odd if colour_nan else odd[~np.isnan(odd)]]))
        return a.reshape(N, H, W, 3)
    gt = {"albedo": colour(), "kd": colour()}
    r = rng.random(P).astype(F)
    r[rng.random(P) < 0.3] = F(1.0)
    _plant(rng, r, np.concatenate([near, odd]))
    r = r.reshape(N, H, W)
    r[:, 0, :] = F(1.0)                                                # a row exactly 1.0 ...
    if H > 1:
        r[:, 1, :] = np.nextafter(F(1.0), F(0))                        # ... and one just below: code 254, not diffuse
    if H > 2:
        r[:, 2, ::2] = F(1.0) - F(2.0 ** -9)                           # x * 255 rounds below 255 in float32
    gt["rough"] = r

    e = np.zeros((P, 3), F)
    lit = rng.random(P) < 0.25
    e[lit] = (rng.random((int(lit.sum()), 3)) * rng.choice([0.01, 1.0, 50.0], (int(lit.sum()), 1))).astype(F)
    idx = rng.permutation(P)
    for j, row in enumerate(([1e-8, -1e-8, 0.0], [-0.5, 0.25, 0.125], [0.25, 0.25, -0.5], [-0.0, 0.0, 0.0], [1e30, 0.0, 0.0], [-0.999, 0.5, 0.6])):
        e[idx[j::37][:max(1, P // 40)]] = np.array(row, F)             # (the first row lands on idx[0]: also in a one-pixel view)
    e = e.reshape(N, H, W, 3)
    if emitter_views is not None:
        for n, has in enumerate(emitter_views):
            if not has:
                e[n] = np.minimum(e[n], F(0)) * F(0.5)                 # nothing positive: the sum is never > 0
    gt["emit"] = e

    est = e.reshape(P, 3).copy() * rng.choice([0.0, 0.5, 1.0, 1.5], (P, 1)).astype(F)
    extra = rng.random(P) < 0.1                                        # emitters the ground truth does not have
    est[extra] = rng.random((int(extra.sum()), 3)).astype(F) * F(2)
    est = np.maximum(est, F(-0.999)).reshape(N, H, W, 3)

    def u8(n):
        a = rng.integers(0, 256, n).astype(np.uint8)
        _plant(rng, a, np.arange(256, dtype=np.uint8))
        return a

    def f32(n):
        a = ((rng.integers(0, 256, n) + rng.random(n)) / 255.0).astype(F)
        _plant(rng, a, np.concatenate([near, odd]))
        return a
    est_u8 = {"emit": est, "albedo": u8(P * 3).reshape(N, H, W, 3), "kd": u8(P * 3).reshape(N, H, W, 3), "rough": u8(P).reshape(N, H, W)}
    est_f32 = {"emit": est, "albedo": f32(P * 3).reshape(N, H, W, 3), "kd": f32(P * 3).reshape(N, H, W, 3), "rough": f32(P).reshape(N, H, W)}
    return gt, est_u8, est_f32


# ---- the two trees of files the command line reads (written with the package's EXR writer and PIL: the only use of the package here)
def write_gt_tree(root, gt, n_images=None):
    """the ground-truth folder of a synthetic split: Emit/, albedo/, DiffCol/, Roughness/ (the roughness in the B channel only) and n_images files under Image/"""
    import os
    from iris_amd.utils.exr import write_exr
    N = gt["rough"].shape[0]
    for d in ("Image", "Emit", "albedo", "DiffCol", "Roughness"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for i in range(N):
        write_exr(os.path.join(root, "Emit", "%03d_0001.exr" % i), gt["emit"][i], "zip")
        write_exr(os.path.join(root, "albedo", "%03d.exr" % i), gt["albedo"][i], "zips")
        write_exr(os.path.join(root, "DiffCol", "%03d_0001.exr" % i), gt["kd"][i], "none")
        rough = np.stack([gt["rough"][i] * 0 + 0.25, gt["rough"][i] * 0 + 0.5, gt["rough"][i]], -1)          # R, G, B: only B is the roughness
        write_exr(os.path.join(root, "Roughness", "%03d_0001.exr" % i), rough, "zip")
    for i in range(N if n_images is None else n_images):
        write_exr(os.path.join(root, "Image", "%03d_0001.exr" % i), np.zeros((2, 2, 3), np.float32))


def write_method_tree(root, est_u8):
    """<output_path>/<split> as the render stage writes it, from uint8 maps; the roughness PNG's three channels differ: only B is the roughness"""
    import os
    from PIL import Image
    from iris_amd.utils.exr import write_exr
    for d in ("emission", "a_prime", "diffuse", "roughness"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for i in range(est_u8["rough"].shape[0]):
        write_exr(os.path.join(root, "emission", "%05d_emission.exr" % i), est_u8["emit"][i], "zip")
        Image.fromarray(est_u8["albedo"][i]).save(os.path.join(root, "a_prime", "%05d_a_prime.png" % i))
        Image.fromarray(est_u8["kd"][i]).save(os.path.join(root, "diffuse", "%05d_kd.png" % i))
        r = est_u8["rough"][i]
        Image.fromarray(np.stack([r // 2, 255 - r, r], -1)).save(os.path.join(root, "roughness", "%05d_roughness.png" % i))
