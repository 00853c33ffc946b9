"""The two kernels of iris_amd/csrc/iris_validate.h restated in numpy, for clarity and not for speed: the float32 steps as include/iris_hip.h states them,
float64 sums for the loss (in numpy's order: the kernel's differs, and the tests bound the difference of two float64 sums), sequential float32 sums for
the maps (the kernel's order: compared bit for bit)."""
import numpy as np

F = np.float32


def kd_loss_sums(albedo, metallic, valid, img_hw, *, gt=None, emit=None, codes=None, lut=None):
    """iris_val_kd_loss: albedo (N HW, 3), metallic (N HW), valid (N HW); gt, emit (N HW, 3) float32, or codes (N HW, 3) uint8 with lut (256,) float32
    -> S (N,) float64"""
    hw = int(img_hw[0]) * int(img_hw[1])
    albedo = np.asarray(albedo, F).reshape(-1, 3)
    metallic = np.asarray(metallic, F).reshape(-1, 1)
    valid = np.asarray(valid).reshape(-1, 1) != 0
    assert (gt is None) != (codes is None)
    if codes is None:
        e = np.asarray(emit, F).reshape(-1, 3)
        m = (((e[:, 0] + e[:, 1]) + e[:, 2]) == 0).astype(F).reshape(-1, 1)
        g = np.asarray(gt, F).reshape(-1, 3)
    else:
        m = np.ones((albedo.shape[0], 1), F)
        g = np.asarray(lut, F)[np.asarray(codes, np.uint8).reshape(-1, 3)]
    with np.errstate(invalid="ignore", over="ignore"):
        est = np.where(valid, albedo * (F(1.0) - metallic), F(0.0)).astype(F)
        d = (g * m - est * m).astype(F)
        q = (d * d).astype(F)
    return q.astype(np.float64).reshape(-1, hw * 3).sum(1)


def loss_and_psnr(S, img_hw):
    loss = np.asarray(S, np.float64) / float(3 * int(img_hw[0]) * int(img_hw[1]))
    return loss, -10.0 * np.log10(np.maximum(loss, 1e-5))


def val_intrinsics(radiance, e0, valid_next, albedo, roughness, metallic, spp, maps=None):
    """iris_val_intrinsics: per-sample arrays of N = B spp rows (pixel-major) -> {'albedo' (B,3), 'roughness' (B,1), 'metallic' (B,1), 'emission' (B,3)} float32,
    map[b] += (x_0 + ... + x_{spp-1}) * (1.0f / spp) with the samples added in order in float32; maps: what to add into (default zeros)"""
    radiance = np.asarray(radiance, F).reshape(-1, 3)
    e0 = np.asarray(e0, np.int64).reshape(-1)
    n = e0.shape[0]
    B = n // spp
    hit = (e0 >= 0) & (e0 < radiance.shape[0])
    em = np.where(hit[:, None], radiance[np.where(hit, e0, 0)], F(0.0)).astype(F)
    keep = ((np.asarray(valid_next).reshape(-1) != 0) | (e0 >= 0)) & (((em[:, 0] + em[:, 1]) + em[:, 2]) == 0)
    terms = {"albedo": np.where(keep[:, None], np.asarray(albedo, F).reshape(n, 3), F(0.0)),
             "roughness": np.where(keep[:, None], np.asarray(roughness, F).reshape(n, 1), F(0.0)),
             "metallic": np.where(keep[:, None], np.asarray(metallic, F).reshape(n, 1), F(0.0)), "emission": em}
    inv = F(1.0) / F(spp)
    out = {}
    for k, x in terms.items():
        x = x.astype(F).reshape(B, spp, -1)
        acc = np.zeros((B, x.shape[2]), F)
        with np.errstate(invalid="ignore", over="ignore"):
            for s in range(spp):
                acc = (acc + x[:, s]).astype(F)
            base = np.zeros_like(acc) if maps is None else np.asarray(maps[k], F).reshape(acc.shape)
            out[k] = (base + (acc * inv).astype(F)).astype(F)
    return out
