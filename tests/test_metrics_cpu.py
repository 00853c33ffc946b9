"""SSIM / PSNR without a GPU: the float64 restatement of the contract (tests/ssim_ref64.py) against closed forms and against skimage's literal formula, why the
kernel's moments are taken of the shifted window, and the host-side surface (IrisError on CPU tensors, --metrics, the metrics.txt formats)."""
import numpy as np
import pytest
import torch

from ssim_ref64 import case_pairs, psnr_ref64, ssim_f32, ssim_ref64

H, W, C = 40, 56, 3


def test_constant_images_closed_form():
    for a, b, R in ((0.7, 0.5, 1.0), (0.0, 1.0, 1.0), (2.0, 0.25, 2.5)):
        S, m = ssim_ref64(np.full((9, 11, 3), a), np.full((9, 11, 3), b), R)
        c1 = (0.01 * R) ** 2
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        assert S.shape == (1, 3, 5, 3) and np.abs(S - want).max() <= 1e-15 and abs(m[0] - want) <= 1e-15


def test_identical_images_give_one():
    for name, (a, _, R) in case_pairs(H, W, C).items():
        S, m = ssim_ref64(a, a, R)
        assert (S == 1.0).all() and m[0] == 1.0, name
        assert psnr_ref64(a, a, R)[0] == np.inf, name


def _skimage_literal(a, b, R, dtype):
    """structural_similarity(a, b, data_range=R, channel_axis=-1) as skimage writes it: uniform_filter per channel, E[x^2] - E[x]^2, crop 3"""
    ndi = pytest.importorskip("scipy.ndimage")
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    cov_norm = 49.0 / 48.0
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    out = []
    for c in range(a.shape[-1]):
        x, y = a[..., c], b[..., c]
        ux, uy = ndi.uniform_filter(x, size=7), ndi.uniform_filter(y, size=7)
        uxx, uyy, uxy = ndi.uniform_filter(x * x, size=7), ndi.uniform_filter(y * y, size=7), ndi.uniform_filter(x * y, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        out.append(S[3:-3, 3:-3])
    return np.stack(out, -1)[None]


def test_contract_is_skimages_definition_and_the_shift_is_needed():
    pytest.importorskip("scipy")
    cases = case_pairs(H, W, C)
    for name in ("noise", "smooth", "step"):
        a, b, R = cases[name]
        S64, _ = ssim_ref64(a, b, R)
        lit = _skimage_literal(a, b, R, np.float64)
        dev = float(np.abs(lit - S64).max())
        print(f"{name}: skimage's formula in float64 against ssim_ref64 {dev:.3g}")
        assert lit.shape == S64.shape and dev <= 1e-10, name
    a, b, R = cases["bright_flat"]
    S64, _ = ssim_ref64(a, b, R)
    S32, _ = ssim_f32(a, b, R)
    d32 = float(np.abs(S32.astype(np.float64) - S64).max())
    lit32 = float(np.abs(_skimage_literal(a, b, R, np.float32).astype(np.float64) - S64).max())
    print(f"bright, nearly flat pair: E[x^2] - E[x]^2 in float32 deviates by {lit32:.3g}, the shifted window by {d32:.3g}")
    assert lit32 > 8 * d32


def test_f32_order_is_close_on_every_case():
    """ssim_f32 (the kernel's operation order) stays within 49 * 2^-23 of float64 on every input the GPU test uses (49 taps, one float32 rounding of relative
    2^-24 each, in numerator and denominator of a ratio <= 1): the bound 8 d32 of the GPU test is rounding-sized, the shift leaves no cancellation"""
    tol = 49 * 2.0 ** -23
    for name, (a, b, R) in case_pairs(H, W, C).items():
        S64, m64 = ssim_ref64(a, b, R)
        S32, m32 = ssim_f32(a, b, R)
        assert float(np.abs(S32 - S64).max()) <= tol and abs(m32[0] - m64[0]) <= tol, name


def test_cpu_tensors_raise():
    from iris_amd import _lib as L
    from iris_amd.utils.metrics import image_metrics, psnr_device, ssim
    a = torch.rand(9, 9, 3)
    for fn in (image_metrics, ssim, psnr_device):
        with pytest.raises(L.IrisError):
            fn(a, a)
    with pytest.raises(L.IrisError):
        image_metrics(a, torch.rand(9, 8, 3))


def test_parser_metrics_flag():
    from iris_amd import render as R
    base = ["--experiment_name", "e", "--emitter_path", "p"]
    assert R.build_parser().parse_args(base).metrics == "psnr"
    assert R.build_parser().parse_args(base + ["--metrics", "psnr,ssim"]).metrics == "psnr,ssim"
    with pytest.raises(SystemExit):
        R.build_parser().parse_args(base + ["--metrics", "lpips"])


def test_write_metrics_formats(tmp_path):
    from iris_amd import _lib as L
    from iris_amd import render as R
    p = tmp_path / "metrics.txt"
    R.write_metrics(str(p), [(0, 30.123456), (2, 20.0)], [(0, 0.912345678), (2, 0.5)])
    assert p.read_bytes() == b"Name, PSNR, SSIM\n00000, 30.12346, 0.91235\n00002, 20.00000, 0.50000\nmean , 25.06173, 0.70617\n"
    R.write_metrics(str(p), [(0, 30.123456), (2, 20.0)])
    assert p.read_bytes() == b"Name, PSNR\n00000, 30.12346\n00002, 20.00000\nmean , 25.06173\n"
    R.write_metrics(str(p), [])
    assert p.read_bytes() == b"Name, PSNR\nmean , nan\n"
    R.write_metrics(str(p), [], [])
    assert p.read_bytes() == b"Name, PSNR, SSIM\nmean , nan, nan\n"
    with pytest.raises(L.IrisError):
        R.write_metrics(str(p), [(0, 1.0)], [(1, 1.0)])
