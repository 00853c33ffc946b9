"""SSIM / PSNR on the GPU (iris_amd/csrc/iris_metrics.h, iris_amd/utils/metrics.py) against the float64 restatement of the contract (tests/ssim_ref64.py, which
tests/test_metrics_cpu.py ties to skimage's literal formula).

Bounds (the rule of tests/test_render.py and tests/test_crf.py), per case:
    ssim_map: max |S - S64| <= max(8 d32, 2^-22)          d32 = max |ssim_f32 - ssim_ref64| on that same input (the documented float32 order against float64)
    ssim:     |ssim - mssim64| <= max(8 |mssim_f32 - mssim64|, 2^-24)
    mse (from the double sums): relative 1e-12 against float64 numpy -- the sums differ from numpy's in order only
Shapes: 7 x 7 (one window), 8 x 9, and 21 x 139 -- the kernel's tile is 64 x 16 pixels, so three tiles in x and two in y, both ragged -- each at C = 1 and 3.
No figure from an MI355X is recorded in this file; the tests print them."""
import functools

import numpy as np
import pytest
import torch

from ssim_ref64 import case_pairs, psnr_ref64, ssim_f32, ssim_ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(7, 7), (8, 9), (21, 139)]


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared references are read-only)


@functools.lru_cache(maxsize=None)
def reference(H, W, C):
    """name -> (a, b, R, S64, m64, S32, m32, mse64): computed once per shape, shared, never written to"""
    out = {}
    for name, (a, b, R) in case_pairs(H, W, C, seed=H * 1000 + W * 10 + C).items():
        S64, m64 = ssim_ref64(a, b, R)
        S32, m32 = ssim_f32(a, b, R)
        mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
        for x in (a, b, S64, S32):
            x.setflags(write=False)
        out[name] = (a, b, R, S64, float(m64[0]), S32, float(m32[0]), mse)
    return out


def check(name, got, S64, m64, S32, m32, mse64, H, W, C, R):
    """got: image_metrics(..., full=True) of ONE image (index 0 of the tensors handed in)"""
    smap = got["ssim_map"].cpu().numpy().astype(np.float64)
    ssim, psnr = float(got["ssim"].cpu()), float(got["psnr"].cpu())
    mse = float(got["sums"][:, 0].sum().cpu()) / (H * W * C)
    d32 = float(np.abs(S32.astype(np.float64) - S64).max())
    b_map, b_ssim = max(8 * d32, 2.0 ** -22), max(8 * abs(m32 - m64), 2.0 ** -24)
    dev_map, dev_ssim = float(np.abs(smap - S64[0]).max()), abs(ssim - m64)
    same_bits = bool(np.array_equal(smap.astype(np.float32), S32[0]))
    print(f"{H}x{W}x{C} {name}: map deviation {dev_map:.3g} (bound {b_map:.3g}, d32 {d32:.3g}), ssim deviation {dev_ssim:.3g} (bound {b_ssim:.3g}), "
          f"mse relative {abs(mse - mse64) / mse64 if mse64 else abs(mse):.3g}, map equals the float32 restatement bit for bit: {same_bits}")
    assert smap.shape == S64[0].shape and np.isfinite(smap).all()
    assert dev_map <= b_map, name
    assert dev_ssim <= b_ssim, name
    assert abs(mse - mse64) <= 1e-12 * mse64, name
    want_psnr = 10.0 * np.log10(R * R / mse64) if mse64 else np.inf
    assert psnr == want_psnr or abs(psnr - want_psnr) <= 5e-12, name                  # d psnr = (10 / ln 10) d mse / mse = 4.4e-12 at 1e-12


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_case_against_float64(hw, C):
    """every input, one image per launch (N = 1): map, ssim and mse under the bounds; the constant pair also against its closed form"""
    from iris_amd.utils.metrics import image_metrics
    H, W = hw
    for name, (a, b, R, S64, m64, S32, m32, mse64) in reference(H, W, C).items():
        ta, tb = T(a), T(b)
        if C == 1 and name == "noise":
            ta, tb = ta[..., 0], tb[..., 0]                 # the (H, W) form
        got = image_metrics(ta, tb, R, full=True)
        assert got["ssim"].shape == (1,) and got["psnr"].shape == (1,) and got["ssim"].dtype == torch.float64 and got["ssim"].is_cuda
        check(name, {k: v[0] for k, v in got.items()}, S64, m64, S32, m32, mse64, H, W, C, R)
        if name == "constant":
            x, y, c1 = float(np.float32(0.7)), float(np.float32(0.5)), 0.01 ** 2          # the pixels are float32
            closed = (2 * x * y + c1) / (x * x + y * y + c1)
            assert abs(float(got["ssim"].cpu()) - closed) <= max(8 * abs(m32 - m64), 2.0 ** -24)
            assert float(psnr_ref64(a, b, R)[0]) == pytest.approx(float(got["psnr"].cpu()), abs=5e-12)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stack_of_different_images(hw, C):
    """N = 3, three different pairs in one launch: every image against its own reference (a wrong image's slab would show), the same bits as its own N = 1
    launch; two calls and the call without the map give bitwise equal sums; a buffer that is 4- but not 16-byte aligned gives the same bits"""
    from iris_amd.utils.metrics import image_metrics
    H, W = hw
    ref = reference(H, W, C)
    names = ("noise", "half_dark", "step")
    a, b = T(np.stack([ref[n][0] for n in names])), T(np.stack([ref[n][1] for n in names]))
    got = image_metrics(a, b, 1.0, full=True)
    again = image_metrics(a, b, 1.0, full=True)
    plain = image_metrics(a, b, 1.0)
    assert "ssim_map" not in plain and got["ssim"].shape == (3,)
    assert torch.equal(got["sums"].view(torch.int64), again["sums"].view(torch.int64))
    assert torch.equal(got["sums"].view(torch.int64), plain["sums"].view(torch.int64))
    assert torch.equal(got["ssim_map"].view(torch.int32), again["ssim_map"].view(torch.int32))
    for i, n in enumerate(names):
        _, _, R, S64, m64, S32, m32, mse64 = ref[n]
        check(f"stack[{i}] {n}", {k: v[i] for k, v in got.items()}, S64, m64, S32, m32, mse64, H, W, C, R)
        single = image_metrics(a[i], b[i], 1.0)
        assert torch.equal(single["sums"][0].view(torch.int64), got["sums"][i].view(torch.int64)), n
    buf_a, buf_b = torch.empty(a.numel() + 1, device=DEV), torch.empty(b.numel() + 3, device=DEV)
    ua, ub = buf_a[1:].view(a.shape), buf_b[3:].view(b.shape)
    ua.copy_(a); ub.copy_(b)
    assert ua.data_ptr() % 16 and ub.data_ptr() % 16 and ua.is_contiguous()
    shifted = image_metrics(ua, ub, 1.0, full=True)
    assert torch.equal(shifted["sums"].view(torch.int64), got["sums"].view(torch.int64))
    assert torch.equal(shifted["ssim_map"].view(torch.int32), got["ssim_map"].view(torch.int32))


def test_identical_images():
    from iris_amd.utils.metrics import image_metrics, psnr_device, ssim
    for C in (1, 3):
        for name, (a, _, R, *_rest) in reference(21, 139, C).items():
            got = image_metrics(T(a), T(a), R)
            assert abs(1.0 - float(got["ssim"].cpu())) <= 1e-7 and float(got["psnr"].cpu()) == np.inf, (name, C)
    a = T(reference(8, 9, 3)["noise"][0])
    assert abs(1.0 - ssim(a, a)) <= 1e-7 and psnr_device(a, a) == np.inf


def test_nan_pixel_stays_in_its_image():
    from iris_amd.utils.metrics import image_metrics
    ref = reference(21, 139, 3)
    a = np.stack([ref[n][0] for n in ("noise", "smooth", "step")])
    b = np.stack([ref[n][1] for n in ("noise", "smooth", "step")])
    clean = image_metrics(T(a), T(b))
    a = a.copy(); a[1, 10, 70, 2] = np.nan
    got = image_metrics(T(a), T(b), full=True)
    ssim = got["ssim"].cpu().numpy()
    assert np.isnan(ssim[1]) and np.isfinite(ssim[[0, 2]]).all()
    assert torch.equal(got["sums"][[0, 2]].view(torch.int64), clean["sums"][[0, 2]].view(torch.int64))
    m = got["ssim_map"][1].cpu().numpy()
    bad = np.isnan(m)
    assert bad[4:11, 64:71, 2].all() and bad.sum() == 49                     # exactly the windows that hold the pixel, in its channel
    assert np.isfinite(got["sums"][1, :2].cpu().numpy()).all()                # the other channels of that image stay finite


def test_bad_arguments_raise():
    from iris_amd import _lib as L
    from iris_amd.utils.metrics import image_metrics
    ok = torch.rand(9, 9, 3, device=DEV)
    for a, b in ((torch.rand(6, 9, 3, device=DEV),) * 2, (torch.rand(9, 6, 3, device=DEV),) * 2, (torch.rand(9, 9, 2, device=DEV),) * 2,
                 (ok, torch.rand(9, 10, 3, device=DEV)), (ok.double(), ok.double()), (torch.rand(2, 2, 9, 9, 3, device=DEV),) * 2):
        with pytest.raises(L.IrisError) as e:
            image_metrics(a, b)
        assert str(e.value)
    with pytest.raises(L.IrisError):
        image_metrics(ok, ok, data_range=0.0)
    with pytest.raises(L.IrisError):
        image_metrics(ok.clone().requires_grad_(), ok)
    with torch.no_grad():
        image_metrics(ok.clone().requires_grad_(), ok)
    lib = L.lib()
    assert lib.iris_image_metrics_workspace_bytes(1, 6, 9, 3) == 0 and lib.iris_image_metrics_workspace_bytes(1, 9, 9, 2) == 0
    assert lib.iris_image_metrics_workspace_bytes(0, 9, 9, 3) == 0
    assert lib.iris_image_metrics_workspace_bytes(2, 21, 139, 3) == 2 * 6 * 3 * 2 * 8
    sums, ws = torch.zeros(1, 3, 2, dtype=torch.float64, device=DEV), torch.zeros(64, dtype=torch.float64, device=DEV)
    rc = lib.iris_image_metrics(L.ptr(ok), L.ptr(ok), 1, 9, 9, 3, 1.0, L.ptr(sums), None, L.ptr(ws), 0, L.stream())
    assert rc != 0 and b"workspace" in lib.iris_last_error()
    with pytest.raises(L.IrisError):
        L.check(lib.iris_image_metrics(L.ptr(ok), L.ptr(ok), 1, 9, 9, 3, 1.0, L.ptr(sums), None, None, 0, L.stream()))
    torch.cuda.synchronize()
    assert float(sums.abs().sum()) == 0.0                                      # nothing was launched
