"""The photometric step loss on the GPU (iris_loss_photometric through iris_amd.utils.losses.photometric_loss) against float64 over the float32 pieces the
existing entry points return: rgb = EmorCRF.forward(L_sum / n, e) and `slope e` = iris_crf_bwd on a cotangent of ones (tests/photometric_ref64.from_pieces).

Sizes: one lane; 63 / 64 / 65 rays (both sides of a wave boundary); 257 (a second workgroup); 8195 (33 workgroup partials for the last reduction level).
Tolerances: the gradient ((2 d) / (3 B)) * (slope e) / n is four float32 roundings of half an ulp each over exact inputs, (1 + 2^-24)^4 - 1 < 2.4e-7: 3e-7
relative, absolute against the smallest normal where the exact value lies below float32's normal range; the loss is summed in double and rounded once: 2^-23;
the psnr is the formula on that float32 loss: 1e-5 dB."""
import numpy as np
import pytest
import torch

import photometric_ref64 as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = [1, 63, 64, 65, 257, 8195]
TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def crf():
    from iris_amd.model.crf import EmorCRF
    s = torch.linspace(0, 1, 256)
    m = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)]))
    with torch.no_grad():
        m.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    m.weight.requires_grad_(False)
    return m.to(DEV)


def inputs(B, n_calls, exposure):
    """L_sum / n spread over [-0.5, 2.5) with exact zeros, negatives and values that saturate after the exposure; every third ray of the larger batches at 0"""
    g = torch.Generator().manual_seed(1000 * B + 10 * n_calls + len(exposure))
    L_sum = (torch.rand(B, 3, generator=g) * 3 - 0.5) * n_calls
    L_sum[::3, 0] = 0.0
    if B > 4:
        L_sum[1] = torch.tensor([-2.0, 0.0, 50.0]) * n_calls
        L_sum[2] = 0.0
    gt = torch.rand(B, 3, generator=g)
    e = {"number": 0.8, "one": torch.tensor([1.3]), "per_ray": 0.4 + torch.rand(B, 1, generator=g)}[exposure]
    return L_sum.to(DEV), gt.to(DEV), (e.to(DEV) if torch.is_tensor(e) else e)


def pieces(crf, L_sum, n_calls, e):
    """(rgb, slope e, L e) through the existing entry points: the forward lookup and its backward on ones"""
    L = (L_sum / n_calls).requires_grad_(True)
    rgb = crf(L, e)
    (se,) = torch.autograd.grad(rgb, L, torch.ones_like(rgb))
    return rgb.detach(), se, (L.detach() * (e if not torch.is_tensor(e) else e.reshape(-1, 1)))


def run(crf, L_sum, n_calls, e, gt):
    from iris_amd.utils.losses import photometric_loss
    x = L_sum.clone().requires_grad_(True)
    out = photometric_loss(x, n_calls, crf=crf, exposure=e, rgbs_gt=gt)
    assert out["loss_c"].shape == () and out["psnr"].shape == () and out["loss_c"].requires_grad and not out["psnr"].requires_grad
    out["loss_c"].backward()
    return out["loss_c"].detach(), out["psnr"].detach(), x.grad


@pytest.mark.parametrize("exposure", ["number", "one", "per_ray"])
@pytest.mark.parametrize("n_calls", [1, 4])
@pytest.mark.parametrize("B", SIZES)
def test_loss_psnr_and_gradient_against_float64_over_the_float32_pieces(crf, B, n_calls, exposure):
    L_sum, gt, e = inputs(B, n_calls, exposure)
    rgb, se, xe = pieces(crf, L_sum, n_calls, e)
    want_loss, _, want_g = P.from_pieces(rgb, gt, se, n_calls)
    loss, psnr, grad = run(crf, L_sum, n_calls, e, gt)
    got_loss, got_g = float(loss.double()), grad.double().cpu().numpy()
    err_loss = abs(got_loss - want_loss) / want_loss
    err_g = float((np.abs(got_g - want_g) / np.maximum(np.abs(want_g), TINY)).max())
    err_psnr = abs(float(psnr) - P.psnr_of(np.float32(got_loss)))
    clamped = ((xe < 0) | (xe > 1)).cpu().numpy()
    print(f"B {B} n_calls {n_calls} exposure {exposure}: loss {got_loss:.9g} rel err {err_loss:.3g}; gradient worst rel err {err_g:.3g}; psnr err {err_psnr:.3g} dB; "
          f"{int(clamped.sum())} of {clamped.size} entries clamp")
    assert err_loss <= 2.0 ** -23
    assert err_g <= 3e-7
    assert err_psnr <= 1e-5
    assert not got_g[clamped].any()                                  # the gradient is zero where the response model clamps
    if B > 4:
        assert clamped.any() and (~clamped).any() and np.abs(got_g[~clamped]).max() > 0


@pytest.mark.parametrize("B", SIZES)
def test_two_calls_agree_bit_for_bit_and_backward_scales(crf, B):
    from iris_amd.utils.losses import photometric_loss
    L_sum, gt, e = inputs(B, 4, "per_ray")
    a, b = run(crf, L_sum, 4, e, gt), run(crf, L_sum, 4, e, gt)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    x = L_sum.clone().requires_grad_(True)
    (photometric_loss(x, 4, crf=crf, exposure=e, rgbs_gt=gt)["loss_c"] * 3.0).backward()
    assert torch.equal(x.grad, 3.0 * a[2])                           # backward is grad_out * dL_sum
    # in a no-grad region, and for an input that asks for no gradient, the numbers are the same
    with torch.no_grad():
        out = photometric_loss(L_sum, 4, crf=crf, exposure=e, rgbs_gt=gt)
    assert torch.equal(out["loss_c"], a[0]) and torch.equal(out["psnr"], a[1]) and not out["loss_c"].requires_grad


def test_a_perfect_fit_has_zero_loss_and_the_clamped_psnr(crf):
    L_sum, _, e = inputs(257, 4, "per_ray")
    with torch.no_grad():
        gt = crf(L_sum / 4, e)
    loss, psnr, grad = run(crf, L_sum, 4, e, gt)
    assert float(loss) == 0.0 and float(psnr) == 50.0 and not grad.any()


def test_rows_that_are_not_contiguous_and_a_trainable_response(crf):
    from iris_amd import _lib as L
    from iris_amd.utils.losses import photometric_loss
    L_sum, gt, e = inputs(65, 1, "one")
    wide = torch.zeros(65, 5, device=DEV)
    wide[:, 1:4] = L_sum
    a = photometric_loss(wide[:, 1:4], 1, crf=crf, exposure=e, rgbs_gt=gt)
    b = photometric_loss(L_sum, 1, crf=crf, exposure=e, rgbs_gt=gt)
    assert torch.equal(a["loss_c"], b["loss_c"])
    crf.weight.requires_grad_(True)
    try:
        with pytest.raises(L.IrisError, match="initialize_loss"):
            photometric_loss(L_sum, 1, crf=crf, exposure=e, rgbs_gt=gt)
    finally:
        crf.weight.requires_grad_(False)
