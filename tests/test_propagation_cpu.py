"""Argument checks of iris_amd/utils/propagation.py that need no GPU: CPU tensors are refused (there is no CPU path), and shape errors are reported
before any tensor is touched.  That the new entry points are declared, exported and bound consistently is tests/test_abi.py's job."""
import pytest
import torch

from iris_amd import _lib as L
from iris_amd.utils import propagation as P

KW = dict(sigma_albedo=0.05 / 3, sigma_pos=0.1, ls=1e-3)


def _inputs(n=6):
    return torch.rand(n, 1), torch.rand(n, 1), torch.rand(n, 3), torch.rand(n, 3), torch.arange(n) // 2


def test_cpu_tensors_raise():
    r, m, a, p, seg = _inputs()
    with pytest.raises(L.IrisError):
        P.semantic_propagation_loss(r, m, a, p, seg, **KW)
    with pytest.raises(L.IrisError):
        P.part_propagation_loss(r, m, seg, lp=5e-3)
    with pytest.raises(L.IrisError):
        P.propagation_draws(seg, 8, 0)
    with pytest.raises(L.IrisError):                       # an empty batch is no exception
        P.part_propagation_loss(r[:0], m[:0], seg[:0], lp=5e-3)


def test_mismatched_lengths_raise_value_error():
    r, m, a, p, seg = _inputs()
    for bad in ((r[:5], m, a, p, seg), (r, m[:5], a, p, seg), (r, m, a[:5], p, seg), (r, m, a, p[:5], seg), (r, m, a, p, seg[:5])):
        with pytest.raises(ValueError):
            P.semantic_propagation_loss(*bad, **KW)
    with pytest.raises(ValueError):
        P.semantic_propagation_loss(r, m, a, p, seg, draws=torch.zeros(6, 7, dtype=torch.int64), n_samples=8, **KW)
    with pytest.raises(ValueError):
        P.part_propagation_loss(r, m[:5], seg, lp=5e-3)
    with pytest.raises(ValueError):
        P.part_propagation_loss(r, m, seg[:5], lp=5e-3)


def test_n_samples_below_one_raises_value_error():
    r, m, a, p, seg = _inputs()
    for k in (0, -3):
        with pytest.raises(ValueError):
            P.semantic_propagation_loss(r, m, a, p, seg, n_samples=k, **KW)
        with pytest.raises(ValueError):
            P.propagation_draws(seg, k, 0)


def test_voxel_bounds_go_together():
    r, m, a, p, seg = _inputs()
    with pytest.raises(ValueError):
        P.semantic_propagation_loss(r, m, a, p, seg, voxel_min=-1.0, **KW)


def test_positions_that_require_grad_raise():
    r, m, a, p, seg = _inputs()
    with pytest.raises(L.IrisError, match="requires grad"):
        P.semantic_propagation_loss(r, m, a, p.requires_grad_(True), seg, **KW)
