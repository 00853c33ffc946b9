"""The trainers' step losses (reference: train_brdf_crf.py:192-314, initialize.py:165-202) and their albedo regulariser as fused HIP kernels.

The reference builds the albedo term from a ``segmentation.unique``, three ``torch_scatter.scatter`` calls and, in the BRDF-CRF trainer,
``compute_scale(...).item()`` (utils/loss.py:14-20): a host round trip in every step.  Here it is four kernels over the batch sorted by segment id
(iris_amd/csrc/iris_loss.h), the sorted batch shared with the propagation regulariser, differentiable in ``albedo``; the scale stays on the device.

    out = brdf_crf_loss(material(positions), cache=cache, idx=idx, crf=model_crf, exposure=exposure, rgbs_gt=rgbs_gt, segmentation=segmentation,
                        positions=positions, albedo_prior=int_albedo, has_part=0, la=0.01, seed=global_step,
                        voxel_min=material.voxel_min, voxel_max=material.voxel_max)
    out = initialize_loss(mat['albedo'], L, crf=model_crf, exposure=exposure, rgbs_gt=rgbs_gt, albedo_prior=int_albedo, segmentation=segmentation)
    out['loss'].backward()
    out = photometric_loss(L_sum, SPP // spp, crf=model_crf, exposure=exposure, rgbs_gt=rgbs_gt)        # the response model frozen: loss_c, psnr

A trainer stage is a data loader (``iris_amd.utils.dataset.PixelSet``), ``torch.optim.Adam`` and a checkpoint writer around one of these calls; the
``valid`` filtering of the batch is the caller's (``PixelSet.restrict_to_hits`` makes every batch all-valid).  Every returned entry is a device tensor: logging them is the caller's synchronisation, not the step's.
"""
import torch

from .. import _lib
from .propagation import _lengths, _runs, part_propagation_loss, semantic_propagation_loss

_BLOCK, _MAX_BLOCKS = 256, 4096          # iris_loss.h: one partial per 256 positions, 4096 at the most


class _SegmentAlbedo(torch.autograd.Function):
    """saved_tensors = (runs, order, albedo, seg_means, k): k is the 1-element device tensor holding the scale (1 in mode mse)"""

    @staticmethod
    def forward(ctx, albedo, prior, sr, weight, scale_invariant):
        N, dev = sr.n, sr.order.device
        a = _lib.require_gpu(albedo.detach(), torch.float32, "albedo").reshape(-1, 3)
        means = torch.empty(N, 4, device=dev, dtype=torch.float32)
        partials = torch.empty(3 * min((N + _BLOCK - 1) // _BLOCK, _MAX_BLOCKS), device=dev, dtype=torch.float32)
        k = torch.empty(1, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().iris_loss_albedo_fwd(_lib.ptr(sr.runs), _lib.ptr(sr.order), _lib.ptr(a), _lib.ptr(prior), N, int(scale_invariant), weight,
                                                       _lib.ptr(means), _lib.ptr(partials), _lib.ptr(k), _lib.ptr(loss), _lib.stream()))
        ctx.save_for_backward(sr.runs, sr.order, a, means, k)
        ctx.weight, ctx.shape = weight, albedo.shape
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        runs, order, a, means, k = ctx.saved_tensors
        N, dev = order.shape[0], order.device
        g_loss = _lib.require_gpu(g_loss.reshape(1), torch.float32, "g_loss")
        ga = torch.empty(N, 3, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().iris_loss_albedo_bwd(_lib.ptr(runs), _lib.ptr(order), _lib.ptr(a), _lib.ptr(means), _lib.ptr(k), N, ctx.weight,
                                                       _lib.ptr(g_loss), _lib.ptr(ga), _lib.stream()))
        return ga.reshape(ctx.shape), None, None, None, None


def segment_albedo_loss(albedo, albedo_prior, segmentation, *, weight=1.0, scale_invariant=False):
    """The albedo regulariser -> 0-d float32 tensor, differentiable in albedo (N x 3); albedo_prior (N x 3) is detached.

    With tbar_i the mean of the prior over pixel i's segment (train_brdf_crf.py:294-303, initialize.py:191-200; the weights there are all ones):
      scale_invariant=False   weight * mean (albedo - tbar)^2                                                   (initialize.py:201)
      scale_invariant=True    weight * mean (k tbar - albedo)^2, k = sum(tbar albedo) / sum(tbar tbar)          (train_brdf_crf.py:305-306, utils/loss.py:33-37)
    k is a constant of the backward, as the reference's ``.item()`` makes it (it is the least-squares scale, so its own gradient term vanishes anyway);
    it is computed and consumed on the device.  A prior that is zero everywhere gives k = NaN and a NaN loss, as the reference does.
    segmentation: (N,) int64 ids, or a SegmentRuns built from them (a step that also calls a propagation loss then sorts once).  No atomics: loss and
    gradient are bitwise reproducible."""
    N = _lengths(segmentation, albedo=(albedo, 3), albedo_prior=(albedo_prior, 3))
    _lib.require_gpu(albedo, torch.float32, "albedo")
    prior = _lib.require_gpu(albedo_prior.detach(), torch.float32, "albedo_prior").reshape(-1, 3)
    sr = _runs(segmentation)
    if N == 0:
        return albedo.sum() * 0.0
    return _SegmentAlbedo.apply(albedo, prior, sr, float(weight), bool(scale_invariant))


def diffuse_regulariser(roughness, metallic, *, ld):
    """train_brdf_crf.py:210: ld * (mean |roughness - 1| + mean metallic).  Plain torch on purpose: there are no segments here, and four tiny
    elementwise ops and two means leave nothing to fuse that a test could tell apart."""
    return ld * ((roughness - 1).abs().mean() + metallic.mean())


def _psnr(loss_c):
    return -10.0 * torch.log10(loss_c.detach().clamp_min(1e-5))


def _on_gpu(**tensors):
    for name, (t, dtype) in tensors.items():
        if t is not None:
            _lib.require_gpu(t, dtype, name)


def brdf_crf_loss(mat, *, cache, idx, crf, exposure, rgbs_gt, segmentation, positions, albedo_prior=None, has_part=1, ld=5e-4, lp=5e-3, ls=1e-3, la=0.0,
                  sigma_albedo=0.05 / 3.0, sigma_pos=0.3 / 3.0, l_crf_increasing=0.1, l_crf_weight=0.001, seed=0, voxel_min=None, voxel_max=None):
    """The BRDF-CRF trainer's step loss (train_brdf_crf.py:192-314) for already-valid pixels -> dict of 0-d device tensors with the names the
    reference logs: loss, loss_c, loss_d, loss_seg, loss_a, reg_crf, psnr.

    mat: the material network's output for the batch ({'albedo' (N x 3), 'metallic', 'roughness' (N x 1)}); cache / idx: the ShadingCache and the
    batch's rows in it (None = all rows in order); crf: the EmorCRF; exposure as EmorCRF.forward takes it; rgbs_gt (N x 3); segmentation: (N,) int64
    ids or a SegmentRuns (one is built per call otherwise, shared by the propagation and the albedo term); positions (N x 3) world positions, used by
    the semantic branch (has_part == 0; normalised with voxel_min / voxel_max as :244 when both are given; seed: the trainer's global step);
    albedo_prior (N x 3): the loader's ``int_albedo``, needed when la > 0.  The hyper-parameters default to configs/config.py.
    loss = loss_c + loss_d + loss_seg + loss_a + reg_crf in that order; loss_a is the constant 0 when la == 0; psnr carries no gradient."""
    albedo, metallic, roughness = mat["albedo"], mat["metallic"], mat["roughness"]
    if la > 0 and albedo_prior is None:
        raise ValueError("albedo_prior is needed when la > 0 (the loader's int_albedo)")
    shapes = dict(albedo=(albedo, 3), metallic=(metallic, 1), roughness=(roughness, 1), rgbs_gt=(rgbs_gt, 3), positions=(positions, 3))
    if idx is not None:
        shapes["idx"] = (idx, 1)
    if albedo_prior is not None:
        shapes["albedo_prior"] = (albedo_prior, 3)
    _lengths(segmentation, **shapes)
    f32 = torch.float32
    _on_gpu(albedo=(albedo, f32), metallic=(metallic, f32), roughness=(roughness, f32), rgbs_gt=(rgbs_gt, f32), positions=(positions, f32),
            albedo_prior=(albedo_prior, f32), idx=(idx, torch.int64))
    sr = _runs(segmentation)

    rgbs_ldr = crf(cache.shade(idx, albedo, metallic, roughness), exposure)
    loss_c = torch.nn.functional.mse_loss(rgbs_ldr, rgbs_gt.reshape(rgbs_ldr.shape))
    loss_d = diffuse_regulariser(roughness, metallic, ld=ld)
    if has_part:
        loss_seg = part_propagation_loss(roughness, metallic, sr, lp=lp)
    else:
        loss_seg = semantic_propagation_loss(roughness, metallic, albedo, positions, sr, sigma_albedo=sigma_albedo, sigma_pos=sigma_pos, ls=ls, seed=seed,
                                             voxel_min=voxel_min, voxel_max=voxel_max)
    if la > 0:
        loss_a = segment_albedo_loss(albedo, albedo_prior, sr, weight=la, scale_invariant=True)
    else:
        loss_a = torch.zeros((), device=loss_c.device, dtype=torch.float32)
    reg_crf = l_crf_increasing * crf.reg_monotonically_increasing() + l_crf_weight * crf.reg_weight()
    loss = loss_c + loss_d + loss_seg + loss_a + reg_crf
    return dict(loss=loss, loss_c=loss_c, loss_d=loss_d, loss_seg=loss_seg, loss_a=loss_a, reg_crf=reg_crf, psnr=_psnr(loss_c))


def initialize_loss(albedo, L, *, crf, exposure, rgbs_gt, albedo_prior, segmentation):
    """The initialisation stage's step loss (initialize.py:182-202) -> dict of 0-d device tensors: loss = loss_a + loss_c, loss_c, loss_a, psnr.

    L (N x 3) is the caller's ``path_tracing_single_step(...) / n_calls`` (the material network frozen around it, as :170-186); loss_a is the mse
    between albedo and the segment means of albedo_prior, weight 1: the only term through which this stage trains the material network."""
    shapes = dict(albedo=(albedo, 3), L=(L, 3), rgbs_gt=(rgbs_gt, 3), albedo_prior=(albedo_prior, 3))
    _lengths(segmentation, **shapes)
    _on_gpu(**{name: (t, torch.float32) for name, (t, _) in shapes.items()})
    rgbs_ldr = crf(L, exposure)
    loss_c = torch.nn.functional.mse_loss(rgbs_ldr, rgbs_gt.reshape(rgbs_ldr.shape))
    loss_a = segment_albedo_loss(albedo, albedo_prior, segmentation, weight=1.0, scale_invariant=False)
    return dict(loss=loss_a + loss_c, loss_c=loss_c, loss_a=loss_a, psnr=_psnr(loss_c))


class _Photometric(torch.autograd.Function):
    """loss and psnr of iris_loss_photometric; the call also leaves d loss / d L_sum, which the backward scales by the incoming gradient"""

    @staticmethod
    def forward(ctx, L_sum, n_calls, table, grid, e, n_exposure, exposure_value, gt):
        x = _lib.require_gpu(L_sum.detach(), torch.float32, "L_sum")
        B, n, dev = x.shape[0], table.shape[1], x.device
        lib = _lib.lib()
        loss, psnr = torch.empty((), device=dev, dtype=torch.float32), torch.empty((), device=dev, dtype=torch.float32)
        g = torch.empty(B, 3, device=dev, dtype=torch.float32)
        ws_bytes = lib.iris_loss_photometric_workspace_bytes(B)
        ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            _lib.check(lib.iris_loss_photometric(_lib.ptr(x), n_calls, _lib.ptr(grid), _lib.ptr(table), n, _lib.ptr(e), n_exposure, exposure_value, _lib.ptr(gt), B,
                                                 _lib.ptr(loss), _lib.ptr(psnr), _lib.ptr(g), _lib.ptr(ws), ws_bytes, _lib.stream()))
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(psnr)
        return loss, psnr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_psnr):
        g, = ctx.saved_tensors
        return (g_loss * g,) + (None,) * 7


def photometric_loss(L_sum, n_calls, *, crf, exposure, rgbs_gt):
    """The emitter and initialisation stages' photometric term (train_emitter.py:189-195, initialize.py:180-184, 206) with the response model frozen
    -> {'loss_c', 'psnr'}, 0-d device tensors: loss_c = mse_loss(crf(L_sum / n_calls, exposure), rgbs_gt), psnr = -10 log10(max(loss_c, 1e-5)).

    L_sum (B x 3): ``path_tracing_single_step(..., spp, n_calls)``, the integrator's sum before the reference's division by SPP // spp; exposure as
    EmorCRF.forward takes it; rgbs_gt (B x 3).  One call (iris_loss_photometric) computes the loss, the psnr and d loss_c / d L_sum in one pass over the
    batch, in place of the division, the lookup, the mse and their autograd nodes; differentiable in L_sum only (psnr carries no gradient), no atomics:
    loss and gradient are bitwise reproducible.  A response model that trains needs the gradient by its weights, which this call does not compute:
    IrisError -- use brdf_crf_loss / initialize_loss there."""
    from ..model.crf import _check_tables, _exposure_args
    if crf.weight.requires_grad:
        raise _lib.IrisError("photometric_loss: the response model is trainable (crf.weight.requires_grad) and this loss computes no gradient for it: freeze "
                             "it, or use brdf_crf_loss / initialize_loss for a trainable response model")
    n_calls = int(n_calls)
    if not 1 <= n_calls <= 1 << 24:
        raise _lib.IrisError(f"photometric_loss: n_calls = {n_calls}, expected 1 <= n_calls <= 2^24 (SPP // spp)")
    for name, t in (("L_sum", L_sum), ("rgbs_gt", rgbs_gt)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
            raise _lib.IrisError(f"photometric_loss: {name} has shape {tuple(getattr(t, 'shape', ()))}, expected (B, 3)")
    B = L_sum.shape[0]
    if B < 1 or rgbs_gt.shape[0] != B:
        raise _lib.IrisError(f"photometric_loss: L_sum holds {B} rays and rgbs_gt {rgbs_gt.shape[0]}: expected the same number, at least 1")
    if torch.is_tensor(exposure) and exposure.numel() not in (1, B):
        raise _lib.IrisError(f"photometric_loss: exposure has {exposure.numel()} values, expected 1 or {B} (one per ray)")
    _on_gpu(L_sum=(L_sum, torch.float32))
    gt = _lib.require_gpu(rgbs_gt.detach(), torch.float32, "rgbs_gt")
    if rgbs_gt.device != L_sum.device or crf.weight.device != L_sum.device:
        raise _lib.IrisError(f"photometric_loss: L_sum ({L_sum.device}), rgbs_gt ({rgbs_gt.device}) and the response model ({crf.weight.device}) must share a HIP device")
    with torch.no_grad():
        table, grid = _check_tables(crf.get_crf(), crf.grid)
    e, ne, ev = _exposure_args(exposure, B, L_sum.device)
    loss_c, psnr = _Photometric.apply(L_sum, n_calls, table, grid, e, ne, ev, gt)
    return dict(loss_c=loss_c, psnr=psnr)
