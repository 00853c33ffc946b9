"""The BRDF trainer's roughness-metallic propagation regulariser (reference: train_brdf_crf.py:212-290) as fused HIP kernels.

The reference's semantic branch (``has_part == 0``, :243-290) loops over the segments of the batch on the host, draws 1024 partners per pixel from the
pixel's own segment, materialises the pair lists (8.4 M rows at a batch of 8192) and a dozen intermediates of that length; its part branch (``has_part == 1``,
:216-238) needs ``torch_scatter``.  Here both are a handful of kernels over the batch sorted by segment id (iris_amd/csrc/iris_prop.h), differentiable in
``roughness`` and ``metallic``; nothing goes to the host between the call and the returned scalar.

    loss_seg = semantic_propagation_loss(roughness, metallic, albedo, positions, segmentation, sigma_albedo=..., sigma_pos=..., ls=...,
                                         seed=global_step, voxel_min=material.voxel_min, voxel_max=material.voxel_max)
    loss_seg = part_propagation_loss(roughness, metallic, segmentation, lp=...)

The random draws are Philox4x32-10 words keyed on (seed, pixel, draw), not torch's generator: parity unpinned.  ``draws=`` takes recorded local ranks
instead (what the reference's ``torch.randint(0, c, ...)`` returned), which pins the arithmetic against a restatement.
"""
import torch

from .. import _lib as L


class SegmentRuns:
    """The batch sorted by segment id: ``order`` (N int64, torch.sort(stable=True): a segment's pixels stay in ascending index, the order of the
    reference's torch.where) and ``runs`` (N x 2 int32: start and count of the run every sorted position lies in).  Shared by both branches."""

    def __init__(self, segmentation):
        seg = L.require_gpu(segmentation.reshape(-1), torch.int64, "segmentation")
        self.n = seg.shape[0]
        keys, self.order = torch.sort(seg, stable=True)
        self.runs = torch.empty(self.n, 2, device=seg.device, dtype=torch.int32)
        with torch.cuda.device(seg.device):
            L.check(L.lib().iris_prop_runs(L.ptr(keys), self.n, L.ptr(self.runs), L.stream()))


def _runs(segmentation):
    return segmentation if isinstance(segmentation, SegmentRuns) else SegmentRuns(segmentation)


def _flat(t, name):
    return L.require_gpu(t.detach().reshape(-1), torch.float32, name)


def _lengths(segmentation, **tensors):
    """N, after checking that every tensor (name=(tensor, entries per pixel)) has that many pixels: shapes only, so it runs before any tensor is touched"""
    N = segmentation.n if isinstance(segmentation, SegmentRuns) else segmentation.numel()
    for name, (t, per) in tensors.items():
        if t.numel() != N * per:
            raise ValueError(f"{name} has {t.numel()} entries, expected {N} x {per} (segmentation has {N} pixels)")
    return N


def propagation_draws(segmentation, n_samples=1024, seed=0):
    """(N, n_samples) int64: the local ranks semantic_propagation_loss(seed=seed) draws, row i for pixel i, each in [0, size of i's segment)."""
    if int(n_samples) < 1:
        raise ValueError("n_samples must be at least 1")
    sr = _runs(segmentation)
    draws = torch.empty(sr.n, int(n_samples), device=sr.order.device, dtype=torch.int64)
    with torch.cuda.device(draws.device):
        L.check(L.lib().iris_prop_draws(L.ptr(sr.runs), L.ptr(sr.order), sr.n, int(n_samples), int(seed) & (2 ** 64 - 1), L.ptr(draws), L.stream()))
    return draws


class _Semantic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, roughness, metallic, albedo, positions, sr, draws, cfg):
        N, dev = sr.n, sr.order.device
        r, m = _flat(roughness, "roughness"), _flat(metallic, "metallic")
        K, seed, sa, sp, ls, norm, vmin, vmax = cfg
        records = torch.empty(N, 8, device=dev, dtype=torch.float32)
        saved = torch.empty(N, 4, device=dev, dtype=torch.float32)
        terms = torch.empty(N, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_prop_semantic_fwd(L.ptr(sr.runs), L.ptr(sr.order), L.ptr(r), L.ptr(m), L.ptr(albedo), L.ptr(positions), N, K, L.ptr(draws),
                                                   seed, sa, sp, norm, vmin, vmax, ls, L.ptr(records), L.ptr(saved), L.ptr(terms), L.ptr(loss), L.stream()))
        ctx.save_for_backward(sr.runs, sr.order, records, saved, draws if draws is not None else torch.empty(0, device=dev, dtype=torch.int64))
        ctx.cfg, ctx.has_draws, ctx.shapes = cfg, draws is not None, (roughness.shape, metallic.shape)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        runs, order, records, saved, draws = ctx.saved_tensors
        K, seed, sa, sp, ls = ctx.cfg[:5]
        N, dev = order.shape[0], order.device
        g_loss = L.require_gpu(g_loss.reshape(1), torch.float32, "g_loss")
        g_sorted = torch.empty(2 * N, device=dev, dtype=torch.float32)
        gr = torch.empty(N, device=dev, dtype=torch.float32)
        gm = torch.empty(N, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_prop_semantic_bwd(L.ptr(runs), L.ptr(order), L.ptr(records), L.ptr(saved), N, K, L.ptr(draws) if ctx.has_draws else None,
                                                   seed, sa, sp, ls, L.ptr(g_loss), L.ptr(g_sorted), L.ptr(gr), L.ptr(gm), L.stream()))
        rs, ms = ctx.shapes
        return gr.reshape(rs), gm.reshape(ms), None, None, None, None, None


def semantic_propagation_loss(roughness, metallic, albedo, positions, segmentation, *, sigma_albedo, sigma_pos, ls, n_samples=1024, seed=0, draws=None,
                              voxel_min=None, voxel_max=None):
    """train_brdf_crf.py:243-290 -> 0-d float32 tensor, differentiable in roughness and metallic (N or N x 1).

    albedo (N x 3) is detached (the reference's ``.data``); positions (N x 3) never get a gradient and raise if they require one.  With voxel_min and
    voxel_max the positions are normalised to [-1, 1] as :244 does, otherwise they are taken as normalised.  segmentation: (N,) int64 ids, or a
    SegmentRuns built from them.  A pixel whose segment has c < n_samples members is paired with all c members once each; otherwise with n_samples
    members drawn with replacement: local rank ``draws[i, k]`` ((N, n_samples) int64, clamped into [0, c)) when draws is given, else Philox keyed on
    (seed, i, k) -- the ranks ``propagation_draws`` returns; the trainer passes seed=global_step.  The forward is bitwise reproducible for given draws;
    the gradient sums with float atomics and is reproducible up to the order of those sums."""
    K = int(n_samples)
    if K < 1:
        raise ValueError("n_samples must be at least 1")
    if (voxel_min is None) != (voxel_max is None):
        raise ValueError("voxel_min and voxel_max go together")
    N = _lengths(segmentation, roughness=(roughness, 1), metallic=(metallic, 1), albedo=(albedo, 3), positions=(positions, 3))
    if draws is not None and tuple(draws.shape) != (N, K):
        raise ValueError(f"draws has shape {tuple(draws.shape)}, expected {(N, K)}")
    L.no_autograd("semantic_propagation_loss", positions)
    sr = _runs(segmentation)
    for name, t in (("roughness", roughness), ("metallic", metallic)):
        L.require_gpu(t, torch.float32, name)
    albedo = L.require_gpu(albedo.detach(), torch.float32, "albedo").reshape(-1, 3)
    positions = L.require_gpu(positions.detach(), torch.float32, "positions").reshape(-1, 3)
    if draws is not None:
        draws = L.require_gpu(draws, torch.int64, "draws")
    if N == 0:
        return (roughness.sum() + metallic.sum()) * 0.0
    norm = voxel_min is not None
    cfg = (K, int(seed) & (2 ** 64 - 1), float(sigma_albedo), float(sigma_pos), float(ls), int(norm), float(voxel_min) if norm else 0.0,
           float(voxel_max) if norm else 1.0)
    return _Semantic.apply(roughness, metallic, albedo, positions, sr, draws, cfg)


class _Part(torch.autograd.Function):
    @staticmethod
    def forward(ctx, roughness, metallic, sr, lp):
        N, dev = sr.n, sr.order.device
        r, m = _flat(roughness, "roughness"), _flat(metallic, "metallic")
        means = torch.empty(N, 4, device=dev, dtype=torch.float32)
        signs = torch.empty(N, 2, device=dev, dtype=torch.float32)
        terms = torch.empty(N, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_prop_part_fwd(L.ptr(sr.runs), L.ptr(sr.order), L.ptr(r), L.ptr(m), N, lp, L.ptr(means), L.ptr(signs), L.ptr(terms), L.ptr(loss),
                                               L.stream()))
        ctx.save_for_backward(sr.runs, sr.order, r, means, signs)
        ctx.lp, ctx.shapes = lp, (roughness.shape, metallic.shape)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        runs, order, r, means, signs = ctx.saved_tensors
        N, dev = order.shape[0], order.device
        g_loss = L.require_gpu(g_loss.reshape(1), torch.float32, "g_loss")
        gr = torch.empty(N, device=dev, dtype=torch.float32)
        gm = torch.empty(N, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_prop_part_bwd(L.ptr(runs), L.ptr(order), L.ptr(r), L.ptr(means), L.ptr(signs), N, ctx.lp, L.ptr(g_loss), L.ptr(gr), L.ptr(gm),
                                               L.stream()))
        rs, ms = ctx.shapes
        return gr.reshape(rs), gm.reshape(ms), None, None


def part_propagation_loss(roughness, metallic, segmentation, *, lp):
    """train_brdf_crf.py:216-238 without torch_scatter -> 0-d float32 tensor: lp * (mean |m - M_s| + mean |r - R_s|) with the segment means M_s, R_s weighted
    by (1 - r) + 1e-4 (detached).  Differentiable in roughness and metallic through the deviations and the means' numerators, not through the weights.
    No atomics: forward and gradient are bitwise reproducible."""
    N = _lengths(segmentation, roughness=(roughness, 1), metallic=(metallic, 1))
    sr = _runs(segmentation)
    for name, t in (("roughness", roughness), ("metallic", metallic)):
        L.require_gpu(t, torch.float32, name)
    if N == 0:
        return (roughness.sum() + metallic.sum()) * 0.0
    return _Part.apply(roughness, metallic, sr, float(lp))
