"""Helper (not a test): the trainers' albedo regulariser (train_brdf_crf.py:292-306 with utils/loss.py:14-37; initialize.py:188-201) restated on the CPU.

The reference's training steps cannot be imported here (Lightning, Mitsuba, torch_scatter), so the yardstick is this restatement: the reference's lines
with ``index_add`` in the place of ``torch_scatter.scatter(reduce='sum')``, run in a given dtype.  float64 is the reference of the GPU tests; the float32
run of the SAME lines measures d32, the deviation those tests' tolerances are built from.

albedo_restatement   (loss, grad_albedo, k) of one mode; k is 1.0 in mode mse
scale_invariant_mse  utils/loss.py:14-20,33-37 on its own: what test_losses_cpu.py holds the restatement against
make_inputs / case   the inputs the tests share (seeded) and their restatements, computed once
"""
import functools

import torch


def scale_invariant_mse(source, target):
    """utils/loss.py:33-37 with compute_scale (:14-20): the scale of `source` that fits `target`, fetched to the host, then the mse"""
    s, t = source.reshape(-1), target.reshape(-1)
    scale = (torch.dot(s, t) / torch.dot(s, s)).item()
    return torch.nn.functional.mse_loss(source * scale, target)


def segment_mean(prior, seg):
    """train_brdf_crf.py:294-303 / initialize.py:189-200: the prior's mean over every pixel's segment, with unit weights"""
    seg_idxs, inv_idxs = seg.unique(return_inverse=True)
    weight_seg_ = torch.ones(prior.shape[0], dtype=prior.dtype)
    weight_seg = torch.zeros(len(seg_idxs), dtype=prior.dtype).index_add(0, inv_idxs, weight_seg_).unsqueeze(-1)
    mean = torch.zeros(len(seg_idxs), 3, dtype=prior.dtype).index_add(0, inv_idxs, prior * weight_seg_.unsqueeze(-1))
    mean = mean / weight_seg
    return mean[inv_idxs]


def albedo_restatement(albedo, prior, seg, dtype, scale_invariant, weight=1.0, detach_scale=True):
    """(loss, grad_albedo (N, 3), k) in `dtype` on the CPU.  detach_scale=False keeps the scale in the graph (what the reference's .item() prevents)."""
    a = albedo.to(dtype).clone().requires_grad_(True)
    tbar = segment_mean(prior.to(dtype), seg)
    if not scale_invariant:
        k = 1.0
        loss = weight * torch.nn.functional.mse_loss(a, tbar)
    elif detach_scale:
        s, t = tbar.reshape(-1), a.reshape(-1)
        k = (torch.dot(s, t) / torch.dot(s, s)).item()
        loss = weight * torch.nn.functional.mse_loss(tbar * k, a)
    else:
        s, t = tbar.reshape(-1), a.reshape(-1)
        scale = torch.dot(s, t) / torch.dot(s, s)
        k = scale.item()
        loss = weight * torch.nn.functional.mse_loss(tbar * scale, a)
    loss.backward()
    return loss.detach(), a.grad, k


CASES = {"small": (1, 2, 39, 40, 41, 64, 146),       # N = 333: a singleton, runs below, at and above a wave, N no multiple of 64
         "multi": (4097, 4095, 1),                     # N = 8193: runs across many workgroups, long lane-strided chains, N no multiple of 256
         "stride": (13107,) * 80 + (316,)}             # N = 1 048 876 > 4096 x 256: some threads take two positions, the last passes add 16 partials per thread
BIG_ID = 2 ** 40 + 5                                   # one segment's id: a key truncated to 32 bits shows
LA = 0.01


def make_inputs(sizes, seed):
    """Segments of the given sizes with ids 7k+3 (segment 1: 2^40 + 5) in shuffled pixel order; albedo uniform in [0.05, 0.95]; the prior k / 255,
    k uniform in 0..255 (what the loaders read from PNG); roughness, metallic and positions for the step losses."""
    g = torch.Generator().manual_seed(seed)
    ids = [BIG_ID if k == 1 else 7 * k + 3 for k in range(len(sizes))]
    seg = torch.cat([torch.full((c,), i, dtype=torch.int64) for i, c in zip(ids, sizes)])
    seg = seg[torch.randperm(seg.numel(), generator=g)]
    N = seg.numel()
    return dict(seg=seg, sizes=tuple(sizes),
                albedo=(0.05 + 0.9 * torch.rand(N, 3, generator=g, dtype=torch.float64)).float(),
                prior=torch.randint(0, 256, (N, 3), generator=g).float() / 255.0,
                r=(0.02 + 0.98 * torch.rand(N, 1, generator=g, dtype=torch.float64)).float(),
                m=torch.rand(N, 1, generator=g, dtype=torch.float64).float(),
                pos=((torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.15).float())


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, {mode: (ref64, ref32)}) of a case, mode in ("mse", "scale_invariant"); computed once and shared (never modified)"""
    d = make_inputs(CASES[name], seed=11 + len(name))
    refs = {}
    for mode, si, w in (("mse", False, 1.0), ("scale_invariant", True, LA)):
        refs[mode] = tuple(albedo_restatement(d["albedo"], d["prior"], d["seg"], dt, si, w) for dt in (torch.float64, torch.float32))
    return d, refs
