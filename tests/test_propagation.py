"""The roughness-metallic propagation regulariser (iris_amd/utils/propagation.py; reference train_brdf_crf.py:212-290) against a torch restatement.

The reference's training step cannot be imported here (Lightning, Mitsuba, torch_scatter), so the yardstick is the restatement below: the reference's lines
written with explicit pair lists built from the same recorded draws, run on the CPU in float64.  Tolerances come from the float32 run of the SAME
restatement (d32, its own deviation from float64) and from the first-order worst case of summing K non-negative float32 terms, K * 2^-24:
    loss:      |rel deviation| <= max(8 d32, K 2^-24)
    gradients: |deviation|     <= max(8 max|g32 - g64|, K 2^-24 max|g64|)   elementwise
Every pixel of the recorded-draw cases has |rbar - r| and |mbar - m| above 1e-5 in float64 (asserted), so no sign can differ between precisions and no
pixel is left out.  Figures for case 1 (seed 1): loss 2.03e-3 over 13 166 pairs, d32 3.4e-9, float32 restatement's gradient deviation 2.9e-11 at magnitude
3.5e-4; the kernels measured 3.4e-9 and 1.1e-11 on an MI355X (case 2: 6.3e-8 and 3.6e-12; two backward passes 1.8e-12 apart).
"""
import functools

import pytest
import torch

SIGMA_A, SIGMA_P, LS, LP = 0.05 / 3, 0.1, 1e-3, 5e-3


def make_inputs(sizes, K, seed):
    """Segments of the given sizes with ids 7k+3 in shuffled pixel order, inputs in the issue's ranges, and recorded local ranks for every pixel."""
    g = torch.Generator().manual_seed(seed)
    seg = torch.cat([torch.full((c,), 7 * k + 3, dtype=torch.int64) for k, c in enumerate(sizes)])
    seg = seg[torch.randperm(seg.numel(), generator=g)]
    N = seg.numel()
    d = dict(seg=seg, K=K,
             albedo=(0.4 + 0.05 * torch.rand(N, 3, generator=g, dtype=torch.float64)).float(),
             pos=((torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.15).float(),
             r=(0.02 + 0.98 * torch.rand(N, 1, generator=g, dtype=torch.float64)).float(),
             m=torch.rand(N, 1, generator=g, dtype=torch.float64).float())
    count = torch.zeros(int(seg.max()) + 1, dtype=torch.int64).index_add_(0, seg, torch.ones_like(seg))[seg]
    d["count"] = count
    d["draws"] = (torch.rand(N, K, generator=g, dtype=torch.float64) * count[:, None]).long().minimum(count[:, None] - 1)
    return d


def pair_lists(seg, K, draws):
    """ii, jj of train_brdf_crf.py:248-262, with draws[i, k] in the place of torch.randint's output"""
    ii, jj = [], []
    for s in seg.unique():
        i = torch.where(seg == s)[0]
        c = i.numel()
        if K > c:
            j = torch.arange(c)[None].repeat_interleave(c, 0).reshape(-1)
            n = c
        else:
            j = draws[i].reshape(-1)
            n = K
        jj.append(i[j]); ii.append(i.repeat_interleave(n, 0))
    return torch.cat(ii), torch.cat(jj)


def semantic_restatement(d, dtype):
    """(loss, g_r, g_m, |rbar - r|, |mbar - m|) of :243-290 in `dtype` on the CPU"""
    seg, K = d["seg"], d["K"]
    ii, jj = pair_lists(seg, K, d["draws"])
    a, p = d["albedo"].to(dtype), d["pos"].to(dtype)
    r, m = d["r"].to(dtype).clone().requires_grad_(True), d["m"].to(dtype).clone().requires_grad_(True)
    w = torch.exp(-((a[ii] - a[jj]).pow(2).sum(-1) / SIGMA_A ** 2) / 2.0)
    w = w * torch.exp(-((p[ii] - p[jj]).pow(2).sum(-1) / SIGMA_P ** 2) / 2.0)
    N = seg.numel()
    W = torch.zeros(N, dtype=dtype) + 1e-4
    W = W.index_add(0, ii, w)
    rbar = torch.zeros(N, dtype=dtype).index_add(0, ii, r[jj].squeeze(-1) * w) / W
    mbar = torch.zeros(N, dtype=dtype).index_add(0, ii, m[jj].squeeze(-1) * w) / W
    dr, dm = rbar - r.squeeze(-1), mbar - m.squeeze(-1)
    l = dr.abs() + dm.abs()
    loss = LS * (l / d["count"].to(dtype)).sum()          # sum over segments of the segment's mean
    loss.backward()
    return loss.detach(), r.grad.reshape(-1), m.grad.reshape(-1), dr.detach().abs(), dm.detach().abs(), ii.numel()


def part_restatement(d, dtype):
    seg = d["seg"]
    r, m = d["r"].to(dtype).clone().requires_grad_(True), d["m"].to(dtype).clone().requires_grad_(True)
    _, inv = seg.unique(return_inverse=True)
    n = int(inv.max()) + 1
    w = (1 - r).squeeze(-1).detach() + 1e-4
    S = torch.zeros(n, dtype=dtype).index_add(0, inv, w)
    M = (torch.zeros(n, dtype=dtype).index_add(0, inv, m.squeeze(-1) * w) / S).unsqueeze(-1)
    R = (torch.zeros(n, dtype=dtype).index_add(0, inv, r.squeeze(-1) * w) / S).unsqueeze(-1)
    loss = LP * ((m - M[inv]).abs().mean() + (r - R[inv]).abs().mean())
    loss.backward()
    return loss.detach(), r.grad.reshape(-1), m.grad.reshape(-1)


def bounds(ref64, ref32, floor_terms):
    """(relative loss bound, absolute gradient bounds for r and m) from the restatement's own float32 deviation and the floor_terms * 2^-24 floor"""
    floor = floor_terms * 2.0 ** -24
    d32 = abs(float(ref32[0]) - float(ref64[0])) / abs(float(ref64[0]))
    gb = [max(8 * float((ref32[i].double() - ref64[i]).abs().max()), floor * float(ref64[i].abs().max())) for i in (1, 2)]
    return max(8 * d32, floor), gb[0], gb[1]


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and the float64 / float32 restatements of a case, computed once and shared (never modified)"""
    if name == "small":
        d = make_inputs((1, 2, 39, 40, 41, 64, 146), 40, seed=1)
    else:
        d = make_inputs((1023, 1024, 53), 1024, seed=2)
    ref64, ref32 = semantic_restatement(d, torch.float64), semantic_restatement(d, torch.float32)
    return d, ref64, ref32


def run_semantic(d, dev, **kw):
    from iris_amd.utils.propagation import semantic_propagation_loss
    r, m = d["r"].to(dev).requires_grad_(True), d["m"].to(dev).requires_grad_(True)
    kw.setdefault("draws", d["draws"].to(dev))
    loss = semantic_propagation_loss(r, m, d["albedo"].to(dev), d["pos"].to(dev), d["seg"].to(dev), sigma_albedo=SIGMA_A, sigma_pos=SIGMA_P, ls=LS,
                                     n_samples=d["K"], **kw)
    return loss, r, m


def check_semantic(name, expect_pairs):
    d, ref64, ref32 = case(name)
    assert ref64[5] == expect_pairs
    assert float(ref64[3].min()) > 1e-5 and float(ref64[4].min()) > 1e-5, "precondition: a deviation within 1e-5 of zero could flip its sign in float32"
    loss_tol, gr_tol, gm_tol = bounds(ref64, ref32, d["K"])
    loss, r, m = run_semantic(d, "cuda")
    loss.backward()
    rel = abs(float(loss.detach()) - float(ref64[0])) / float(ref64[0])
    dgr = float((r.grad.reshape(-1).cpu().double() - ref64[1]).abs().max())
    dgm = float((m.grad.reshape(-1).cpu().double() - ref64[2]).abs().max())
    print(f"{name}: loss {float(loss.detach()):.9g} rel dev {rel:.3g} (bound {loss_tol:.3g}); grad dev r {dgr:.3g} (bound {gr_tol:.3g}) m {dgm:.3g} (bound {gm_tol:.3g}); "
          f"max|g64| {float(ref64[1].abs().max()):.3g}")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert rel <= loss_tol
    assert dgr <= gr_tol and dgm <= gm_tol


@pytest.mark.gpu
def test_recorded_draws_small_k():
    """N = 333, K = 40: segments below, at and above K and a singleton; 1 + 4 + 39^2 + 40 (40 + 41 + 64 + 146) pairs"""
    check_semantic("small", 1 + 4 + 39 * 39 + 40 * (40 + 41 + 64 + 146))


@pytest.mark.gpu
def test_recorded_draws_trainer_k():
    """K = 1024: a segment at the sampling threshold, one just below it (exhaustive, c^2 pairs) and a small one: the LDS path of the backward"""
    check_semantic("trainer", 1023 * 1023 + 1024 * 1024 + 53 * 53)


@pytest.mark.gpu
def test_singleton_closed_form():
    """One pixel, one segment: W = 1 + 1e-4, loss = ls (r + m) 1e-4 / (1 + 1e-4); d/dr = d/dm = +ls 1e-4 / (1 + 1e-4) (rbar - r = r (1 / W - 1) is negative,
    so its sign is -1: direct part -sign ls = +ls, propagated part sign ls / W = -ls / W; they nearly cancel).  float32 rounding: rbar = fl(r / fl(1 + 1e-4)) carries two roundings relative to r, the subtraction rbar - r is exact (Sterbenz), the sum and
    the product with ls add two more relative to the small result: bound 3 * 2^-24 * ls * (r + m) on the loss.  The gradient is fl(g - fl(g / W)) with g = fl(ls): bound
    3 * 2^-24 * ls."""
    from iris_amd.utils.propagation import semantic_propagation_loss
    r = torch.tensor([[0.37]], device="cuda", requires_grad=True)
    m = torch.tensor([[0.81]], device="cuda", requires_grad=True)
    loss = semantic_propagation_loss(r, m, torch.full((1, 3), 0.4, device="cuda"), torch.zeros(1, 3, device="cuda"), torch.tensor([12345], device="cuda"),
                                     sigma_albedo=SIGMA_A, sigma_pos=SIGMA_P, ls=LS)
    loss.backward()
    r64, m64 = float(r.detach().double()), float(m.detach().double())
    want = LS * (r64 + m64) * 1e-4 / (1 + 1e-4)
    g_want = LS * 1e-4 / (1 + 1e-4)
    print(f"singleton: loss {float(loss.detach()):.9g} want {want:.9g}; grads {float(r.grad):.9g} {float(m.grad):.9g} want {g_want:.9g}")
    assert abs(float(loss.detach()) - want) <= 3 * 2.0 ** -24 * LS * (r64 + m64)
    for g in (r.grad, m.grad):
        assert abs(float(g) - g_want) <= 3 * 2.0 ** -24 * LS


@pytest.mark.gpu
def test_philox_mode():
    from iris_amd.utils.propagation import propagation_draws
    d, _, _ = case("small")
    seg = d["seg"].cuda()
    K = d["K"]
    dr5, dr6 = propagation_draws(seg, K, 5), propagation_draws(seg, K, 6)
    assert dr5.shape == (seg.numel(), K) and dr5.dtype == torch.int64
    assert torch.equal(dr5, propagation_draws(seg, K, 5)) and not torch.equal(dr5, dr6)
    count = d["count"].cuda()
    assert bool((dr5 >= 0).all()) and bool((dr5 < count[:, None]).all())
    big = torch.where(d["seg"] == 7 * 6 + 3)[0]                     # the 146-member segment
    assert not torch.equal(dr5[big[0]], dr5[big[1]])
    a = run_semantic(d, "cuda", draws=None, seed=5)[0]
    b = run_semantic(d, "cuda", draws=None, seed=5)[0]
    c = run_semantic(d, "cuda", draws=dr5)[0]
    assert a.view(torch.int32).item() == b.view(torch.int32).item() == c.view(torch.int32).item()
    assert a.item() != run_semantic(d, "cuda", draws=None, seed=6)[0].item()
    t, _, _ = case("trainer")                                      # K = 1024: draws beyond the first Philox block of a lane
    a = run_semantic(t, "cuda", draws=None, seed=7)[0]
    c = run_semantic(t, "cuda", draws=propagation_draws(t["seg"].cuda(), 1024, 7))[0]
    assert a.view(torch.int32).item() == c.view(torch.int32).item()
    # uniformity: one 64-member segment, K = 1024: 65 536 draws, each rank's count within 6 sigma of 1024, sigma = sqrt(65536 / 64 * 63 / 64) = 31.7
    u = propagation_draws(torch.full((64,), 9, dtype=torch.int64, device="cuda"), 1024, 3)
    hist = torch.bincount(u.reshape(-1), minlength=64)
    assert hist.numel() == 64 and int((hist - 1024).abs().max()) <= 190, hist.tolist()


@pytest.mark.gpu
def test_gradient_repeatability():
    """the LDS and global float atomics sum in arrival order: two backward passes agree within test 1's tolerance, not necessarily bitwise"""
    d, ref64, ref32 = case("trainer")
    _, gr_tol, gm_tol = bounds(ref64, ref32, d["K"])
    loss, r, m = run_semantic(d, "cuda")
    saved = [t.clone() for t in loss.grad_fn.saved_tensors]
    g1 = torch.autograd.grad(loss, (r, m), retain_graph=True)
    assert all(torch.equal(s, t) for s, t in zip(saved, loss.grad_fn.saved_tensors)), "the backward changed what the forward saved"
    g2 = torch.autograd.grad(loss, (r, m))
    dev_r, dev_m = float((g1[0] - g2[0]).abs().max()), float((g1[1] - g2[1]).abs().max())
    print(f"repeat: max |g1 - g2| r {dev_r:.3g} m {dev_m:.3g} (bounds {gr_tol:.3g}, {gm_tol:.3g})")
    assert dev_r <= gr_tol and dev_m <= gm_tol


@pytest.mark.gpu
def test_part_branch():
    from iris_amd.utils.propagation import part_propagation_loss
    d, _, _ = case("small")
    ref64, ref32 = part_restatement(d, torch.float64), part_restatement(d, torch.float32)
    loss_tol, gr_tol, gm_tol = bounds(ref64, ref32, int(d["count"].max()))          # c_max terms in the longest sum
    out = []
    for _ in range(2):
        r, m = d["r"].cuda().requires_grad_(True), d["m"].cuda().requires_grad_(True)
        loss = part_propagation_loss(r, m, d["seg"].cuda(), lp=LP)
        loss.backward()
        out.append((loss.detach(), r.grad, m.grad))
    loss, gr, gm = out[0]
    rel = abs(float(loss.detach()) - float(ref64[0])) / float(ref64[0])
    dgr, dgm = float((gr.reshape(-1).cpu().double() - ref64[1]).abs().max()), float((gm.reshape(-1).cpu().double() - ref64[2]).abs().max())
    print(f"part: loss {float(loss.detach()):.9g} rel dev {rel:.3g} (bound {loss_tol:.3g}); grad dev r {dgr:.3g} (bound {gr_tol:.3g}) m {dgm:.3g} (bound {gm_tol:.3g})")
    assert rel <= loss_tol and dgr <= gr_tol and dgm <= gm_tol
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out[0], out[1])), "no atomics: two calls must agree bit for bit"


@pytest.mark.gpu
def test_end_to_end_autograd():
    """roughness and metallic as slices of one leaf (NGPBRDF's outputs are views of one network output): .grad is the sum of the two restatement gradients"""
    from iris_amd.utils.propagation import part_propagation_loss, semantic_propagation_loss
    d, s64, s32 = case("small")
    p64, p32 = part_restatement(d, torch.float64), part_restatement(d, torch.float32)
    _, sr_tol, sm_tol = bounds(s64, s32, d["K"])
    _, pr_tol, pm_tol = bounds(p64, p32, int(d["count"].max()))
    leaf = torch.cat([d["albedo"], d["r"], d["m"]], 1).cuda().requires_grad_(True)
    r, m, seg = leaf[:, 3:4], leaf[:, 4:5], d["seg"].cuda()
    total = semantic_propagation_loss(r, m, leaf[:, :3], d["pos"].cuda(), seg, sigma_albedo=SIGMA_A, sigma_pos=SIGMA_P, ls=LS, n_samples=d["K"],
                                      draws=d["draws"].cuda()) + part_propagation_loss(r, m, seg, lp=LP)
    total.backward()
    g = leaf.grad.cpu().double()
    assert float(g[:, :3].abs().max()) == 0.0                               # albedo is detached
    assert float((g[:, 3] - (s64[1] + p64[1])).abs().max()) <= sr_tol + pr_tol
    assert float((g[:, 4] - (s64[2] + p64[2])).abs().max()) <= sm_tol + pm_tol


@pytest.mark.gpu
def test_empty_batch_and_normalisation():
    """N = 0 gives a zero that is still differentiable; voxel_min / voxel_max normalise as train_brdf_crf.py:244 (same loss as pre-normalised positions,
    up to the rounding of the normalisation: positions here are chosen so that it is exact)"""
    from iris_amd.utils.propagation import part_propagation_loss, semantic_propagation_loss
    e = torch.zeros(0, 1, device="cuda", requires_grad=True)
    kw = dict(sigma_albedo=SIGMA_A, sigma_pos=SIGMA_P, ls=LS)
    z = semantic_propagation_loss(e, e, torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), **kw)
    z = z + part_propagation_loss(e, e, torch.zeros(0, dtype=torch.int64, device="cuda"), lp=LP)
    z.backward()
    assert float(z.detach()) == 0.0 and e.grad.shape == (0, 1)
    g = torch.Generator().manual_seed(3)
    world = torch.randint(-64, 64, (50, 3), generator=g).float() / 16.0        # multiples of 1/16 in [-4, 4): (x + 4) / 8 * 2 - 1 is exact
    seg = torch.randint(0, 3, (50,), generator=g).cuda()
    r, m, a = torch.rand(50, 1, generator=g).cuda(), torch.rand(50, 1, generator=g).cuda(), torch.rand(50, 3, generator=g).cuda() * 0.05
    l0 = semantic_propagation_loss(r, m, a, (world / 4.0).cuda(), seg, sigma_albedo=0.05, sigma_pos=0.5, ls=LS)
    l1 = semantic_propagation_loss(r, m, a, world.cuda(), seg, sigma_albedo=0.05, sigma_pos=0.5, ls=LS, voxel_min=-4.0, voxel_max=4.0)
    assert float(l0) > 0 and l0.view(torch.int32).item() == l1.view(torch.int32).item()
