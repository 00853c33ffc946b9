"""The trainers' albedo regulariser and step losses on the GPU (iris_amd/utils/losses.py, iris_amd/csrc/iris_loss.h) against the float64 restatement of the
reference's lines (tests/losses_ref64.py).

Tolerances follow the rule of tests/test_propagation.py::bounds, with the restatement's own float32 deviation (d32, g32 - g64: never the kernel's) and a
floor of n * 2^-24:
    loss, k:   |rel deviation| <= max(8 d32, n 2^-24)
    gradient:  |deviation|     <= max(8 max|g32 - g64|, n 2^-24 max|g64|)   elementwise
n is the longest chain of dependent float additions on the way from an input to the loss in the kernels' own reductions (`chain` below):
    ceil(c_max / 64)   a lane of the segment's wave adds every 64th member of the longest run            (loss_seg_means_kernel)
    + 6                the wave's xor butterfly
    + 2                the three channels of a position
    + P - 1            a thread's further positions, P = ceil(N / (256 B)): 1 up to N = 4096 x 256
    + 8                the tree over a workgroup's 256 positions                                          (loss_dots_kernel / loss_terms_kernel)
    + ceil(B / 256)    a thread of the last pass adds every 256th of the B = min(ceil(N / 256), 4096) partials (loss_terms_kernel's k / prop_sum_kernel)
    + 8                its tree
= 28 for `small` (c_max 146, N 333), 90 for `multi` (c_max 4097, N 8193) and 246 for `stride` (c_max 13107, N 1 048 876, which the issue's two cases do
not reach: the grid stops growing at 4096 workgroups): at most 256, asserted.  The older floor of 3N terms would be 1.5e-3 at
N = 8193: ten thousand times d32, enough to hide a dropped segment.  Nothing is near a cancellation: no pixel is left out.

Figures of the restatement (float64; d32 in brackets): small mse 0.06939 (3.6e-8), scale-invariant at la = 0.01 6.926e-4 (5.9e-8), k 0.97780 (4.5e-8),
gradient deviation 3.2e-10 at magnitude 1.5e-3; multi mse 0.06771 (7.5e-8), scale-invariant 6.771e-4 (1.6e-7), k 0.99964 (4.8e-7), gradient deviation
6.9e-11 at magnitude 4.5e-5.
Measured on an MI355X (relative deviation of the loss / largest gradient deviation / relative deviation of k): small mse 3.6e-8 / 2.3e-10, scale-invariant
2.5e-8 / 2.8e-12 / 1.6e-8; multi mse 3.5e-8 / 8.8e-12, scale-invariant 1.1e-8 / 6.6e-14 / 1.9e-9; stride (restatement: mse 0.06749, d32 2.8e-8, k 1.00052) mse 8.2e-8 / 8.0e-14 at magnitude 3.0e-7, scale-invariant
1.2e-8 / 8.6e-16 / 4.4e-8: all under 8 d32, the n 2^-24 floors (1.7e-6, 5.4e-6, 1.5e-5) are not what lets them pass.  Closed forms: N = 1 loss 0.0489726365 against 0.0489726389, k 0.710412383 against 0.710412373; equal priors c = 16 loss 0.134154245
against 0.134154235, c = 64 0.121938333 against 0.121938332.  Step losses: gradient against the sum of the pieces' 0 on the albedo, 4.7e-10 on roughness, 5.8e-11
on metallic; two passes of the response model's weight gradient 2.3e-10 apart.
"""
import pytest
import torch

from losses_ref64 import BIG_ID, LA, case

pytestmark = pytest.mark.gpu

MODES = {"mse": (False, 1.0), "scale_invariant": (True, LA)}
SAVED_K = 4          # _SegmentAlbedo.saved_tensors = (runs, order, albedo, seg_means, k)
SAVED_MEANS = 3


def chain(sizes):
    """n of the module docstring for segments of these sizes"""
    N = sum(sizes)
    B = min(-(-N // 256), 4096)
    n = -(-max(sizes) // 64) + 6 + 2 + (-(-N // (256 * B)) - 1) + 8 + -(-B // 256) + 8
    assert n <= 256
    return n


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def run_albedo(d, mode, seg=None, dev="cuda"):
    from iris_amd.utils.losses import segment_albedo_loss
    si, w = MODES[mode]
    a = d["albedo"].to(dev).requires_grad_(True)
    loss = segment_albedo_loss(a, d["prior"].to(dev), d["seg"].to(dev) if seg is None else seg, weight=w, scale_invariant=si)
    k = loss.grad_fn.saved_tensors[SAVED_K].clone()
    loss.backward()
    return loss.detach(), a.grad, k


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["small", "multi", "stride"])
def test_against_float64(name, mode):
    d, refs = case(name)
    assert int(d["seg"].max()) == BIG_ID
    ref64, ref32 = refs[mode]
    n = chain(d["sizes"])
    floor = n * 2.0 ** -24
    l64, g64, k64 = float(ref64[0]), ref64[1], ref64[2]
    loss_tol = max(8 * abs(float(ref32[0]) - l64) / l64, floor)
    grad_tol = max(8 * float((ref32[1].double() - g64).abs().max()), floor * float(g64.abs().max()))
    k_tol = max(8 * abs(ref32[2] - k64) / k64, floor)
    loss, grad, k = run_albedo(d, mode)
    rel = abs(float(loss) - l64) / l64
    dg = float((grad.cpu().double() - g64).abs().max())
    dk = abs(float(k) - k64) / k64
    print(f"{name} {mode}: n {n}; loss {float(loss):.9g} rel dev {rel:.3g} (bound {loss_tol:.3g}); grad dev {dg:.3g} (bound {grad_tol:.3g}, max|g64| "
          f"{float(g64.abs().max()):.3g}); k {float(k):.9g} rel dev {dk:.3g} (bound {k_tol:.3g})")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == d["albedo"].shape
    assert rel <= loss_tol
    assert dg <= grad_tol
    if mode == "scale_invariant":
        assert dk <= k_tol
    else:
        assert float(k) == 1.0
    again = run_albedo(d, mode)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((loss, grad, k), again)), "no atomics: two calls must agree bit for bit"


def test_single_pixel_closed_form():
    """N = 1: tbar = t exactly (one value divided by 1).  mse: every (1 t - a) carries one rounding and enters squared (2), the square one, the two channel
    additions two, the trees add zeros, the scale fl(1/3) and its product two: 7 roundings relative to a sum of non-negative terms, bound 8 * 2^-24 loss.
    Its gradient fl(fl(2/3) * fl(a - t)): 3 roundings, bound 4 * 2^-24 |g|.  scale_invariant: k = fl(fl(t.a) / fl(t.t)), each dot three roundings at the
    most on non-negative terms, the division one: bound 8 * 2^-24 k."""
    from iris_amd.utils.losses import segment_albedo_loss
    u = 2.0 ** -24
    a = torch.tensor([[0.31, 0.62, 0.17]], device="cuda", requires_grad=True)
    t = torch.tensor([[37.0, 200.0, 121.0]], device="cuda") / 255.0
    seg = torch.tensor([BIG_ID], device="cuda")
    a64, t64 = a.detach().cpu().double(), t.cpu().double()
    loss = segment_albedo_loss(a, t, seg)
    loss.backward()
    want, g_want = float(((a64 - t64) ** 2).mean()), 2.0 * (a64 - t64) / 3.0
    loss = loss.detach()
    print(f"N = 1 mse: loss {float(loss):.9g} want {want:.9g}; grad {a.grad.tolist()} want {g_want.tolist()}")
    assert abs(float(loss) - want) <= 8 * u * want
    assert bool(((a.grad.cpu().double() - g_want).abs() <= 4 * u * g_want.abs()).all())
    loss = segment_albedo_loss(a, t, seg, weight=LA, scale_invariant=True)
    k, k_want = float(loss.grad_fn.saved_tensors[SAVED_K]), float((t64 * a64).sum() / (t64 * t64).sum())
    print(f"N = 1 scale_invariant: k {k:.9g} want {k_want:.9g}")
    assert abs(k - k_want) <= 8 * u * k_want


@pytest.mark.parametrize("c", [16, 64])
def test_constant_prior_closed_form(c):
    """One segment of c = 2^j <= 64 members that all carry the prior t (multiples of 1/255): every lane holds one member or zero, the butterfly adds equal
    values or zeros, so every partial sum is t times a power of two and the division by c is exact: tbar = t bit for bit.  The loss is then
    mean((a - t)^2) over the 3c entries: per entry 3 roundings (the difference, twice, and the square), 2 for the channels, 6 for the tree levels that
    meet non-zero values (c <= 64 positions), 2 for the scale: 13 roundings on non-negative terms, bound 16 * 2^-24 loss."""
    from iris_amd.utils.losses import segment_albedo_loss
    g = torch.Generator().manual_seed(c)
    t_row = torch.tensor([37.0, 200.0, 121.0]) / 255.0
    a = (0.05 + 0.9 * torch.rand(c, 3, generator=g)).cuda().requires_grad_(True)
    loss = segment_albedo_loss(a, t_row.repeat(c, 1).cuda(), torch.full((c,), 7 * 3 + 3, dtype=torch.int64, device="cuda"))
    means = loss.grad_fn.saved_tensors[SAVED_MEANS]
    assert torch.equal(bits(means[0, :3].cpu()), bits(t_row)), "the segment mean of equal priors is that prior exactly"
    want = float(((a.detach().cpu().double() - t_row.double()) ** 2).mean())
    print(f"c = {c}: loss {float(loss.detach()):.9g} want {want:.9g}")
    assert abs(float(loss.detach()) - want) <= 16 * 2.0 ** -24 * want


def test_detachment_sharing_and_empty_batch():
    from iris_amd.utils.losses import segment_albedo_loss
    from iris_amd.utils.propagation import SegmentRuns
    d, _ = case("small")
    leaf = torch.cat([d["albedo"], d["prior"], d["r"], d["m"]], 1).cuda().requires_grad_(True)        # NGPBRDF's outputs are views of one network output
    seg = d["seg"].cuda()
    loss = segment_albedo_loss(leaf[:, :3], leaf[:, 3:6], seg, weight=LA, scale_invariant=True)
    loss.backward()
    assert float(leaf.grad[:, :3].abs().max()) > 0 and float(leaf.grad[:, 3:].abs().max()) == 0.0     # the prior is detached
    for mode in MODES:
        raw, shared = run_albedo(d, mode), run_albedo(d, mode, seg=SegmentRuns(seg))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(raw, shared))
    assert torch.equal(bits(loss), bits(run_albedo(d, "scale_invariant")[0]))
    e = torch.zeros(0, 3, device="cuda", requires_grad=True)
    for si in (False, True):
        z = segment_albedo_loss(e, torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), scale_invariant=si)
        e.grad = None
        z.backward()
        assert z.dim() == 0 and float(z.detach()) == 0.0 and e.grad.shape == (0, 3)


# ---- the step losses: the composition, not the kernels (those have their own tests)
def step_inputs():
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.shading_cache import ShadingCache
    d, _ = case("small")
    N = d["seg"].numel()
    g = torch.Generator().manual_seed(21)
    cache = ShadingCache(N)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=g))
    s = torch.linspace(0, 1, 64)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)]))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    return dict(d=d, N=N, cache=cache, crf=crf.cuda(), idx=torch.randperm(N, generator=g).cuda(), exposure=(0.5 + torch.rand(N, 1, generator=g)).cuda(),
                rgbs_gt=torch.rand(N, 3, generator=g).cuda(), L=(1.5 * torch.rand(N, 3, generator=g)).cuda())


def reassociation(pieces):
    """elementwise bound on the difference between two orders of adding these addends (autograd's accumulation order against the test's): at most
    len - 1 additions each, every one rounding a partial sum that is at most the sum of the magnitudes: 2 (len - 1) 2^-24 sum |g|"""
    return 2 * (len(pieces) - 1) * 2.0 ** -24 * sum(p.abs() for p in pieces)


def crf_spread(g_weight, N):
    """two backward passes of the response model: its table gradient adds in LDS in arrival order, a bin has at most N addends, so two passes differ by at
    most N 2^-24 max|g| (the rule of tests/test_crf.py::test_table_and_weight_gradients, there with the count K of the fullest bin)"""
    return N * 2.0 ** -24 * float(g_weight.abs().max())


@pytest.mark.parametrize("la", [LA, 0.0])
@pytest.mark.parametrize("has_part", [1, 0])
def test_brdf_crf_loss(has_part, la):
    """Every returned term is, bit for bit, the piece called on its own; loss is their sum in the reference's order; backward from loss gives the sum of
    the pieces' gradients: up to the order of that sum, and for roughness and metallic up to the propagation gradient's own bounds
    (tests/test_propagation.py::bounds: the semantic branch adds with float atomics)."""
    import test_propagation as tp
    from iris_amd.utils.losses import brdf_crf_loss, diffuse_regulariser, segment_albedo_loss
    from iris_amd.utils.propagation import part_propagation_loss, semantic_propagation_loss
    s = step_inputs()
    d, crf, cache, idx, seg = s["d"], s["crf"], s["cache"], s["idx"], s["d"]["seg"].cuda()
    leaf = torch.cat([d["albedo"], d["r"], d["m"]], 1).cuda().requires_grad_(True)
    albedo, r, m = leaf[:, :3], leaf[:, 3:4], leaf[:, 4:5]
    pos, prior = d["pos"].cuda(), d["prior"].cuda()
    hp = dict(ld=5e-4, lp=tp.LP, ls=tp.LS, sigma_albedo=tp.SIGMA_A, sigma_pos=tp.SIGMA_P, l_crf_increasing=0.1, l_crf_weight=0.001)
    out = brdf_crf_loss(dict(albedo=albedo, metallic=m, roughness=r), cache=cache, idx=idx, crf=crf, exposure=s["exposure"], rgbs_gt=s["rgbs_gt"],
                        segmentation=seg, positions=pos, albedo_prior=prior if la > 0 else None, has_part=has_part, la=la, seed=9, **hp)
    assert set(out) == {"loss", "loss_c", "loss_d", "loss_seg", "loss_a", "reg_crf", "psnr"}
    assert all(v.is_cuda and v.dim() == 0 for v in out.values())
    pieces = dict(loss_c=torch.nn.functional.mse_loss(crf(cache.shade(idx, albedo, m, r), s["exposure"]), s["rgbs_gt"]),
                  loss_d=diffuse_regulariser(r, m, ld=hp["ld"]),
                  loss_seg=part_propagation_loss(r, m, seg, lp=hp["lp"]) if has_part else
                  semantic_propagation_loss(r, m, albedo, pos, seg, sigma_albedo=hp["sigma_albedo"], sigma_pos=hp["sigma_pos"], ls=hp["ls"], seed=9),
                  reg_crf=0.1 * crf.reg_monotonically_increasing() + 0.001 * crf.reg_weight())
    if la > 0:
        pieces["loss_a"] = segment_albedo_loss(albedo, prior, seg, weight=la, scale_invariant=True)
    else:
        assert float(out["loss_a"]) == 0.0 and not out["loss_a"].requires_grad
    for name, p in pieces.items():
        assert torch.equal(bits(out[name]), bits(p)), name
    total = out["loss_c"] + out["loss_d"] + out["loss_seg"] + out["loss_a"] + out["reg_crf"]
    assert torch.equal(bits(out["loss"]), bits(total))
    assert torch.equal(bits(out["psnr"]), bits(-10.0 * torch.log10(pieces["loss_c"].detach().clamp_min(1e-5)))) and not out["psnr"].requires_grad
    assert all(float(out[name].detach()) > 0 for name in ("loss_c", "loss_d", "loss_seg", "reg_crf"))

    g_leaf, g_w = torch.autograd.grad(out["loss"], (leaf, crf.weight), retain_graph=True)
    per = [torch.autograd.grad(p, (leaf, crf.weight), allow_unused=True, retain_graph=True) for p in pieces.values()]
    leaf_parts = [g[0] for g in per if g[0] is not None]
    # the weight's addends: the lookup's table gradient and the two regularisers, each through its own get_crf()
    w_parts = [torch.autograd.grad(p, crf.weight, retain_graph=True)[0]
               for p in (pieces["loss_c"], 0.1 * crf.reg_monotonically_increasing(), 0.001 * crf.reg_weight())]
    tol = reassociation(leaf_parts)
    _, inv, counts = d["seg"].unique(return_inverse=True, return_counts=True)
    dd = dict(seg=d["seg"], K=1024, draws=None, albedo=d["albedo"], pos=d["pos"], r=d["r"], m=d["m"], count=counts[inv])
    restate = tp.part_restatement if has_part else tp.semantic_restatement
    _, r_tol, m_tol = tp.bounds(restate(dd, torch.float64), restate(dd, torch.float32), max(d["sizes"]))     # c_max terms in the longest sum (K > c_max: exhaustive)
    tol[:, 3] += r_tol
    tol[:, 4] += m_tol
    dev = (g_leaf - sum(leaf_parts)).abs()
    print(f"has_part {has_part} la {la}: loss {float(out['loss'].detach()):.9g}; max |g - sum of pieces| albedo {float(dev[:, :3].max()):.3g} r {float(dev[:, 3].max()):.3g} "
          f"m {float(dev[:, 4].max()):.3g} (propagation bounds {r_tol:.3g}, {m_tol:.3g})")
    assert bool((dev <= tol).all())
    assert float(g_leaf[:, :3].abs().max()) > 0
    assert bool(((g_w - sum(w_parts)).abs() <= reassociation(w_parts) + crf_spread(g_w, s["N"])).all()) and float(g_w.abs().max()) > 0


def test_initialize_loss():
    """loss = loss_a + loss_c (initialize.py:202), each the piece on its own bit for bit; every leaf gets its gradient from one piece only: albedo and L bit for bit,
    the response model's weight up to the arrival order of its LDS adds"""
    from iris_amd.utils.losses import initialize_loss, segment_albedo_loss
    s = step_inputs()
    d, crf, seg, prior = s["d"], s["crf"], s["d"]["seg"].cuda(), s["d"]["prior"].cuda()
    albedo, L = d["albedo"].cuda().requires_grad_(True), s["L"].requires_grad_(True)
    out = initialize_loss(albedo, L, crf=crf, exposure=s["exposure"], rgbs_gt=s["rgbs_gt"], albedo_prior=prior, segmentation=seg)
    assert set(out) == {"loss", "loss_c", "loss_a", "psnr"} and all(v.is_cuda and v.dim() == 0 for v in out.values())
    loss_c = torch.nn.functional.mse_loss(crf(L, s["exposure"]), s["rgbs_gt"])
    loss_a = segment_albedo_loss(albedo, prior, seg, weight=1.0, scale_invariant=False)
    assert torch.equal(bits(out["loss_c"]), bits(loss_c)) and torch.equal(bits(out["loss_a"]), bits(loss_a))
    assert torch.equal(bits(out["loss"]), bits(out["loss_a"] + out["loss_c"]))
    assert torch.equal(bits(out["psnr"]), bits(-10.0 * torch.log10(loss_c.detach().clamp_min(1e-5))))
    got = torch.autograd.grad(out["loss"], (albedo, L, crf.weight))
    want = torch.autograd.grad(loss_a, albedo) + torch.autograd.grad(loss_c, (L, crf.weight))
    dw = float((got[2] - want[2]).abs().max())
    print(f"initialize: loss {float(out['loss'].detach()):.9g}; weight.grad two passes {dw:.3g} (bound {crf_spread(got[2], s['N']):.3g})")
    assert all(float(x.abs().max()) > 0 for x in got)
    assert torch.equal(bits(got[0]), bits(want[0])), "albedo"
    assert torch.equal(bits(got[1]), bits(want[1])), "L"
    assert dw <= crf_spread(got[2], s["N"])
