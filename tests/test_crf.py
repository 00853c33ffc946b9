"""The camera response model on the GPU (iris_amd/model/crf.py, iris_amd/csrc/iris_crf.h) against tests/golden/crf_emor.npz -- the reference's EmorCRF
run in float32 on the CPU with the project's interpolator (tools/make_crf_golden.py) -- and against tools/crf_restatement.py, which
tests/test_crf_cpu.py ties to that golden bit for bit.

Lookups and g_hdr: every operation of the contract is one correctly rounded IEEE operation in a stated order, so the kernels must reproduce the golden
bit for bit (up to the sign of a zero: the kernel writes +0 where torch's clip gradient multiplies by a zero mask).  Sums (g_table, weight.grad, the
inverse table's normalisation and prefix sum) are taken in another order than torch's: they are compared with the float64 restatement under
    deviation <= max(8 d32, K 2^-24 max |g64|)      per channel, max norm
with d32 the float32 restatement's own deviation from float64 and K the number of addends of the fullest table bin (tests/test_propagation.py's rule).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from tools import crf_restatement as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fixture():
    g = golden("crf_emor.npz")
    return {k: (torch.from_numpy(g[k]) if g[k].dtype == np.float32 else g[k]) for k in g.files}


def same_bits(a, b):
    """bitwise equality up to the sign of a zero (x + 0 turns -0 into +0)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal((a + 0.0).view(torch.int32), (b + 0.0).view(torch.int32))


def grid_of(n, dev="cuda"):
    return torch.linspace(0, 1, n).to(dev)


def model_of(f, k, dev="cuda"):
    from iris_amd.model.crf import EmorCRF
    m = EmorCRF.from_arrays(f["f0"][0], f["basis"])
    m.load_state_dict({"f0": f["f0"], "basis": f["basis"], "weight": f[f"weight_{k}"]})
    return m.to(dev)


def exposure_forms(e, B, dev="cuda"):
    """the forms forward and inverse accept for the exposure `e` (a python float, or (B, 1) values per pixel)"""
    if isinstance(e, float):
        return [e, torch.tensor(e, device=dev), torch.tensor([e], device=dev), torch.full((B,), e, device=dev), torch.full((B, 1), e, device=dev)]
    return [e.to(dev), e.to(dev).reshape(-1)]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_lookups_reproduce_the_golden_bit_for_bit(k):
    """forward, its gradient to hdr and the inverse lookup with the golden's tables handed in: all rows (every knot of the grid and its two float
    neighbours, 0, 1, values outside [0, 1], a subnormal, uniform draws), the five forms of the exposure"""
    from iris_amd.model.crf import crf_lookup, crf_lookup_inverse
    f = fixture()
    x, block = f["x"], f["block"]
    table, inv, grid = f[f"table_{k}"].cuda(), f[f"inv_{k}"].cuda(), grid_of(1024)
    cot = R.cotangent(len(x))
    forms = 0
    for b, e in enumerate((1.0, 1.7, f["e_pixel"])):
        lo, hi = int(block[b]), int(block[b + 1])
        for ef in exposure_forms(e, hi - lo):
            h = x[lo:hi].cuda().requires_grad_(True)
            ldr = crf_lookup(h, table, grid, ef)
            (g_hdr,) = torch.autograd.grad(ldr, h, cot[lo:hi].cuda())
            bad = ((ldr.detach().cpu() + 0.0).view(torch.int32) != (f[f"ldr_{k}"][lo:hi] + 0.0).view(torch.int32)).nonzero()
            assert same_bits(ldr, f[f"ldr_{k}"][lo:hi]), (b, type(ef), bad[:4].tolist(), x[lo:hi][bad[:4, 0], bad[:4, 1]].tolist())
            assert same_bits(g_hdr, f[f"ghdr_{k}"][lo:hi]), (b, type(ef))
            assert same_bits(crf_lookup_inverse(x[lo:hi].cuda(), inv, grid, ef), f[f"hdr_{k}"][lo:hi]), (b, type(ef))
            forms += 1
    assert forms == 12


def table_gradient_case(table, x, e_pixel, block, dtype):
    """(g_table (3, n), addends of the fullest bin per channel) of the restatement in `dtype` over the fixture's blocks"""
    t = table.to(dtype).clone().requires_grad_(True)
    ldr = R.by_block(lambda rows, e: R.forward(t, rows.to(dtype), e.to(dtype) if torch.is_tensor(e) else e), x, e_pixel, block)
    (g,) = torch.autograd.grad((ldr * R.cotangent(len(x)).to(dtype)).sum(), t)
    n = table.shape[1]
    q = R.by_block(lambda rows, e: torch.clip(rows * e, 0, 1), x, e_pixel, block)          # float32, as the kernel forms it
    K = []
    for c in range(3):
        l, r, _, _, _ = R.segment(torch.linspace(0, 1, n), q[:, c])
        K.append(int(torch.bincount(torch.cat([l, r]), minlength=n).max()))
    return g, K


def addends_per_bin(x, e_pixel, block, n):
    """(3, n) number of addends each table bin receives from the fixture's rows"""
    q = R.by_block(lambda rows, e: torch.clip(rows * e, 0, 1), x, e_pixel, block)
    return [torch.bincount(torch.cat(R.segment(torch.linspace(0, 1, n), q[:, c])[:2]), minlength=n) for c in range(3)]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_table_and_weight_gradients(k):
    """g_table (LDS sums per workgroup, slabs added in slab order) and weight.grad through the module against the float64 restatement.
    Prints every deviation, its bound, d32, K and the spread of two backward passes of the same input (the LDS adds inside a workgroup arrive in
    any order).  No figures from an MI355X are recorded yet.  On the host, the kernel's source with one thread per workgroup gives a
    weight.grad within 6.0e-7 of the golden's at magnitude 2.5."""
    from iris_amd.model.crf import crf_lookup
    f = fixture()
    x, e_pixel, block = f["x"], f["e_pixel"], f["block"]
    table = f[f"table_{k}"]
    g64, K = table_gradient_case(table, x, e_pixel, block, torch.float64)
    g32, _ = table_gradient_case(table, x, e_pixel, block, torch.float32)
    grid, cot = grid_of(1024), R.cotangent(len(x)).cuda()

    def device_gradient():
        t = table.cuda().requires_grad_(True)
        ldr = R.by_block(lambda rows, e: crf_lookup(rows, t, grid, e), x.cuda(), e_pixel.cuda(), block)
        return torch.autograd.grad((ldr * cot).sum(), t)[0].cpu()

    g1, g2 = device_gradient(), device_gradient()
    counts = addends_per_bin(x, e_pixel, block, 1024)
    for c in range(3):
        # all bins (the fullest are the two end bins, which take every clipped pixel), then bins 1 .. n-2 alone under the same rule with their own K,
        # d32 and max |g64|: the end bins' bound is a thousand times an interior bin's value and would hide an interior bin that is wrong
        for name, sl in (("all bins", slice(None)), ("interior", slice(1, -1))):
            Kc, gmax = int(counts[c][sl].max()), float(g64[c][sl].abs().max())
            d32 = float((g32[c][sl].double() - g64[c][sl]).abs().max())
            bound = max(8 * d32, Kc * U * gmax)
            dev, spread = float((g1[c][sl].double() - g64[c][sl]).abs().max()), float((g1[c][sl] - g2[c][sl]).abs().max())
            print(f"case {k} channel {c} {name}: g_table dev {dev:.3g} (bound {bound:.3g}, d32 {d32:.3g}, K {Kc}, max|g64| {gmax:.3g}); two passes {spread:.3g}")
            assert dev <= bound and spread <= bound, (name, c)
        assert K[c] == int(counts[c].max())
    # weight.grad = g_table @ basis^T through the module (torch's matmul): the same rule applied to it directly, with the table's K
    basis64 = f["basis"].double()
    w64 = g64 @ basis64.T
    w32 = (g32 @ f["basis"].T).double()
    m = model_of(f, k)
    ldr = R.by_block(m, x.cuda(), e_pixel.cuda(), block)
    (ldr * cot).sum().backward()
    got = m.weight.grad.cpu().double()
    assert got.shape == (3, 11)
    for c in range(3):
        d32, wmax = float((w32[c] - w64[c]).abs().max()), float(w64[c].abs().max())
        bound = max(8 * d32, K[c] * U * wmax)
        dev = float((got[c] - w64[c]).abs().max())
        print(f"case {k} channel {c}: weight.grad dev {dev:.3g} (bound {bound:.3g}, d32 {d32:.3g}, K {K[c]}, max|g64| {wmax:.3g})")
        assert dev <= bound, c


@pytest.mark.parametrize("k", [0, 1, 2])
def test_inverse_table(k):
    """get_inv_crf: a tree sum and a parallel prefix sum where torch's cumsum is sequential -- per channel within max(8 d32, 4 * 2^-24) of the float64
    restatement; non-decreasing; starts at 0.  Cases 1 and 2 add a gap (their tables are not monotone), so their knots repeat.  The kernel's source run
    on the host with 1024 threads deviates by 1.3e-7 .. 4.4e-7 under bounds of 8.7e-7 .. 2.9e-6; device figures are not recorded yet."""
    from iris_amd.model.crf import crf_inverse_table
    f = fixture()
    m = model_of(f, k)
    inv = m.get_inv_crf()
    assert inv.shape == (3, 1024) and not inv.requires_grad and inv.is_cuda
    own = m.get_crf().detach().cpu()                       # the table the module inverted: get_crf's matmul ran on the device
    for name, table, got in (("get_inv_crf", own, inv.cpu()), ("golden's table", f[f"table_{k}"], crf_inverse_table(f[f"table_{k}"].cuda(), grid_of(1024)).cpu())):
        i64, i32 = R.inv_table(table.double()), R.inv_table(table)
        for c in range(3):
            d32 = float((i32[c].double() - i64[c]).abs().max())
            bound = max(8 * d32, 4 * U)
            dev = float((got[c].double() - i64[c]).abs().max())
            print(f"case {k} channel {c} {name}: inverse table dev {dev:.3g} (bound {bound:.3g}, d32 {d32:.3g})")
            assert dev <= bound, (name, c)
        assert bool((got[:, 1:] >= got[:, :-1]).all()) and bool((got[:, 0] == 0).all()), name
    print(f"case {k}: device get_crf against the golden's table {float((own - f[f'table_{k}']).abs().max()):.3g}")


def test_round_trip():
    """inverse(forward(x)) on x in [0.05, 0.95] with zero weights, exposure 1.05 (x * 1.05 stays below 1: nothing is clipped).  Both lookups are piecewise linear over different knots, so the round trip is not the
    identity: the float32 restatement's own round trip deviates by rt32 (printed; it is resampling error, not rounding), and the device may deviate by
    twice that.  rt32 = 7.0e-6 on the CPU; the device figure is not recorded yet."""
    f = fixture()
    m = model_of(f, 0)
    x = torch.linspace(0.05, 0.95, 3000).reshape(-1, 3).contiguous()
    table = f["table_0"]
    rt32 = float((R.inverse(R.inv_table(table), R.forward(table, x, 1.05), 1.05) - x).abs().max())
    with torch.no_grad():
        back = m.inverse(m(x.cuda(), 1.05), 1.05).cpu()
    dev = float((back - x).abs().max())
    print(f"round trip: device {dev:.3g}, float32 restatement {rt32:.3g}")
    assert dev <= 2 * rt32


def restated(table, x, e, cot):
    """(ldr, g_hdr, g_table float32, g_table float64, K per channel) of the restatement on the CPU for one block of rows"""
    out = []
    for dtype in (torch.float32, torch.float64):
        t, h = table.to(dtype).clone().requires_grad_(True), x.to(dtype).clone().requires_grad_(True)
        ldr = R.forward(t, h, e.to(dtype) if torch.is_tensor(e) else e)
        out.append((ldr.detach(),) + torch.autograd.grad((ldr * cot.to(dtype)).sum(), (h, t)))
    n = table.shape[1]
    q = torch.clip(x * e, 0, 1)
    K = [int(torch.bincount(torch.cat(R.segment(torch.linspace(0, 1, n), q[:, c])[:2]), minlength=n).max()) for c in range(3)]
    return out[0][0], out[0][1], out[0][2], out[1][2], K


@pytest.mark.parametrize("B,n", [(1, 1024), (63, 1024), (64, 1024), (65, 1024), (200003, 1024), (777, 256)])
def test_shapes(B, n):
    """one pixel; around a wave; more than one grid-stride pass of both kernels and every slab (200 003); a table of 256 knots"""
    from iris_amd.model.crf import crf_inverse_table, crf_lookup, crf_lookup_inverse
    f = fixture()
    g = torch.Generator().manual_seed(B)
    if n == 1024:
        table = f["table_2"]
    else:
        s = torch.linspace(0, 1, n)
        table = torch.stack([s ** 0.45, s ** 0.5 + 0.02 * torch.sin(40 * s), 1 - (1 - s) ** 2])       # the middle one is not monotone
    x = torch.rand(B, 3, generator=g) * 1.4 - 0.1
    e = torch.rand(B, 1, generator=g) * 1.5 + 0.5
    cot = torch.rand(B, 3, generator=g) - 0.5
    ldr, g_hdr, gt32, gt64, K = restated(table, x, e, cot)
    grid = grid_of(n)
    t, h = table.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    out = crf_lookup(h, t, grid, e.cuda())
    gh, gt = torch.autograd.grad(out, (h, t), cot.cuda())
    assert same_bits(out, ldr) and same_bits(gh, g_hdr)
    for c in range(3):
        bound = max(8 * float((gt32[c].double() - gt64[c]).abs().max()), K[c] * U * float(gt64[c].abs().max()))
        dev = float((gt[c].cpu().double() - gt64[c]).abs().max())
        print(f"B {B} n {n} channel {c}: g_table dev {dev:.3g} (bound {bound:.3g}, K {K[c]})")
        assert dev <= bound
    inv = crf_inverse_table(table.cuda(), grid)
    i64, i32 = R.inv_table(table.double()), R.inv_table(table)
    for c in range(3):
        assert float((inv[c].cpu().double() - i64[c]).abs().max()) <= max(8 * float((i32[c].double() - i64[c]).abs().max()), 4 * U)
    assert same_bits(crf_lookup_inverse(x.cuda(), inv, grid, e.cuda()), R.inverse(inv.cpu(), x, e))


def test_non_contiguous_input_and_argument_errors():
    from iris_amd import _lib as L
    from iris_amd.model.crf import crf_lookup
    f = fixture()
    table, grid = f["table_1"].cuda(), grid_of(1024)
    base = (torch.rand(500, 6, generator=torch.Generator().manual_seed(3)) * 1.2).cuda().requires_grad_(True)
    view = base[:, ::2]
    assert not view.is_contiguous()
    out = crf_lookup(view, table, grid, 1.1)
    ref = crf_lookup(view.detach().contiguous().requires_grad_(True), table, grid, 1.1)
    assert same_bits(out, ref)
    out.sum().backward()
    assert base.grad.shape == base.shape and float(base.grad[:, 1::2].abs().max()) == 0.0 and float(base.grad[:, ::2].abs().max()) > 0.0
    with pytest.raises(ValueError):
        crf_lookup(view, table, grid, torch.ones(7, device="cuda"))           # neither one value nor one per pixel
    with pytest.raises(ValueError):
        crf_lookup(torch.rand(5, 4, device="cuda"), table, grid, 1.0)
    with pytest.raises(ValueError):
        crf_lookup(view, torch.rand(3, 2048, device="cuda"), grid_of(2048), 1.0)
    with pytest.raises(L.IrisError):
        crf_lookup(view, table.cpu(), grid, 1.0)
    e = torch.tensor(1.1, device="cuda", requires_grad=True)                   # the exposure never gets a gradient
    out = crf_lookup(base[:, :3], table, grid, e)
    assert torch.autograd.grad(out.sum(), e, allow_unused=True)[0] is None


def test_gradient_against_finite_differences():
    """64 interior points in the middle of their segments: the lookup is linear there, so a central difference of the float64 restatement is its exact
    slope; the kernel's float32 g_hdr = g * slope * e carries seven roundings (three differences, a sum, a quotient, two products): 8 * 2^-24 relative"""
    from iris_amd.model.crf import crf_lookup
    f = fixture()
    table = f["table_1"]
    g = torch.Generator().manual_seed(5)
    seg = torch.randperm(1000, generator=g)[:192].reshape(64, 3) + 10
    e = 1.25
    hdr = ((seg.double() + 0.5) / 1023 / e).float()
    h = hdr.cuda().requires_grad_(True)
    (gh,) = torch.autograd.grad(crf_lookup(h, table.cuda(), grid_of(1024), e).sum(), h)
    step = 0.2 / 1023 / e
    fd = (R.forward(table.double(), hdr.double() + step, e) - R.forward(table.double(), hdr.double() - step, e)) / (2 * step)
    rel = ((gh.cpu().double() - fd).abs() / fd.abs().clamp_min(1e-12)).max()
    print(f"finite differences: max relative deviation {float(rel):.3g}")
    assert float(fd.abs().min()) > 1e-3 and float(rel) <= 8 * U + 1e-9          # (1e-9: the difference quotient's own rounding in float64)


def test_prebake_stages_take_the_model():
    """bake_slf with LDR photographs, exposure 1.3 and crf=model pools what the same call pools from model.inverse(rgbs, 1.3) given as linear radiance:
    integer tables identical, radiance equal up to the order of the atomics' float sums (the bound tests/test_prebake.py uses)"""
    from iris_amd import slf_bake as sb
    from iris_amd.utils.path_tracing import Scene
    dev = torch.device("cuda:0")
    f = fixture()
    g, p = golden("bake_box.npz"), golden("prebake_box.npz")
    scene = Scene(g["verts"], g["faces"], device=dev)
    m = model_of(f, 1, dev)
    res = int(p["res_spatial"])
    ldr_views, lin_views = [], []
    for k in range(int(p["n_views"])):
        rays = torch.from_numpy(p[f"rays_{k}"]).to(dev)
        with torch.no_grad():
            ldr = m(torch.from_numpy(p[f"rgbs_{k}"]).to(dev), 1.3)
        ldr_views.append({"rays": rays, "rgbs": ldr, "exposure": 1.3})
        lin_views.append({"rays": rays, "rgbs": m.inverse(ldr, 1.3)})
    a = sb.bake_slf(scene, ldr_views, res_spatial=res, dataset="scannetpp", device=dev, crf=m)
    b = sb.bake_slf(scene, lin_views, res_spatial=res, dataset="scannetpp", device=dev)
    assert a["voxel_min"] == b["voxel_min"] and a["voxel_max"] == b["voxel_max"]
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["weight"]["inds"], b["weight"]["inds"]) and torch.equal(a["weight"]["count"], b["weight"]["count"])
    assert float(b["weight"]["radiance"].abs().max()) > 0.1
    np.testing.assert_allclose(a["weight"]["radiance"].numpy(), b["weight"]["radiance"].numpy(), rtol=2e-5, atol=1e-6)
    a2, b2 = sb.refine_slf(a, scene, ldr_views, dev, crf=m), sb.refine_slf(b, scene, lin_views, dev)
    assert torch.equal(a2["weight"]["count"], b2["weight"]["count"])
    np.testing.assert_allclose(a2["weight"]["radiance"].numpy(), b2["weight"]["radiance"].numpy(), rtol=2e-5, atol=1e-6)
    ea = sb.extract_emitters(scene, g["verts"], g["faces"], ldr_views, threshold=float(p["threshold"]), device=dev, crf=m)
    eb = sb.extract_emitters(scene, g["verts"], g["faces"], lin_views, threshold=float(p["threshold"]), device=dev)
    assert torch.equal(ea["is_emitter"], eb["is_emitter"])
