"""The backward pass of the hash-grid material network (iris_ngp_backward, NGPBRDF under autograd; iris_amd/csrc/iris_ngp.h).

Gradient definition (straight-through): every rounding to half of the forward has derivative 1; d/dz of the output stage is g * s (1 - s), s the
forward's half-grid sigmoid (* 0.98 for roughness); ReLU masks from the pre-activations (> 0); padded outputs 5..15 have dz = 0.

Two references, both on the CPU:
  * torch autograd through oracle/ngp_torch.forward as it stands: it rounds GRADIENTS to half at every cast of the forward;
  * `f64_gradient` below: the oracle's own forward values (features, activations, masks, sigmoid) with the backward of the definition in float64.
For each block k (dW1, dW2, rows 0-4 of dW3, each of the 32 levels' tables) floor_k = the relative L2 distance between the two.  The HIP gradient
must lie within 2 * floor_k + 2^-9 of the float64 reference: the factor 2 for atomic ordering and f32 summation order, 2^-9 = four half roundings of
an operand (2^-11 each: dz and the activation of a weight-gradient product, dz and the weight of a data-gradient product), which the oracle's f32
dW3 path does not have.

Measured on an MI355X (worst block: distance to the float64 reference, share of its bar): n = 1: 1.22e-3, 0.35; n = 33: 4.5e-4, 0.16; n = 2500: 3.9e-4, 0.13;
chunk boundary: 4.2e-4, 0.13 (floors 3e-4 .. 7e-4; 2.2e-3 at n = 1).  Also in DESIGN.md section 5f."""
import functools
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, REPO)
from oracle import ngp_torch as ng     # noqa: E402

VMIN, VMAX = -2.0, 2.5
N_MLP = ng.N_MLP_PARAMS


def _params(seed, scale=0.5):
    """tests/test_ngp.py::_params, restated"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(ng.n_params(), generator=g) * 2 - 1) * scale


def _positions(n, seed):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * (VMAX - VMIN) + VMIN


def _cotangents(n, seed):
    """randn of order 1: (albedo (n,3), roughness (n,1), metallic (n,1))"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), torch.randn(n, 1, generator=g), torch.randn(n, 1, generator=g)


def _encoder_input(pos):
    p = (pos.to(torch.float32) - np.float32(VMIN)) / np.float32(float(VMAX) - float(VMIN))
    return p * np.float32(2.0) - np.float32(1.0)


def _corners(x):
    """the test's own restatement of the encoding's geometry: per level, the 8 table entries (global entry index, (B, 8) int64) a point reads and their
    trilinear weights ((B, 8) float32) -- the published algorithm as oracle/ngp_torch.encode states it, with the index kept instead of the value"""
    rows, _ = ng.level_tables()
    M = 0xFFFFFFFF
    out = []
    for scale, res, n, off in rows:
        p = (x.numpy().astype(np.float64) * np.float64(np.float32(scale)) + 0.5).astype(np.float32)          # fmaf(scale, x, 0.5)
        fl = np.floor(p)
        w = (p - fl).astype(np.float32)
        cell = fl.astype(np.int64) & M
        dense = res ** 3 <= n
        idx = np.empty((x.shape[0], 8), np.int64); wgt = np.empty((x.shape[0], 8), np.float32)
        for c in range(8):
            t = np.ones(x.shape[0], np.float32); g = []
            for d in range(3):
                if c >> d & 1:
                    t = t * w[:, d]; g.append((cell[:, d] + 1) & M)
                else:
                    t = t * (np.float32(1.0) - w[:, d]); g.append(cell[:, d])
            if dense:
                i = (g[0] + g[1] * res + g[2] * res * res) & M
            else:
                i = g[0] ^ ((g[1] * 2654435761) & M) ^ ((g[2] * 805459861) & M)
            idx[:, c] = off + i % n; wgt[:, c] = t
        out.append((torch.from_numpy(idx), torch.from_numpy(wgt)))
    return out


def _forward_values(params, pos):
    """the oracle's forward with its intermediates kept: features X (half), hidden pre-activations, hidden activations (half), the half-grid sigmoid s"""
    x = _encoder_input(pos)
    w = params[:N_MLP].to(torch.float16)
    W1, W2, W3 = w[:4096].reshape(64, 64), w[4096:8192].reshape(64, 64), w[8192:].reshape(16, 64)
    X = ng.encode(params, x)
    pre1 = X.float() @ W1.float().T
    H1 = torch.relu(pre1).to(torch.float16)
    pre2 = H1.float() @ W2.float().T
    H2 = torch.relu(pre2).to(torch.float16)
    out_half = (H2.float() @ W3.float().T)[:, :5].to(torch.float16)
    s = torch.sigmoid(out_half.float()).to(torch.float16).float()
    return dict(x=x, X=X, pre1=pre1, H1=H1, pre2=pre2, H2=H2, s=s, W1=W1, W2=W2, W3=W3)


def f64_gradient(params, pos, cot):
    """d sum(outputs * cot) / d params by the straight-through definition, float64 arithmetic on the oracle's forward values"""
    v = _forward_values(params, pos)
    d = lambda t: t.to(torch.float64)
    s = d(v["s"])
    g = torch.cat([d(cot[0]), d(cot[1]) * 0.98, d(cot[2])], dim=1)
    dz3 = torch.zeros(pos.shape[0], 16, dtype=torch.float64)
    dz3[:, :5] = g * s * (1 - s)
    dW3 = dz3.T @ d(v["H2"])
    dz2 = (dz3 @ d(v["W3"])) * d(v["pre2"] > 0)
    dW2 = dz2.T @ d(v["H1"])
    dz1 = (dz2 @ d(v["W2"])) * d(v["pre1"] > 0)
    dW1 = dz1.T @ d(v["X"])
    dX = dz1 @ d(v["W1"])
    _, total = ng.level_tables()
    tab = torch.zeros(total, 2, dtype=torch.float64)
    for l, (idx, wgt) in enumerate(_corners(v["x"])):
        for c in range(8):
            tab.index_add_(0, idx[:, c], d(wgt[:, c])[:, None] * dX[:, 2 * l:2 * l + 2])
    return torch.cat([dW1.reshape(-1), dW2.reshape(-1), dW3.reshape(-1), tab.reshape(-1)])


def oracle_gradient(params, pos, cot):
    p = params.clone().requires_grad_(True)
    out = ng.forward(p, pos, VMIN, VMAX)
    ((out["albedo"] * cot[0]).sum() + (out["roughness"] * cot[1]).sum() + (out["metallic"] * cot[2]).sum()).backward()
    return p.grad.detach()


def _blocks():
    rows, _ = ng.level_tables()
    b = [("dW1", slice(0, 4096)), ("dW2", slice(4096, 8192)), ("dW3[0:5]", slice(8192, 8192 + 5 * 64))]
    return b + [("level%02d" % l, slice(N_MLP + 2 * off, N_MLP + 2 * (off + n))) for l, (_, _, n, off) in enumerate(rows)]


def _dist(a, ref):
    a, ref = a.to(torch.float64), ref.to(torch.float64)
    den = float(ref.norm())
    num = float((a - ref).norm())
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """(params, positions, cotangents, float64 reference, {block: floor}); computed once per case and shared, never modified"""
    if kind == "chunk":
        n = (1 << 20) + 77
        pos = _positions(n, 77)
        sel = torch.cat([torch.arange(100), torch.arange((1 << 20) - 60, (1 << 20) + 63), torch.arange(n - 77, n)])
        assert sel.numel() == 300
        c = _cotangents(300, 78)
        # (the last 77 points ARE the second chunk, so 63 of them are chosen twice: such a point carries the sum of its two cotangents, which by linearity
        #  is what the reference evaluated on the 300 chosen points, repeats included, differentiates)
        cot = tuple(torch.zeros(n, t.shape[1]).index_add_(0, sel, t) for t in c)
        sub_pos, sub_cot = pos[sel], c
    else:
        n = int(kind)
        pos, cot = _positions(n, 100 + n), _cotangents(n, 200 + n)
        sub_pos, sub_cot = pos, cot
    params = _params(4, 0.3)
    ref = f64_gradient(params, sub_pos, sub_cot)
    orc = oracle_gradient(params, sub_pos, sub_cot)
    floors = {name: _dist(orc[sl], ref[sl]) for name, sl in _blocks()}
    return params, pos, cot, ref, floors


def _check_bars(grad, ref, floors, what):
    worst = (0.0, None)
    bad = []
    for name, sl in _blocks():
        dist, bar = _dist(grad[sl], ref[sl]), 2 * floors[name] + 2.0 ** -9
        if dist / bar > worst[0]:
            worst = (dist / bar, (name, dist, floors[name]))
        if not dist <= bar:
            bad.append((name, dist, bar))
    print("%s: worst block %s: distance %.3e (floor %.3e), %.2f of its bar; max floor %.3e" % (what, worst[1][0], worst[1][1], worst[1][2], worst[0], max(floors.values())))
    assert not bad, (what, bad)


# ----------------------------------------------------------------------------------------------------------------------------------------------
# not gpu
# ----------------------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("iris_ngp_set_params_dev", "iris_ngp_backward_workspace_bytes", "iris_ngp_backward")


def test_header_and_prototypes_declare_the_training_entry_points():
    src = open(os.path.join(REPO, "include", "iris_hip.h")).read()
    declared = set(re.findall(r"IRIS_API[^;(]*?\b(iris_\w+)\s*\(", src))
    from iris_amd import _lib as L
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in L.PROTOTYPES, name
    assert "inference only" not in src and "inference only" not in open(os.path.join(REPO, "iris_amd", "csrc", "iris_ngp.h")).read()


def test_the_two_references_agree_to_their_floor():
    """33 points: pins the test's own restatement (corner indices and weights, the forward's intermediates) against the oracle.  The oracle's gradients pass
    through at most six successive roundings to half (2^-11 each) on their way from the outputs to a parameter: every block's floor must be below 2^-8."""
    params, pos, cot, ref, floors = _reference("33")
    v = _forward_values(params, pos)
    out = ng.forward(params, pos, VMIN, VMAX)
    assert torch.equal(out["albedo"], v["s"][:, :3]) and torch.equal(out["metallic"], v["s"][:, 4:5])
    assert torch.equal(out["roughness"], v["s"][:, 3:4] * np.float32(0.98) + np.float32(0.02))
    # the restated corners reproduce the oracle's features up to its 8 half roundings per feature
    grid = params[N_MLP:].to(torch.float16).to(torch.float64).reshape(-1, 2)
    for l, (idx, wgt) in enumerate(_corners(v["x"])):
        f = (wgt.to(torch.float64)[:, :, None] * grid[idx]).sum(1)
        assert float((f - v["X"][:, 2 * l:2 * l + 2].to(torch.float64)).abs().max()) <= 16 * 2.0 ** -11 * 0.3, l
    print("floors at 33 points:", {k: "%.2e" % f for k, f in floors.items()})
    assert all(f < 2.0 ** -8 for f in floors.values()), floors
    assert all(float(ref[sl].norm()) > 0 for _, sl in _blocks())
    assert float(ref[8192 + 5 * 64:N_MLP].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------------------------
# gpu
# ----------------------------------------------------------------------------------------------------------------------------------------------
def _net(params, dev, trainable=True):
    from iris_amd.model.brdf import NGPBRDF
    net = NGPBRDF(VMIN, VMAX)
    net.load_state_dict({"mlp.params": params})
    if trainable:
        net.to(dev)
        net.mlp.params.requires_grad_(True)
    return net


def _hip_gradient(net, pos, cot):
    net.mlp.params.grad = None
    out = net(pos)
    ((out["albedo"] * cot[0]).sum() + (out["roughness"] * cot[1]).sum() + (out["metallic"] * cot[2]).sum()).backward()
    return net.mlp.params.grad


def _raw_backward(net, pos, cot, grad, workspace_bytes=None):
    from iris_amd import _lib as L
    n = pos.shape[0]
    nbytes = int(L.lib().iris_ngp_backward_workspace_bytes(n)) if workspace_bytes is None else workspace_bytes
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=pos.device)
    ga, gr, gm = cot[0].contiguous(), cot[1].reshape(-1).contiguous(), cot[2].reshape(-1).contiguous()
    rc = L.lib().iris_ngp_backward(net._handle(pos.device), L.ptr(pos), n, L.ptr(ga), L.ptr(gr), L.ptr(gm), float(net.loss_scale), L.ptr(grad), L.ptr(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 5000])
def test_forward_under_autograd_equals_the_frozen_path(n):
    dev = torch.device("cuda:0")
    params = _params(4, 0.3)
    pos = _positions(n, n).to(dev)
    frozen = _net(params, dev, trainable=False)(pos)
    out = _net(params, dev)(pos)
    for k in frozen:
        assert out[k].requires_grad and not frozen[k].requires_grad
        assert torch.equal(out[k].detach(), frozen[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 33, 2500])
def test_gradient_against_the_reference(n):
    """a lone lane, a partial 32-point tile, many tiles per wave"""
    dev = torch.device("cuda:0")
    params, pos, cot, ref, floors = _reference(str(n))
    grad = _hip_gradient(_net(params, dev), pos.to(dev), tuple(c.to(dev) for c in cot)).cpu()
    assert grad.shape == (ng.n_params(),) and bool(torch.isfinite(grad).all())
    _check_bars(grad, ref, floors, "n = %d" % n)
    assert float(grad[8192 + 5 * 64:N_MLP].abs().max()) == 0.0                       # rows 5 .. 15 of dW3
    assert float(grad[N_MLP:][ref[N_MLP:] == 0].abs().max()) == 0.0                  # table entries no point touches


@pytest.mark.gpu
def test_gradient_across_the_chunk_boundary():
    """2^20 + 77 points, cotangents zero except at the first 100, 123 straddling 2^20 and the last 77: the gradient of those 300 points alone"""
    dev = torch.device("cuda:0")
    params, pos, cot, ref, floors = _reference("chunk")
    grad = _hip_gradient(_net(params, dev), pos.to(dev), tuple(c.to(dev) for c in cot)).cpu()
    _check_bars(grad, ref, floors, "chunk boundary")
    assert float(grad[8192 + 5 * 64:N_MLP].abs().max()) == 0.0
    assert float(grad[N_MLP:][ref[N_MLP:] == 0].abs().max()) == 0.0


@pytest.mark.gpu
def test_reproducibility_and_accumulation():
    dev = torch.device("cuda:0")
    params, pos, cot, ref, floors = _reference("2500")
    net = _net(params, dev)
    pos, cot = pos.to(dev), tuple(c.to(dev) for c in cot)
    g1 = torch.zeros(ng.n_params(), device=dev); g2 = torch.zeros_like(g1); g3 = torch.full_like(g1, 0.5)
    assert _raw_backward(net, pos, cot, g1) == 0 and _raw_backward(net, pos, cot, g2) == 0 and _raw_backward(net, pos, cot, g3) == 0
    assert torch.equal(g1[:N_MLP], g2[:N_MLP])                                       # the slab reducer: bitwise
    _check_bars(g2.cpu(), ref, floors, "second call")
    assert torch.equal(g3[:N_MLP], g1[:N_MLP] + 0.5)                                 # ADDED to: one f32 add per weight
    _check_bars((g3.double() - 0.5).cpu(), ref, floors, "pre-filled buffer")
    assert float((g3[N_MLP:] - 0.5)[(ref[N_MLP:] == 0).to(dev)].abs().max()) == 0.0


@pytest.mark.gpu
def test_device_refresh_after_an_optimizer_step():
    from iris_amd.model.brdf import NGPBRDF
    dev = torch.device("cuda:0")
    params, pos, cot, _, _ = _reference("2500")
    net = _net(params, dev)
    pos, cot = pos.to(dev), tuple(c.to(dev) for c in cot)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    _hip_gradient(net, pos, cot)
    handle = net._native.ptr.value
    before = net.mlp.params.detach().clone()
    opt.step()
    assert not torch.equal(before, net.mlp.params.detach())
    with torch.no_grad():
        out = net(pos)
    assert net._native.ptr.value == handle                                                   # refreshed in place, not re-created
    fresh = NGPBRDF(VMIN, VMAX)
    fresh.load_state_dict({"mlp.params": net.mlp.params.detach().cpu()})            # CPU-resident, frozen: the host path
    ref = fresh(pos)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.gpu
def test_trainer_shaped_step():
    """train_brdf_crf.py:163-207: material(positions) -> kd / ks combine over the cached shading -> loss -> backward()"""
    from iris_amd.utils.shading_cache import ShadingCache
    dev = torch.device("cuda:0")
    n = 1000
    net = _net(_params(4, 0.3), dev)
    pos = _positions(n, 5).to(dev)
    g = torch.Generator().manual_seed(6)
    cache = ShadingCache(n, 6, dev)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=g).to(dev))
    target = torch.rand(n, 3, generator=g).to(dev)
    mat = net(pos)
    rgb = cache.shade(None, mat["albedo"], mat["metallic"], mat["roughness"])
    torch.nn.functional.mse_loss(rgb, target).backward()
    grad = net.mlp.params.grad.cpu()
    assert bool(torch.isfinite(grad).all())
    blocks = _blocks()
    assert all(float(grad[sl].abs().max()) > 0 for _, sl in blocks[:3])
    assert sum(float(grad[sl].abs().max()) > 0 for _, sl in blocks[3:]) >= 30


CURVE_MARGIN = 3.1e-4     # twice the largest relative gap of the first MI355X run (1.542e-4, at step 8)


@pytest.mark.gpu
def test_training_curve_follows_the_oracle():
    """tools/make_ngp_train_golden.py fitted 256 points for 20 Adam steps through the oracle's autograd on the CPU (tests/golden/ngp_train_curve.npz);
    the same loop through the HIP path: every loss within CURVE_MARGIN (relative) of the golden's, and the final loss below the first.
    CURVE_MARGIN = 3.1e-4: twice the largest gap of the first run on an MI355X (1.542e-4; losses 90.54 -> 32.27 against the golden's 90.54 -> 32.26)."""
    spec = importlib.util.spec_from_file_location("make_ngp_train_golden", os.path.join(REPO, "tools", "make_ngp_train_golden.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    from iris_amd.model.brdf import NGPBRDF
    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(REPO, "tests", "golden", "ngp_train_curve.npz"))
    assert int(gold["param_seed"]) == tool.PARAM_SEED and int(gold["point_seed"]) == tool.POINT_SEED and int(gold["n_steps"]) == tool.N_STEPS
    params, pos, target = tool.problem(ng.n_params())
    net = NGPBRDF(tool.VOXEL_MIN, tool.VOXEL_MAX)
    net.load_state_dict({"mlp.params": params})
    net.to(dev)
    net.mlp.params.requires_grad_(True)
    opt = torch.optim.Adam(net.parameters(), lr=float(gold["lr"]))
    pos, target = pos.to(dev), target.to(dev)
    losses = []
    for step in range(tool.N_STEPS + 1):
        opt.zero_grad(set_to_none=True)
        loss = tool.loss_of(net(pos), target)
        losses.append(float(loss.detach()))
        if step < tool.N_STEPS:
            loss.backward()
            opt.step()
    losses, want = np.asarray(losses), gold["losses"]
    gap = np.abs(losses - want) / want
    print("training curve: hip", np.round(losses, 4).tolist(), "golden", np.round(want, 4).tolist(), "largest relative gap %.3e" % gap.max())
    assert losses[-1] < losses[0]
    assert float(gap.max()) <= CURVE_MARGIN, gap.tolist()


@pytest.mark.gpu
def test_errors_and_empty_input():
    from iris_amd import _lib as L
    from iris_amd.model.brdf import NGPBRDF
    dev = torch.device("cuda:0")
    params = _params(4, 0.3)
    net = _net(params, dev)
    with pytest.raises(L.IrisError):
        net(_positions(4, 1).to(dev).requires_grad_(True))
    cpu_net = NGPBRDF(VMIN, VMAX)
    cpu_net.load_state_dict({"mlp.params": params})
    cpu_net.mlp.params.requires_grad_(True)
    with pytest.raises(L.IrisError, match="to\\(device\\)"):
        cpu_net(_positions(4, 1).to(dev))
    out = net(torch.empty(0, 3, device=dev))
    assert out["albedo"].shape == (0, 3) and out["roughness"].shape == (0, 1) and out["metallic"].shape == (0, 1)
    (out["albedo"].sum() + out["roughness"].sum() + out["metallic"].sum()).backward()
    assert net.mlp.params.grad.shape == (ng.n_params(),) and float(net.mlp.params.grad.abs().max()) == 0.0
    pos, cot = _positions(100, 2).to(dev), tuple(c.to(dev) for c in _cotangents(100, 3))
    grad = torch.zeros(ng.n_params(), device=dev)
    need = int(L.lib().iris_ngp_backward_workspace_bytes(100))
    assert _raw_backward(net, pos, cot, grad, workspace_bytes=need - 1) == 1           # IRIS_ERR_ARG
    assert "workspace" in L.lib().iris_last_error().decode()
    assert float(grad.abs().max()) == 0.0
