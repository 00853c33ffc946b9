"""The fused Adam step on the GPU: iris_adam_step / iris_ngp_adam_step (iris_amd/csrc/iris_optim.h), FusedAdam (iris_amd/utils/optim.py) and
NGPBRDF.adam_step_.

The kernels are pinned BIT FOR BIT to tests/adam_ref.py, the numpy float32 restatement of the arithmetic in include/iris_hip.h: the scalars formed in
double and rounded once, every per-element operation a separate float32 operation (the library is compiled with -ffp-contract=off, and HIP's float32
division and sqrtf are correctly rounded by default).  tests/test_fused_adam_cpu.py pins that restatement to torch.optim.Adam: its error against
torch's float64 Adam is at most 4 x the error of torch's own float32 Adam (measured there: 1.0 - 1.4 x); the factor allows for a different but equally
valid order of float32 operations.  The same bound is used here where a result is compared with torch's."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import adam_ref
from conftest import REPO

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -777.25, 64          # PAD floats = 256 B: a view at PAD is 16-byte aligned, at PAD + 1 it is not
LRS = [1e-3, 1e-3, 1e-3, 5e-4, 5e-4, 5e-4]
SIZES = [0, 1, 3, 7, 8, 9, 255, 256, 257, 4101]
BOUND = 4.0


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def hip_adam(p, g, m, v, step, lr, wd=0.0, beta1=0.9, beta2=0.999, eps=1e-8, n=None):
    from iris_amd import _lib as L
    return L.lib().iris_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel() if n is None else n, step, lr, beta1, beta2, eps, wd, L.stream())


def guarded(values, offset):
    """(whole buffer, view of len(values) floats at PAD + offset): the view holds `values`, everything around it the sentinel"""
    n = len(values)
    buf = torch.full((PAD + offset + n + PAD,), SENTINEL, device="cuda")
    view = buf[PAD + offset:PAD + offset + n]
    view.copy_(torch.from_numpy(np.asarray(values, np.float32)))
    assert n == 0 or view.data_ptr() % 16 == (4 * offset) % 16          # (an empty view has no address)
    return buf, view


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_adam_step_equals_the_restatement_bit_for_bit(weight_decay, offset):
    from iris_amd import _lib as L
    for n in SIZES:
        p0, grads = adam_ref.problem(n, 100 + n, len(LRS))
        want = adam_ref.run(p0, grads, LRS, weight_decay=weight_decay)
        (pb, p), (mb, m), (vb, v) = guarded(p0, offset), guarded(np.zeros(n), offset), guarded(np.zeros(n), offset)
        for k, (g_host, lr) in enumerate(zip(grads, LRS)):
            gb, g = guarded(g_host, offset)
            L.check(hip_adam(p, g, m, v, k + 1, lr, weight_decay))
            assert same_bits(g, g_host) and bool((gb[:PAD + offset] == SENTINEL).all()) and bool((gb[PAD + offset + n:] == SENTINEL).all())
        for name, buf, view, ref in (("p", pb, p, want[0]), ("exp_avg", mb, m, want[1]), ("exp_avg_sq", vb, v, want[2])):
            differ = int((bits(view) != bits(ref)).sum())
            assert differ == 0, f"n {n}, {name}: {differ} entries differ from the restatement, largest gap {np.abs(view.cpu().numpy() - ref).max():.3e}"
            assert bool((buf[:PAD + offset] == SENTINEL).all()) and bool((buf[PAD + offset + n:] == SENTINEL).all()), f"n {n}, {name}: written outside the buffer"


def test_invalid_arguments_launch_nothing():
    from iris_amd import _lib as L
    p0, grads = adam_ref.problem(16, 1, 1)
    p, g, m, v = (torch.from_numpy(a).cuda() for a in (p0, grads[0], np.zeros(16, np.float32), np.zeros(16, np.float32)))
    for kw in (dict(step=0), dict(n=-1), dict(lr=float("inf")), dict(lr=float("nan")), dict(lr=0.0), dict(beta2=1.0), dict(wd=-1.0), dict(eps=0.0)):
        args = dict(step=1, lr=1e-3)
        args.update(kw)
        assert hip_adam(p, g, m, v, **args) != 0, kw
        assert L.lib().iris_last_error().decode().startswith("iris_adam_step"), kw
        torch.cuda.synchronize()
        assert same_bits(p, p0) and not bool(m.any()) and not bool(v.any()), kw
    assert L.lib().iris_adam_step(None, L.ptr(g), L.ptr(m), L.ptr(v), 16, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, L.stream()) != 0
    assert L.lib().iris_adam_step(None, None, None, None, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, L.stream()) == 0          # n = 0: a no-op


def test_fused_adam_steps_two_tensors_and_skips_one_without_gradient():
    from iris_amd import _lib as L
    from iris_amd.utils.optim import FusedAdam
    problems = [adam_ref.problem(n, 7 + n, 3) for n in (9, 1000)]
    params = [torch.nn.Parameter(torch.from_numpy(p0).cuda()) for p0, _ in problems]
    idle = torch.nn.Parameter(torch.arange(5, dtype=torch.float32, device="cuda"))
    opt = FusedAdam(params + [idle], lr=1e-3, weight_decay=1e-2)
    lrs = [1e-3, 1e-3, 2.5e-4]
    versions = [p._version for p in params]
    for k, lr in enumerate(lrs):
        opt.param_groups[0]["lr"] = lr                        # read at every step: a scheduler works
        for p, (_, grads) in zip(params, problems):
            p.grad = torch.from_numpy(grads[k]).cuda()
        opt.step()
    for p, (p0, grads), before in zip(params, problems, versions):
        want = adam_ref.run(p0, grads, lrs, weight_decay=1e-2)
        st = opt.state[p]
        assert same_bits(p, want[0]) and same_bits(st["exp_avg"], want[1]) and same_bits(st["exp_avg_sq"], want[2])
        assert p._version >= before + len(lrs)
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 3.0
    assert torch.equal(idle.detach().cpu(), torch.arange(5, dtype=torch.float32)) and idle._version == 0 and len(opt.state[idle]) == 0
    for bad, grad in ((torch.nn.Parameter(torch.zeros(4)), torch.zeros(4)), (torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float64)), torch.zeros(4, device="cuda", dtype=torch.float64)),
                      (torch.nn.Parameter(torch.zeros(4, 4, device="cuda").t()), torch.zeros(4, 4, device="cuda")),
                      (torch.nn.Parameter(torch.zeros(4, 4, device="cuda")), torch.zeros(4, 4, device="cuda").to_sparse())):
        bad.grad = grad
        with pytest.raises(L.IrisError):
            FusedAdam([bad]).step()


def test_state_dicts_travel_between_fused_adam_and_torch_adam():
    from iris_amd.utils.optim import FusedAdam
    n = 4096
    p0, grads = adam_ref.problem(n, 9, 3)
    lr, wd = 1e-3, 1e-2

    def run(make, steps, p=None, state=None):
        p = torch.nn.Parameter(torch.from_numpy(p0).cuda()) if p is None else p
        opt = make([p])
        if state is not None:
            opt.load_state_dict(state)
        for k in steps:
            p.grad = torch.from_numpy(grads[k]).cuda()
            opt.step()
        return p, opt

    fused = lambda ps: FusedAdam(ps, lr=lr, weight_decay=wd)
    plain = lambda ps: torch.optim.Adam(ps, lr=lr, weight_decay=wd)
    ref = torch.nn.Parameter(torch.from_numpy(p0).double())
    ref_opt = torch.optim.Adam([ref], lr=lr, weight_decay=wd, foreach=False)
    for k in range(3):
        ref.grad = torch.from_numpy(grads[k]).double()
        ref_opt.step()
    want = [t.detach().numpy() for t in (ref, ref_opt.state[ref]["exp_avg"], ref_opt.state[ref]["exp_avg_sq"])]
    t_p, t_opt = run(plain, range(3))                                            # torch's float32 Adam on the GPU all the way: the yardstick
    f2_p, f2_opt = run(fused, range(2))
    t2_p, t2_opt = run(plain, range(2))
    t2_state = [bits(t).copy() for t in (t2_p, t2_opt.state[t2_p]["exp_avg"], t2_opt.state[t2_p]["exp_avg_sq"])]
    a_p, a_opt = run(plain, [2], p=torch.nn.Parameter(f2_p.detach().clone()), state=copy.deepcopy(f2_opt.state_dict()))        # FusedAdam's state into torch's Adam
    b_p, b_opt = run(fused, [2], p=torch.nn.Parameter(t2_p.detach().clone()), state=copy.deepcopy(t2_opt.state_dict()))        # torch's state into FusedAdam
    c_p, c_opt = f2_p, f2_opt                                                                                     # (the loads above took deep copies of the state)
    c_p.grad = torch.from_numpy(grads[2]).cuda()
    c_opt.step()                                                                                                 # FusedAdam all the way
    assert float(a_opt.state[a_p]["step"]) == 3.0 and float(b_opt.state[b_p]["step"]) == 3.0
    # the two results FusedAdam made equal the restatement bit for bit
    for got, ref_bits in zip((c_p, c_opt.state[c_p]["exp_avg"], c_opt.state[c_p]["exp_avg_sq"]), adam_ref.run(p0, grads, [lr] * 3, weight_decay=wd)):
        assert same_bits(got, ref_bits)
    t2_p0, t2_m, t2_v = (a.view(np.float32) for a in t2_state)
    from_torch = adam_ref.adam_step(t2_p0, grads[2], t2_m, t2_v, 3, lr, weight_decay=wd)
    for got, ref_bits in zip((b_p, b_opt.state[b_p]["exp_avg"], b_opt.state[b_p]["exp_avg_sq"]), from_torch):
        assert same_bits(got, ref_bits)
    # and all three agree with torch's within the bound of the CPU test
    err = lambda tensors: [float(np.abs(t.detach().double().cpu().numpy() - w).max()) for t, w in zip(tensors, want)]
    triple = lambda p, opt: (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
    yard = err(triple(t_p, t_opt))
    for label, p, opt in (("fused -> torch", a_p, a_opt), ("torch -> fused", b_p, b_opt), ("fused", c_p, c_opt)):
        e = err(triple(p, opt))
        print(f"{label}: error against float64 Adam {['%.3e' % x for x in e]}, torch float32 on the GPU {['%.3e' % x for x in yard]}")
        assert all(y > 0 and x <= BOUND * y for x, y in zip(e, yard)), (label, e, yard)


def _ngp_problem(dev):
    """(parameters on the CPU, their gradient after a backward at 256 points on `dev`, the network it was taken with)"""
    from iris_amd import _lib as L
    from iris_amd.model.brdf import NGPBRDF
    n = int(L.lib().iris_ngp_n_params())
    params = (torch.rand(n, generator=torch.Generator().manual_seed(31)) * 2 - 1) * 0.3
    net = NGPBRDF(-2.0, 2.5)
    net.load_state_dict({"mlp.params": params})
    net.to(dev)
    net.mlp.params.requires_grad_(True)
    g = torch.Generator().manual_seed(32)
    pos = (torch.rand(256, 3, generator=g) * 4.5 - 2.0).to(dev)
    cot = [torch.randn(256, c, generator=g).to(dev) for c in (3, 1, 1)]
    out = net(pos)
    (out["albedo"] * cot[0]).sum().add((out["roughness"] * cot[1]).sum()).add((out["metallic"] * cot[2]).sum()).backward()
    return params, net.mlp.params.grad.detach().clone(), net


@pytest.mark.parametrize("handle", ["after_a_forward", "created_in_the_step"])
def test_ngpbrdf_step_updates_parameters_and_the_half_copy_in_one_pass(handle):
    from iris_amd import _lib as L
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.utils.optim import FusedAdam
    dev = torch.device("cuda:0")
    params, grad, net = _ngp_problem(dev)
    assert 0 < int((grad == 0).sum()) < grad.numel() and bool(torch.isfinite(grad).all())
    if handle == "created_in_the_step":
        net = NGPBRDF(-2.0, 2.5)
        net.load_state_dict({"mlp.params": params})
        net.to(dev)
        net.mlp.params.requires_grad_(True)
        net.mlp.params.grad = grad.clone()
        assert net._native.ptr is None
    else:
        assert net._native.ptr is not None
    p = net.mlp.params
    before_handle = net._native.ptr.value if net._native.ptr is not None else None
    before, version = p.detach().clone(), p._version
    # the plain kernel on copies
    want_p, want_m, want_v = before.clone(), torch.zeros_like(before), torch.zeros_like(before)
    L.check(hip_adam(want_p, grad, want_m, want_v, 1, 1e-2))
    opt = FusedAdam(net.parameters(), lr=1e-2, networks=[net])
    opt.step()
    st = opt.state[p]
    assert torch.equal(p.detach().view(torch.int32), want_p.view(torch.int32))
    assert torch.equal(st["exp_avg"].view(torch.int32), want_m.view(torch.int32)) and torch.equal(st["exp_avg_sq"].view(torch.int32), want_v.view(torch.int32))
    assert not torch.equal(p.detach(), before) and p._version > version
    untouched = grad == 0
    assert torch.equal(p.detach()[untouched].view(torch.int32), before[untouched].view(torch.int32))
    assert net._native.ptr is not None and net._native.keys[0].fresh(p)
    if before_handle is not None:
        assert net._native.ptr.value == before_handle
    handle_after = net._native.ptr.value
    pos = (torch.rand(64, 3, generator=torch.Generator().manual_seed(33)) * 4.5 - 2.0).to(dev)
    with torch.no_grad():
        out = net(pos)
    assert net._native.ptr.value == handle_after and net._native.keys[0].fresh(p)                # neither re-created nor refreshed
    fresh = NGPBRDF(-2.0, 2.5)
    fresh.load_state_dict({"mlp.params": p.detach().cpu()})                                     # CPU-resident, frozen: the host path
    ref = fresh(pos)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    # existing behaviour: torch.optim.Adam, then a forward, still refreshes through iris_ngp_set_params_dev
    p.grad = grad.clone()
    torch.optim.Adam(net.parameters(), lr=1e-2).step()
    assert not net._native.keys[0].fresh(p)
    with torch.no_grad():
        out = net(pos)
    assert net._native.ptr.value == handle_after and net._native.keys[0].fresh(p)
    fresh.load_state_dict({"mlp.params": p.detach().cpu()})
    ref = fresh(pos)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


CURVE_MARGIN = 3.1e-4     # tests/test_ngp_backward.py: the project's margin for the same loop under torch.optim.Adam


def test_training_curve_with_fused_adam_follows_the_oracle():
    """the 20-step fit of tests/golden/ngp_train_curve.npz (tools/make_ngp_train_golden.py's problem / loss_of) with FusedAdam in place of torch.optim.Adam"""
    spec = importlib.util.spec_from_file_location("make_ngp_train_golden", os.path.join(REPO, "tools", "make_ngp_train_golden.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    from iris_amd import _lib as L
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.utils.optim import FusedAdam
    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(REPO, "tests", "golden", "ngp_train_curve.npz"))
    assert int(gold["param_seed"]) == tool.PARAM_SEED and int(gold["point_seed"]) == tool.POINT_SEED and int(gold["n_steps"]) == tool.N_STEPS
    params, pos, target = tool.problem(int(L.lib().iris_ngp_n_params()))
    net = NGPBRDF(tool.VOXEL_MIN, tool.VOXEL_MAX)
    net.load_state_dict({"mlp.params": params})
    net.to(dev)
    net.mlp.params.requires_grad_(True)
    opt = FusedAdam(net.parameters(), lr=float(gold["lr"]), networks=[net])
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
    print("training curve: fused", np.round(losses, 4).tolist(), "golden", np.round(want, 4).tolist(), "largest relative gap %.3e" % gap.max())
    assert losses[-1] < losses[0]
    assert float(gap.max()) <= CURVE_MARGIN, gap.tolist()
