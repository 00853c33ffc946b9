"""What of the BRDF-CRF training stage can be checked without a GPU: the arithmetic the fused Adam kernel is pinned to (tests/adam_ref.py) against
torch.optim.Adam, the learning-rate schedule, and the checkpoint's layout."""
import functools
import os

import numpy as np
import pytest
import torch

import adam_ref

N, STEPS, LR = 4096, 12, 1e-3
BOUND = 4.0          # times torch's own float32 error: a different but equally valid order of float32 operations (see the module docstring of the GPU test)


def torch_adam(p0, grads, lrs, weight_decay, dtype):
    """torch.optim.Adam(foreach=False) on the CPU in `dtype` -> (p, exp_avg, exp_avg_sq) as float64 arrays"""
    p = torch.nn.Parameter(torch.from_numpy(p0).to(dtype).clone())         # (.to() of the same dtype shares p0's memory)
    opt = torch.optim.Adam([p], lr=lrs[0], weight_decay=weight_decay, foreach=False)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = torch.from_numpy(g).to(dtype)
        opt.step()
    st = opt.state[p]
    return tuple(t.detach().double().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


@functools.lru_cache(maxsize=None)
def references(weight_decay):
    """(problem, lrs, float64 result, float32 result) of torch.optim.Adam: computed once per weight decay, shared, never written to"""
    p0, grads = adam_ref.problem(N, 5, STEPS)
    lrs = [LR] * (STEPS // 2) + [LR / 2] * (STEPS - STEPS // 2)
    return p0, grads, lrs, torch_adam(p0, grads, lrs, weight_decay, torch.float64), torch_adam(p0, grads, lrs, weight_decay, torch.float32)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_restatement_against_torch_adam_in_float64(weight_decay):
    """12 steps, the learning rate halved after 6; parameters at 1e-4 and 0.3; gradients 1e-12 .. 1, half of them zero.  The largest absolute error of
    p, m and v against float64 torch.optim.Adam is at most 4 x the error of torch's own float32 CPU Adam on the same inputs."""
    p0, grads, lrs, want, torch32 = references(weight_decay)
    assert all(int((g == 0).sum()) == N // 2 for g in grads)
    got = adam_ref.run(p0, grads, lrs, weight_decay=weight_decay)
    for name, mine, ref, t32 in zip(("p", "exp_avg", "exp_avg_sq"), got, want, torch32):
        err, yard = float(np.abs(mine.astype(np.float64) - ref).max()), float(np.abs(t32 - ref).max())
        print(f"wd {weight_decay}: {name}: restatement error {err:.3e}, torch float32 error {yard:.3e}, ratio {err / yard:.2f}, "
              f"bit-equal to torch float32: {np.array_equal(mine.astype(np.float64), t32)}")
        assert yard > 0 and err <= BOUND * yard, (name, err, yard)


def test_one_minus_beta2_in_float_is_not_the_contract():
    """1 - float32(beta2) differs from float32(1 - beta2) by 6e-5 relative: the scalars are formed in double"""
    s = adam_ref.adam_scalars(3, 1e-3)
    assert s["w2"] == np.float32(1.0 - 0.999) and s["w2"] != np.float32(1) - np.float32(0.999)
    assert s["step_size"] == np.float32(1e-3 / (1.0 - 0.9 ** 3)) and s["bc2"] == np.float32(np.sqrt(1.0 - 0.999 ** 3))


@pytest.mark.parametrize("milestones", [[], [3], [2, 5]])
@pytest.mark.parametrize("gamma", [0.5, 0.1])
def test_multistep_lr_is_torchs_schedule(milestones, gamma):
    from iris_amd.train_brdf_crf import multistep_lr
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=gamma)
    for epoch in range(10):
        assert multistep_lr(1e-3, milestones, gamma, epoch) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-14), epoch     # (torch multiplies step by step)
        opt.step()
        sched.step()
    assert multistep_lr(1e-3, [2, 5], 0.5, 5) == 1e-3 * 0.25


def test_checkpoint_round_trip(tmp_path):
    from iris_amd.train_brdf_crf import read_checkpoint, write_checkpoint
    g = torch.Generator().manual_seed(3)
    material = torch.nn.Module()
    material.mlp = torch.nn.Module()
    material.mlp.params = torch.nn.Parameter(torch.randn(1000, generator=g))
    crf = torch.nn.Module()
    crf.register_buffer("f0", torch.rand(1, 16, generator=g))
    crf.register_buffer("basis", torch.rand(3, 16, generator=g))
    crf.weight = torch.nn.Parameter(torch.randn(3, 3, generator=g))
    params = [material.mlp.params, crf.weight]
    opt = torch.optim.Adam(params, lr=2e-3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    opt.step()
    path = os.path.join(tmp_path, "exp", "last.ckpt")
    write_checkpoint(path, material.state_dict(), crf.state_dict(), opt.state_dict(), epoch=3, global_step=41, hyper_parameters=dict(learning_rate=2e-3, milestones=[1000]))
    assert os.listdir(os.path.dirname(path)) == ["last.ckpt"]

    # the reference's loaders (refine_shading.py:84-89, train_brdf_crf.py:72-97)
    state_dict = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
    assert set(state_dict) == {"material.mlp.params", "model_crf.f0", "model_crf.basis", "model_crf.weight"}
    weight = {k.replace("material.", ""): v for k, v in state_dict.items() if "material." in k}
    assert list(weight) == ["mlp.params"] and torch.equal(weight["mlp.params"], material.mlp.params.detach())
    weight = {k.replace("model_crf.", ""): v for k, v in state_dict.items() if "model_crf." in k}
    assert torch.equal(weight["weight"], crf.weight.detach()) and torch.equal(weight["f0"], crf.f0) and torch.equal(weight["basis"], crf.basis)

    ck = read_checkpoint(path)
    assert ck["epoch"] == 3 and ck["global_step"] == 41 and ck["hyper_parameters"] == dict(learning_rate=2e-3, milestones=[1000])
    assert torch.equal(ck["material"]["mlp.params"], material.mlp.params.detach()) and torch.equal(ck["model_crf"]["weight"], crf.weight.detach())
    fresh = [torch.nn.Parameter(torch.zeros_like(p)) for p in params]
    other = torch.optim.Adam(fresh, lr=1.0)
    other.load_state_dict(ck["optimizer_states"][0])
    assert other.param_groups[0]["lr"] == 2e-3
    for a, b in zip(params, fresh):
        assert torch.equal(opt.state[a]["exp_avg"], other.state[b]["exp_avg"]) and torch.equal(opt.state[a]["exp_avg_sq"], other.state[b]["exp_avg_sq"])
        assert float(other.state[b]["step"]) == 1.0


def test_ranger_is_a_clear_error():
    from iris_amd import _lib as L
    from iris_amd.train_brdf_crf import make_optimizer
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(L.IrisError, match="Ranger"):
        make_optimizer("Ranger", [p], 1e-3, 0.0, networks=())
    assert isinstance(make_optimizer("SGD", [p], 1e-3, 0.0, networks=()), torch.optim.SGD)
