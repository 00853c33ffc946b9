"""NGPBRDF on an MI355X in the regime the trainer runs it in (tests/ngp_ref64.py: inputs, restated backward, per-element envelope; tests/test_ngp_regime_cpu.py
vouches for them without a GPU).

  forward   the encoding of fresh-init and checkpoint-like tables bit for bit (subnormal halves, ties, values that round to zero); the exact network with
            SUBNORMAL operands on the matrix cores, to the exact bar of test_ngp.py (a v_mfma_f32_32x32x16_f16 that flushed subnormal A / B inputs would output 0.5
            everywhere: every output off by up to 0.498); both ends of the half output stage; the three ways the handle's half copy of the parameters is written
  backward  every element of the gradient within C tol_i of the float64 definition (C = 4 E, E measured here again from the restatement alone), for
            {init, uniform, mixed} x cotangent scales {1, 3e-5, 1e-6} x {1, 33, 2500} points, 2 500 points clustered in one coarse cell, and two saturated inputs;
            rows 5 .. 15 of dW3 and untouched table entries exactly zero; the matrices' gradient bitwise equal on a second call

Measured on an MI355X: the exact networks come out equal to the restatement in every output (0 beyond 3e-7): the f16 MFMA keeps subnormal A / B inputs; the worst
|err| / (C tol) of every class on every input is 0.232 .. 0.276 (0.25 = the restatement itself), block relative L2 within 0.3 % of the restatement's.  DESIGN.md section 5f."""
import numpy as np
import pytest
import torch

import ngp_ref64 as R
from ngp_ref64 import N_MLP, VMAX, VMIN, ng
from test_ngp_backward import _hip_gradient, _net


def _encode(net, pos, dev):
    """iris_debug_ngp_encode -> (32, n, 2) half bits"""
    from iris_amd import _lib as L
    n = pos.shape[0]
    feat = torch.zeros(32, n, dtype=torch.int32, device=dev)
    L.check(L.lib().iris_debug_ngp_encode(net._handle(dev), L.ptr(pos.to(dev)), n, L.ptr(feat), L.stream()))
    torch.cuda.synchronize()
    return feat.cpu().numpy().view(np.uint16).reshape(32, n, 2)


def _encode_ref(params, pos):
    return ng.encode(params, R.encoder_input(pos)).numpy().view(np.uint16).reshape(pos.shape[0], 32, 2).transpose(1, 0, 2)


def _host_net(params, vmin=VMIN, vmax=VMAX):
    """CPU-resident, frozen: iris_ngp_create converts the parameters on the host"""
    from iris_amd.model.brdf import NGPBRDF
    net = NGPBRDF(vmin, vmax)
    net.load_state_dict({"mlp.params": params})
    return net


@pytest.mark.gpu
def test_init_parameters_are_the_modules():
    from iris_amd.model.brdf import NGPBRDF
    assert torch.equal(NGPBRDF(VMIN, VMAX).init_parameters(1337).mlp.params.detach(), R.parameters("init"))


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["init", "mixed"])
def test_encoding_bit_exact_in_the_subnormal_range(pname):
    """2(a): 3 000 points, two of them box corners"""
    dev = torch.device("cuda:0")
    params, pos = R.parameters(pname), R.encode_positions()
    ref = _encode_ref(params, pos)
    sub = float(R.is_subnormal(torch.from_numpy(ref.view(np.float16).astype(np.float32))).double().mean())
    print("%s: %.1f %% of the features are subnormal halves" % (pname, 100 * sub))
    np.testing.assert_array_equal(_encode(_host_net(params), pos, dev), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("w3_scale", [1.0, 2.0, -2.0])
def test_exact_network_with_subnormal_operands(w3_scale):
    """2(b): w3_scale 1: every feature and most activations are subnormal halves, every sum is exact in f32 in any order; 2(c): +-2: the half sigmoid rounds to
    exactly 1 (x 2) and to subnormal halves (x -2).  The bar of test_hip_forward_exact_with_dyadic_weights."""
    dev = torch.device("cuda:0")
    params, pos = R.dyadic_parameters(w3_scale)
    pos = pos[:2500]                                  # (a partial last tile; the CPU test vouches for all 4 096 points)
    out = _host_net(params, 0.0, 1.0)(pos.to(dev))
    ref = R.outputs_of(R.dyadic_forward(params, pos)["s"])
    for k in ("albedo", "roughness", "metallic"):
        diff = np.abs(out[k].cpu().numpy().astype(np.float64) - ref[k].numpy())
        print("w3 x %g, %s: max |d| %.3e, %d beyond 3e-7" % (w3_scale, k, float(diff.max()), int((diff > 3e-7).sum())))
        assert float(diff.max()) <= 2.0 ** -12 + 1e-7 and int((diff > 3e-7).sum()) <= max(2, diff.size // 2000), (k, float(diff.max()), int((diff > 3e-7).sum()))


@pytest.mark.gpu
def test_parameter_conversion_paths():
    """2(d): the handle's half copy after iris_ngp_set_params_dev, after iris_ngp_create from the host and after one NGPBRDF.adam_step_ is torch's
    float32 -> float16 on the CPU (ties to even, subnormals kept, below 2^-25 to zero), seen through the encoding and the forward outputs: bit for bit"""
    dev = torch.device("cuda:0")
    params, pos = R.parameters("mixed"), R.encode_positions(2500)
    dpos = pos.to(dev)
    host = _host_net(params)                                                      # iris_ngp_create
    want = _encode_ref(params, pos)
    np.testing.assert_array_equal(_encode(host, pos, dev), want)
    want_out = host(dpos)
    net = _net(params, dev)                                                       # iris_ngp_set_params_dev
    np.testing.assert_array_equal(_encode(net, pos, dev), want)
    with torch.no_grad():
        out = net(dpos)
    assert all(torch.equal(out[k], want_out[k]) for k in want_out)

    # one Adam step that leaves the parameters with a zero gradient where they are (the ties, the values below 2^-25) and moves the others by ~2^-18
    g = torch.Generator().manual_seed(41)
    grad = torch.randn(params.numel(), generator=g) * (torch.rand(params.numel(), generator=g) < 0.5)
    handle = net._native.ptr.value
    net.adam_step_(grad.to(dev), torch.zeros(params.numel(), device=dev), torch.zeros(params.numel(), device=dev), 1, 2.0 ** -18)
    new = net.mlp.params.detach().cpu()
    moved = new != params
    assert bool((moved == (grad != 0)).all()) and 0.4 < float(moved.double().mean()) < 0.6
    got = _encode(net, pos, dev)
    assert net._native.ptr.value == handle                                        # the step wrote the half copy: nothing re-created, nothing re-cast
    want = _encode_ref(new, pos)
    assert int((want != _encode_ref(params, pos)).sum()) > 0
    np.testing.assert_array_equal(got, want)
    with torch.no_grad():
        out = net(dpos)
    want_out = _host_net(new)(dpos)
    assert all(torch.equal(out[k], want_out[k]) for k in want_out)


@pytest.mark.gpu
@pytest.mark.parametrize("pname,kind,c", R.CASES, ids=["%s-%s-%g" % t for t in R.CASES])
def test_gradient_within_the_envelope(pname, kind, c):
    dev = torch.device("cuda:0")
    a, pos, cot, ref, res, tol, E = R.case(pname, kind, c)
    assert all(0 < E[k] <= 1.0 for k in R.CLASSES), E
    net = _net(R.parameters(pname), dev)
    dpos, dcot = pos.to(dev), tuple(t.to(dev) for t in cot)
    first = _hip_gradient(net, dpos, dcot).clone()
    second = _hip_gradient(net, dpos, dcot)
    assert torch.equal(first[:N_MLP], second[:N_MLP])                                # the slab reducer: bitwise
    grad = first.cpu()
    assert grad.shape == (ng.n_params(),) and bool(torch.isfinite(grad).all())
    got = R.compact(a, grad)
    q = R.ratios(got, ref, tol)
    print("%s n %s c %g: |err| / (C tol) %s;  E %s;  worst block L2 %.2e (restatement %.2e)" % (
        pname, kind, c, " ".join("%s %.3f" % (k, q[k] / (4 * E[k])) for k in R.CLASSES), " ".join("%.3f" % E[k] for k in R.CLASSES), R.block_l2(a, got, ref), R.block_l2(a, res, ref)))
    assert float(grad[8192 + 5 * 64:N_MLP].abs().max()) == 0.0                       # rows 5 .. 15 of dW3
    tab = grad[N_MLP:].clone().reshape(-1, 2)
    tab[a.entries] = 0.0
    assert float(tab.abs().max()) == 0.0                                             # table entries no point touches
    assert float(got[1].abs().max()) > 0.0
    bad = {k: q[k] / (4 * E[k]) for k in R.CLASSES if not q[k] <= 4 * E[k]}
    assert not bad, bad
