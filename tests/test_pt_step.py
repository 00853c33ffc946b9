"""path_tracing_single_step: the reference's training step (train_emitter.py:181-189 -- SPP // spp calls of path_tracing_single on the same rays, summed) as one
fused call.  The yardstick everywhere is the EXISTING per-call function: `L = zeros; L += path_tracing_single(..., spp, uniforms=u_c, compact=False)` over the calls.
Scene and rays: the box room of tests/golden/bake_box.npz / pt_single.npz (misses and primary emitter hits included), StubMaterial, draws from a seeded CPU generator."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO, golden, rel_l2
from stub_material import StubMaterial, stub_material_np

SHAPES = [(4, 1), (3, 3), (32, 4), (70, 2)]          # (spp, n_calls): n_calls = 1; spp no power of two (partially filled lane groups); spp = 32; spp > 64 (rounds of 64)
TILE_PATHS = (1, 1 << 40)                            # iris_debug_set("pt_tile_min"): every call through the tile kernels / through the one-ray-per-lane kernels


# --------------------------------------------------------------------------------------------------------- CPU
def test_step_abi_and_import():
    """the two entry points are declared, bound with matching arity and exported; the public function imports and rejects CPU tensors"""
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import path_tracing_single_step
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "iris_hip.h")).read(), flags=re.S)
    exported = set(re.findall(r" T (iris_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()))
    for name in ("iris_pt_step_accumulate_fwd", "iris_pt_step_accumulate_bwd"):
        m = re.search(r"IRIS_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name + " is not declared in include/iris_hip.h"
        assert len(m.group(1).split(",")) == len(L.PROTOTYPES[name]), name
        assert name in exported, name
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name]
    r = torch.rand(4, 3)
    with pytest.raises(L.IrisError):
        path_tracing_single_step(None, None, StubMaterial(), r, r, r, r, 2, 2)


# --------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def box(tmp_path_factory):
    from test_pt_single import _gpu_setup
    dev = torch.device("cuda:0")
    g, p, sc, em = _gpu_setup(tmp_path_factory.mktemp("pt_step"), dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    return {"dev": dev, "g": g, "p": p, "sc": sc, "em": em, "rays": [T(p[k]) for k in ("rays_o", "rays_d", "dx_du", "dy_dv")]}


def _draws(B, spp, n_calls, seed, dev):
    """n_calls entries of the five draws of a call, in the un-compacted shapes"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [[torch.rand(*s, generator=gen).to(dev) for s in ((2, B, spp), (B * spp,), (B * spp, 2), (B * spp,), (B * spp, 2))] for _ in range(n_calls)]


def _continues(box, rays, dudv, spp):
    """which of the B * spp paths of a call continue after the primary hit (a hit that is no emitter), as test_pt_single derives it"""
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import ray_intersect
    dev, B = box["dev"], rays[0].shape[0]
    wi = torch.empty(B * spp, 3, device=dev)
    dudv = dudv.reshape(2, B, spp).contiguous()
    L.check(L.lib().iris_pt_jitter(L.ptr(rays[1]), L.ptr(rays[2]), L.ptr(rays[3]), L.ptr(dudv), B, spp, L.ptr(wi), L.stream()))
    _, _, _, tri, _ = ray_intersect(box["sc"], rays[0].repeat_interleave(spp, 0), wi)
    e0 = torch.empty(B * spp, device=dev, dtype=torch.int32); vn = torch.empty(B * spp, device=dev, dtype=torch.bool)
    L.check(L.lib().iris_pt_primary_emit(box["em"].handle(dev), L.ptr(tri), B * spp, L.ptr(e0), L.ptr(vn), L.stream()))
    return vn


def _loop(box, rays, spp, unif, mat=None, **kw):
    from iris_amd.utils.path_tracing import path_tracing_single
    mat = mat if mat is not None else StubMaterial()
    Lsum = torch.zeros(rays[0].shape[0], 3, device=box["dev"])
    for u in unif:
        Lsum += path_tracing_single(box["sc"], box["em"], mat, *rays, spp, uniforms=u, compact=False, **kw).detach()
    return Lsum


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays", [256, 37])
@pytest.mark.parametrize("spp,n_calls", SHAPES)
def test_step_forward_equals_the_loop_bit_for_bit(box, spp, n_calls, n_rays):
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import path_tracing_single_step
    rays = [r[:n_rays].contiguous() for r in box["rays"]]
    assert rays[0].shape[0] == n_rays
    unif = _draws(n_rays, spp, n_calls, 100 * spp + n_calls, box["dev"])
    if n_rays == 256:                                   # the fixture's rays: some paths end at the primary hit (misses, emitters), and are masked
        for u in unif:
            n_cont = int(_continues(box, rays, u[0], spp).sum())
            assert 0 < n_cont < n_rays * spp
    for tile_min in TILE_PATHS:
        L.debug_set("pt_tile_min", tile_min)
        try:
            loop = _loop(box, rays, spp, unif)
            step = path_tracing_single_step(box["sc"], box["em"], StubMaterial(), *rays, spp, n_calls, uniforms=unif)
        finally:
            L.debug_set("pt_tile_min", -1)
        assert step.shape == (n_rays, 3) and float(loop.abs().sum()) > 0
        assert torch.equal(step.detach(), loop), (tile_min, float((step.detach() - loop).abs().max()))


@pytest.mark.gpu
def test_step_of_one_call_is_path_tracing_single(box):
    from iris_amd.utils.path_tracing import path_tracing_single, path_tracing_single_step
    (u,) = _draws(256, 5, 1, 7, box["dev"])
    one = path_tracing_single(box["sc"], box["em"], StubMaterial(), *box["rays"], 5, uniforms=u, compact=False)
    step = path_tracing_single_step(box["sc"], box["em"], StubMaterial(), *box["rays"], 5, 1, uniforms=[u])
    assert torch.equal(step.detach(), one.detach())


@pytest.mark.gpu
def test_step_gradient_is_the_sum_of_the_per_call_gradients(box):
    from iris_amd.utils.path_tracing import path_tracing_single, path_tracing_single_step
    em, rays, spp, n_calls = box["em"], box["rays"], 6, 3
    unif = _draws(256, spp, n_calls, 11, box["dev"])
    w = torch.rand(256, 3, generator=torch.Generator().manual_seed(1)).to(box["dev"])
    per_call = torch.zeros(em.radiance.shape, dtype=torch.float64)
    for u in unif:
        Lc = path_tracing_single(box["sc"], em, StubMaterial(), *rays, spp, uniforms=u, compact=False)
        per_call += torch.autograd.grad((Lc * w).sum(), em.radiance)[0].double().cpu()
    L = path_tracing_single_step(box["sc"], em, StubMaterial(), *rays, spp, n_calls, uniforms=unif)
    assert L.requires_grad
    (gr,) = torch.autograd.grad((L * w).sum(), em.radiance)
    assert gr.shape == em.radiance.shape and float(per_call.abs().sum()) > 0
    assert rel_l2(gr.cpu().numpy(), per_call.numpy()) <= 1e-5               # (a scatter of float atomics: equal up to summation order, the bar of tests/test_pt_single.py)
    assert bool((gr.cpu()[per_call.abs().sum(-1) == 0] == 0).all())         # rows no call lights stay exactly zero
    assert int((gr.abs().sum(-1) > 0).sum()) <= int(box["g"]["is_emitter"].sum())


@pytest.mark.gpu
def test_step_equals_the_summed_oracle_calls_bit_for_bit(box, oracle_mod):
    from test_pt_single import _box
    from iris_amd.utils.path_tracing import path_tracing_single_step
    p, rays, spp, n_calls = box["p"], box["rays"], 4, 2
    unif = _draws(256, spp, n_calls, 23, box["dev"])
    step = path_tracing_single_step(box["sc"], box["em"], StubMaterial(), *rays, spp, n_calls, uniforms=unif)
    _, _, osc, oem = _box(oracle_mod)
    acc = np.zeros((256, 3), np.float32)
    for u in unif:
        vn = _continues(box, rays, u[0], spp)                                # the call's own continuation mask compacts its draws, as the reference sizes them
        compacted = [u[0].cpu().numpy()] + [t[vn].cpu().numpy() for t in u[1:]]
        with oracle_mod.device_arithmetic():
            oL, terms = oracle_mod.path_tracing_single(osc, oem, stub_material_np, p["rays_o"], p["rays_d"], p["dx_du"], p["dy_dv"], spp, compacted, radiance=p["radiance"])
        assert len(terms["e1"]) == int(vn.sum())
        acc += oL                                                            # float32, in call order
    np.testing.assert_array_equal(step.detach().cpu().numpy(), acc)


@pytest.mark.gpu
def test_step_second_material_evaluation(box):
    """a material that declares `roughness_min` on the instance is not evaluated at the sampled hits (same bits either way); a plain callable is always evaluated
    there -- ONCE per step, not once per call"""
    from iris_amd.utils.path_tracing import path_tracing_single_step
    spp, n_calls = 4, 3
    unif = _draws(256, spp, n_calls, 31, box["dev"])
    seen = []

    class Declared(StubMaterial):
        def forward(self, x):
            seen.append(tuple(x.shape))
            return super().forward(x)
    mat = Declared()
    mat.roughness_min = 0.05                                                 # StubMaterial's roughness is 0.35 + 0.3 sin(.) >= 0.05
    res = {}
    for skip in (True, False):
        seen.clear()
        res[skip] = (path_tracing_single_step(box["sc"], box["em"], mat, *box["rays"], spp, n_calls, uniforms=unif, skip_unused_material=skip).detach(), len(seen))
    assert res[True][1] == 1 and res[False][1] == 2
    assert torch.equal(res[True][0], res[False][0])
    for skip in (True, False):
        seen.clear()

        def plain(position):
            seen.append(tuple(position.shape))
            return StubMaterial()(position)
        Lp = path_tracing_single_step(box["sc"], box["em"], plain, *box["rays"], spp, n_calls, uniforms=unif, skip_unused_material=skip)
        assert seen == [(n_calls * 256 * spp, 3)] * 2                        # 2 per step, never 2 * n_calls
        assert torch.equal(Lp.detach(), res[False][0])


@pytest.mark.gpu
def test_step_own_draws(box):
    from iris_amd.utils.path_tracing import path_tracing_single_step
    em, spp, n_calls = box["em"], 8, 3
    seen = []

    def mat(position):
        seen.append(tuple(position.shape))
        return StubMaterial()(position)
    out = []
    for _ in range(2):
        torch.manual_seed(9)
        L = path_tracing_single_step(box["sc"], em, mat, *box["rays"], spp, n_calls)
        (gr,) = torch.autograd.grad(L.sum(), em.radiance)
        assert L.shape == (256, 3) and torch.isfinite(L).all() and torch.isfinite(gr).all() and float(L.abs().sum()) > 0
        out.append((L.detach().clone(), gr))
    assert torch.equal(out[0][0], out[1][0])                                 # the same seed: the same draws
    assert seen[0] == (n_calls * 256 * spp, 3) and len(seen) == 4            # one evaluation of all the step's primary hits (+ the one at the sampled hits) per step
    torch.manual_seed(10)
    assert not torch.equal(path_tracing_single_step(box["sc"], em, mat, *box["rays"], spp, n_calls).detach(), out[0][0])


@pytest.mark.gpu
def test_step_captured_as_hip_graph(box):
    """the step draws, traces and accumulates as a linear chain on the caller's stream (no side stream, no host synchronisation): forward + backward captured once in a
    HIP graph (torch.cuda.CUDAGraph) replay to what the eager step gives for the same generator state (the backward scatter: up to summation order)"""
    from iris_amd.utils.path_tracing import path_tracing_single_step
    from tools.bench_pt_single import GpuStub
    em, rays, spp, n_calls = box["em"], box["rays"], 8, 3
    w = torch.rand(256, 3, generator=torch.Generator().manual_seed(1)).to(box["dev"])
    mat = GpuStub()

    def step():
        L = path_tracing_single_step(box["sc"], em, mat, *rays, spp, n_calls)
        (L * w).sum().backward()
        return L
    try:
        em.radiance.grad = torch.zeros_like(em.radiance)
        torch.manual_seed(21)
        L_eager = step().detach().clone(); g_eager = em.radiance.grad.clone()
        assert float(L_eager.abs().sum()) > 0 and float(g_eager.abs().sum()) > 0
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # (torch's recipe: warm up on a side stream before capturing)
            em.radiance.grad.zero_(); step()
        torch.cuda.current_stream().wait_stream(side); torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            em.radiance.grad.zero_()
            L_static = step()
        for _ in range(2):
            L_static.detach().fill_(-1.0); em.radiance.grad.fill_(-1.0)
            torch.manual_seed(21)
            graph.replay(); torch.cuda.synchronize()
            assert torch.equal(L_static.detach(), L_eager)
            assert rel_l2(em.radiance.grad.cpu().numpy(), g_eager.cpu().numpy()) <= 1e-5
    finally:
        em.radiance.grad = None


@pytest.mark.gpu
def test_step_rejects_bad_arguments(box):
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import path_tracing_single_step
    sc, em, rays, spp = box["sc"], box["em"], box["rays"], 4
    unif = _draws(256, spp, 2, 3, box["dev"])
    launched = []

    def mat(position):                                       # the first thing a step launches after its head feeds this: never reached
        launched.append(1)
        return StubMaterial()(position)
    bad_shape = [unif[0], unif[1][:2] + [unif[1][2][:-1]] + unif[1][3:]]
    cases = [dict(n_calls=0), dict(n_calls=2, spp=0), dict(n_calls=2, uniforms=unif[:1]), dict(n_calls=2, uniforms=unif + unif[:1]), dict(n_calls=2, uniforms=bad_shape),
             dict(n_calls=2, uniforms=[unif[0], unif[1][:4]]), dict(n_calls=2, uniforms=[unif[0], [t.cpu() for t in unif[1]]]),
             dict(n_calls=2, rays=[r.cpu() for r in rays]), dict(n_calls=1 << 20, spp=1 << 10)]
    for kw in cases:
        kw = dict(kw)
        with pytest.raises(L.IrisError):
            path_tracing_single_step(sc, em, mat, *kw.pop("rays", rays), kw.pop("spp", spp), kw.pop("n_calls"), **kw)
    assert not launched
