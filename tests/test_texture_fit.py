"""The trainable texture on the GPU (iris_amd/csrc/iris_texmat.h, iris_amd/model/texture.py TextureBRDF, iris_amd/utils/texture.py
fit_textures): the float fetch against the 8-bit fetch and against its numpy restatement bit for bit, the backward against the float64 restatement under a
derived bound, autograd through TextureBRDF, the fit against the restatement's fit, and the export command line with --fit_steps."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import texfit_ref as TF
from conftest import REPO
from test_texture_material import QUAD_F, QUAD_V, QUAD_VT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
KEYS = ("albedo", "roughness", "metallic")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_forward(tri, bary, ft, vt, texels):
    """iris_texture_sample_f32 on host arrays -> (B, 5) float32 numpy: albedo, roughness, metallic"""
    from iris_amd import _lib as L
    tri, bary, ft, vt, texels = dev(np.asarray(tri, np.int64)), dev(np.asarray(bary, np.float32)), dev(np.asarray(ft, np.int32)), dev(np.asarray(vt, np.float32)), dev(texels)
    B, (H, W) = tri.shape[0], texels.shape[:2]
    a, r, m = torch.empty(B, 3, device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    L.check(L.lib().iris_texture_sample_f32(L.ptr(tri), L.ptr(bary), B, L.ptr(ft), ft.shape[0], L.ptr(vt), vt.shape[0], L.ptr(texels), H, W, L.ptr(a), L.ptr(r), L.ptr(m),
                                            L.stream()))
    return torch.cat([a, r[:, None], m[:, None]], 1).cpu().numpy()


def raw_backward(tri, bary, ft, vt, texels, g, into=None):
    """iris_texture_sample_f32_bwd on host arrays, g (B, 5) float32 -> g_texels (H, W, 5) float32 numpy (added into `into`, a device tensor, when given)"""
    from iris_amd import _lib as L
    tri, bary, ft, vt, texels = dev(np.asarray(tri, np.int64)), dev(np.asarray(bary, np.float32)), dev(np.asarray(ft, np.int32)), dev(np.asarray(vt, np.float32)), dev(texels)
    B, (H, W) = tri.shape[0], texels.shape[:2]
    ga, gr, gm = dev(g[:, :3]), dev(g[:, 3]), dev(g[:, 4])
    out = torch.zeros(H, W, 5, device=DEV) if into is None else into
    L.check(L.lib().iris_texture_sample_f32_bwd(L.ptr(tri), L.ptr(bary), B, L.ptr(ft), ft.shape[0], L.ptr(vt), vt.shape[0], L.ptr(texels), H, W, L.ptr(ga), L.ptr(gr),
                                                L.ptr(gm), L.ptr(out), L.stream()))
    return out.cpu().numpy()


def folded(rng, n):
    b = rng.random((n, 2)).astype(np.float32)
    return np.where(b.sum(1, keepdims=True) > 1, np.float32(1) - b, b).astype(np.float32)


def uv_points(uv):
    """(u, v) on the identity quad -> (tri, bary): face 0 = (0, 1, 2) holds v <= u, face 1 = (0, 2, 3) the rest"""
    uv = np.asarray(uv, np.float32)
    lower = uv[:, 1] <= uv[:, 0]
    bary = np.where(lower[:, None], np.stack([uv[:, 0] - uv[:, 1], uv[:, 1]], 1), np.stack([uv[:, 0], uv[:, 1] - uv[:, 0]], 1)).astype(np.float32)
    return np.where(lower, 0, 1).astype(np.int64), bary


def edge_points(H, W, rng):
    """the quad's corners, its edges, the texel centres, the midpoints between texels and random points; then rows with tri = -1, tri = F and a NaN barycentric"""
    cx, cy = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    mx, my = np.arange(W + 1) / W, np.arange(H + 1) / H
    grid = lambda xs, ys: np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    uv = np.concatenate([grid([0.0, 1.0], [0.0, 1.0]), grid(cx, [0.0, 1.0]), grid([0.0, 1.0], cy), grid(cx, cy), grid(mx, my), grid(cx, my), rng.random((257, 2))])
    tri, bary = uv_points(uv)
    tri = np.concatenate([tri, [-1, 2, 0, 1]])
    bary = np.concatenate([bary, np.float32([[0.2, 0.3], [0.2, 0.3], [np.nan, 0.3], [0.25, np.nan]])])
    return tri, bary


@functools.lru_cache(maxsize=None)
def quad_scene():
    from iris_amd.utils.path_tracing import Scene
    return Scene(QUAD_V, QUAD_F, device=torch.device(DEV))


# ------------------------------------------------------------------------------------------------------------------------------ 1. forward against the 8-bit fetch
@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
def test_forward_equals_the_8_bit_fetch(H, W):
    """texels = byte / 255 (a float32 division): iris_texture_sample_f32 and TextureBRDF.sample equal sample_textures bit for bit -- corners, edges, texel centres,
    between texels, UVs stretched to [-1, 2] (clamped), tri = -1, tri = F, a NaN barycentric"""
    from iris_amd.model.texture import TextureBRDF, sample_textures
    rng = np.random.default_rng(10 + H)
    albedo, rm = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rm[0, 0, 0] = 2                                                                   # below the floor: 2 / 255 < 0.02
    texels = np.concatenate([albedo, rm[..., :2]], -1).astype(np.float32) / np.float32(255)
    tri, bary = edge_points(H, W, rng)
    for vt in (QUAD_VT, QUAD_VT * 3 - 1):
        want = sample_textures(dev(tri), dev(bary), QUAD_F, vt, albedo, rm)
        want = torch.cat([want[k] for k in KEYS], 1).cpu().numpy()
        got = raw_forward(tri, bary, QUAD_F, vt, texels)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        net = TextureBRDF(quad_scene(), QUAD_F, vt, albedo, rm)
        assert np.array_equal(net.texels.detach().cpu().numpy().view(np.int32), texels.view(np.int32))
        out = net.sample(dev(tri), dev(bary))
        assert out["roughness"].shape == (len(tri), 1) and out["albedo"].requires_grad
        assert np.array_equal(torch.cat([out[k] for k in KEYS], 1).detach().cpu().numpy().view(np.int32), want.view(np.int32))
        assert (got[-4:-2] == np.float32([0, 0, 0, 0.02, 0])).all() and got[:, 3].min() == np.float32(0.02)
        a, r = net.to_images()                                                        # an unfitted texture goes back to its bytes
        assert np.array_equal(a.cpu().numpy(), albedo) and np.array_equal(r.cpu().numpy()[..., :2], rm[..., :2]) and int(r[..., 2].max()) == 0


# ------------------------------------------------------------------------------------------------------------------------------ 2. forward against the restatement
@pytest.mark.parametrize("H,W,B", [(5, 7, 4097), (1, 1, 65), (37, 53, 70001)])
def test_forward_equals_the_restatement(H, W, B):
    """random float texels in [-0.5, 1.5], a quarter of the roughness texels below 0.02: the device equals the numpy float32 restatement bit for bit"""
    rng = np.random.default_rng(20 + H)
    texels = rng.uniform(-0.5, 1.5, (H, W, 5)).astype(np.float32)
    texels[..., 3] = np.where(rng.random((H, W)) < 0.25, rng.uniform(-0.3, 0.02, (H, W)), texels[..., 3]).astype(np.float32)
    tri, bary = rng.integers(-1, 3, B), folded(rng, B)
    for vt in (QUAD_VT, QUAD_VT * 3 - 1):
        ref = TF.fetch(tri, bary, QUAD_F, vt, texels)
        ref = np.concatenate([ref[k] for k in KEYS], 1)
        got = raw_forward(tri, bary, QUAD_F, vt, texels)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), np.abs(got - ref).max()
    if H * W > 1:                                                                     # (the inputs cover both sides of the floor and of [0, 1])
        assert (got[:, 3] == np.float32(0.02)).any() and (got[:, 3] > 0.5).any() and (got[:, :3] < 0).any() and (got[:, :3] > 1).any()


# ------------------------------------------------------------------------------------------------------------------------------ 3. backward against float64
BACKWARD_CASES = {
    "one point": (5, 7, 1, False),
    "1 x 1 texture": (1, 1, 100, False),
    "4096 points on 2 x 2 (contention)": (2, 2, 4096, False),
    "70 001 points on 37 x 53 (the block's tail)": (37, 53, 70001, False),
    "stretched UVs (border taps with x1 == x0)": (5, 7, 4097, True),
    "4096 * 256 + 257 points (the grid-stride loop's second pass and its tail)": (37, 53, 4096 * 256 + 257, False),
}


@pytest.mark.parametrize("case", list(BACKWARD_CASES))
def test_backward_within_the_derived_bound(case):
    """g_texels against the float64 restatement, per texel channel |g - g64| <= (n + 4) 2^-24 S, n the number of contributions and S = sum |w g| (three roundings
    of the weight, one of the product, n - 1 of the sum: derived, not measured); a texel that no point touches is exactly 0.  Every case has rows with
    tri = -1 and tri = F mixed in (except the single point) and roughness texels at or below 0.02 next to ones above it."""
    H, W, B, stretched = BACKWARD_CASES[case]
    rng = np.random.default_rng(30 + H + B % 97)
    texels = rng.uniform(0.0, 1.0, (H, W, 5)).astype(np.float32)
    texels[..., 3] = np.where(rng.random((H, W)) < 0.5, rng.uniform(-0.2, 0.02, (H, W)), texels[..., 3]).astype(np.float32)
    if H * W == 1:
        texels[0, 0, 3] = 0.5
    tri = rng.integers(-1, 3, B) if B > 1 else np.array([1])
    bary = folded(rng, B)
    vt = QUAD_VT * 3 - 1 if stretched else QUAD_VT
    g = rng.normal(size=(B, 5)).astype(np.float32)
    got = raw_backward(tri, bary, QUAD_F, vt, texels, g)
    ref, n, S = TF.gradient(tri, bary, QUAD_F, vt, texels, g[:, :3], g[:, 3], g[:, 4])
    err, bound = np.abs(got.astype(np.float64) - ref), (n + 4) * U * S
    worst = float((err / np.where(bound > 0, bound, 1)).max())
    print(f"{case}: largest error {worst:.3g} of the bound; most contributions to one texel channel {int(n.max())}; {int((n == 0).sum())} untouched")
    assert (got[n == 0] == 0).all()
    assert (err <= bound).all(), worst
    assert n.sum() > 0 and (B == 1 or H * W == 1 or (n[..., 3] < n[..., 0]).any())          # (some roughness rows were blocked)
    if stretched:
        assert n[0, 0, 0] > n[H // 2, W // 2, 0]                                             # the clamp piles a ninth of the points onto each corner


def test_backward_adds_and_refuses():
    """the call ADDS into g_texels (twice the gradient after two calls); B = 0 launches nothing; H or W above 8192 and g_texels == texels are refused"""
    from iris_amd import _lib as L
    rng = np.random.default_rng(5)
    texels = rng.uniform(0.1, 0.9, (5, 7, 5)).astype(np.float32)
    tri, bary, g = rng.integers(0, 2, 33), folded(rng, 33), rng.normal(size=(33, 5)).astype(np.float32)
    ref, n, S = TF.gradient(tri, bary, QUAD_F, QUAD_VT, texels, g[:, :3], g[:, 3], g[:, 4])
    acc = torch.zeros(5, 7, 5, device=DEV)
    raw_backward(tri, bary, QUAD_F, QUAD_VT, texels, g, into=acc)
    twice = raw_backward(tri, bary, QUAD_F, QUAD_VT, texels, g, into=acc)
    assert (np.abs(twice - 2 * ref) <= (2 * n + 4) * U * 2 * S).all()
    assert (raw_backward(tri[:0], bary[:0], QUAD_F, QUAD_VT, texels, g[:0]) == 0).all() and raw_forward(tri[:0], bary[:0], QUAD_F, QUAD_VT, texels).shape == (0, 5)
    t, z = dev(texels), torch.zeros(4, device=DEV)
    args = (L.ptr(dev(tri)), L.ptr(dev(bary)), 0, L.ptr(dev(QUAD_F)), 2, L.ptr(dev(QUAD_VT)), 4, L.ptr(t))
    assert L.lib().iris_texture_sample_f32(*args, 8193, 7, L.ptr(z), L.ptr(z), L.ptr(z), L.stream()) != 0
    assert L.lib().iris_texture_sample_f32_bwd(*args, 5, 0, L.ptr(z), L.ptr(z), L.ptr(z), L.ptr(acc), L.stream()) != 0
    assert L.lib().iris_texture_sample_f32_bwd(*args, 5, 7, L.ptr(z), L.ptr(z), L.ptr(z), L.ptr(t), L.stream()) != 0
    assert b"g_texels" in L.lib().iris_last_error()


# ------------------------------------------------------------------------------------------------------------------------------ 4. autograd
def test_autograd_through_the_material():
    """sample(...).backward() fills texels.grad with the raw call's result (both within the derived bound of the float64 restatement: the sums are float
    atomics), a second backward accumulates, forward(position) equals sample(*closest_point(scene, position)[:2]) in value (bit for bit) and in gradient, and a
    position or bary that requires grad raises; FusedAdam steps the parameter"""
    from iris_amd import _lib as L
    from iris_amd.model.texture import TextureBRDF
    from iris_amd.utils.closest import closest_point
    from iris_amd.utils.optim import FusedAdam
    rng = np.random.default_rng(40)
    H, W, B = 5, 7, 513
    albedo, rm = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rm[:2, :, 0] = 3                                                                  # a band below the floor
    net = TextureBRDF(quad_scene(), QUAD_F, QUAD_VT, albedo, rm)
    assert [k for k, _ in net.named_parameters()] == ["texels"] and net.texels.is_contiguous() and net.texels.dtype == torch.float32 and net.texels.is_cuda
    texels = net.texels.detach().cpu().numpy()
    tri, bary, g = rng.integers(0, 2, B), folded(rng, B), rng.normal(size=(B, 5)).astype(np.float32)
    ref, n, S = TF.gradient(tri, bary, QUAD_F, QUAD_VT, texels, g[:, :3], g[:, 3], g[:, 4])
    bound = (n + 4) * U * S
    raw = raw_backward(tri, bary, QUAD_F, QUAD_VT, texels, g)

    def loss(out):
        return (torch.cat([out[k] for k in KEYS], 1) * dev(g)).sum()
    loss(net.sample(dev(tri), dev(bary))).backward()
    grad = net.texels.grad.cpu().numpy()
    assert (np.abs(grad - ref) <= bound).all() and (np.abs(raw - ref) <= bound).all() and (grad[n == 0] == 0).all()
    loss(net.sample(dev(tri), dev(bary))).backward()
    assert (np.abs(net.texels.grad.cpu().numpy() - 2 * ref) <= 2 * bound + U * np.abs(2 * ref)).all()
    # through positions: above and below the quad
    pos = dev(np.concatenate([rng.random((B, 2)), rng.uniform(-0.3, 0.3, (B, 1))], 1).astype(np.float32))
    t2, b2, _, _ = closest_point(quad_scene(), pos)
    one, two = net(pos), net.sample(t2, b2)
    for k in KEYS:
        assert torch.equal(one[k], two[k]) and one[k].shape == two[k].shape
    assert net(pos[:12].reshape(3, 4, 3))["albedo"].shape == (3, 4, 3)
    ref2, n2, S2 = TF.gradient(t2.cpu().numpy(), b2.cpu().numpy(), QUAD_F, QUAD_VT, texels, g[:, :3], g[:, 3], g[:, 4])
    for out in (one, two):
        net.texels.grad = None
        loss(out).backward()
        assert (np.abs(net.texels.grad.cpu().numpy() - ref2) <= (n2 + 4) * U * S2).all()
    with pytest.raises(L.IrisError, match="requires grad"):
        net(pos.clone().requires_grad_())
    with pytest.raises(L.IrisError, match="requires grad"):
        net.sample(t2, b2.clone().requires_grad_())
    with torch.no_grad():
        assert not net.sample(t2, b2)["albedo"].requires_grad
    before = net.texels.detach().clone()
    FusedAdam([net.texels], lr=1e-2).step()
    moved = (net.texels.detach() - before).abs()
    touched = torch.from_numpy(n2 > 0).to(DEV)                                        # Adam's first step is lr * g / (|g| + eps): nearly lr wherever g is not tiny
    assert 0.9e-2 <= float(moved.max()) <= 1.001e-2 and float(moved[touched].median()) > 0.9e-2 and float((moved * ~touched).max()) == 0


# ------------------------------------------------------------------------------------------------------------------------------ 5. the fit
class WaveMaterial(torch.nn.Module):
    """tests/texfit_ref.py's wave() as material_net(position), float32 on the position's device"""

    def forward(self, x):
        x = x.reshape(-1, 3)
        ph = torch.tensor(TF.WAVE_PHASE, device=x.device, dtype=torch.float32)
        m = 0.5 + 0.35 * torch.sin(2 * np.pi * 4 * x[:, :1] + ph) * torch.cos(2 * np.pi * 4 * x[:, 1:2])
        return {"albedo": m[:, :3].contiguous(), "roughness": m[:, 3:4].contiguous(), "metallic": m[:, 4:5].contiguous()}


def wave_material(voxel_min=None, voxel_max=None, ckpt=None):
    """--material test_texture_fit:wave_material"""
    return WaveMaterial()


def test_fit_against_the_restatement():
    """The identity quad at 16 x 16, the wave material baked with bake_textures; the device fit and the float64 restatement start from those bytes and see the same
    200 recorded draws of 1024 uniform points, lr 1e-2; both are rounded to 8 bits and scored on 20 000 held-out points by the restatement's float64 fetch.
    The device's held-out MSE must lie below the geometric mean of the initial MSE and the restatement's final one (the bound comes from the reference at run
    time), and its last loss within 5 % of the restatement's (same draws, float32 against float64: the 5 % only has to catch a wrong step)."""
    from iris_amd.model.texture import TextureBRDF
    from iris_amd.utils.texture import bake_textures, fit_textures
    net = WaveMaterial()
    albedo, rm = bake_textures(net, QUAD_VT, QUAD_F, QUAD_V, QUAD_F, 16, device=torch.device(DEV))
    bytes5 = np.concatenate([albedo.cpu().numpy(), rm.cpu().numpy()[..., :2]], -1)
    texels0 = bytes5.astype(np.float32) / np.float32(255)
    rng = np.random.default_rng(0)
    draws = [TF.quad_draw(rng, 1024) for _ in range(200)]
    face, bary, pos = TF.quad_draw(np.random.default_rng(1), 20000)
    want = TF.wave(pos[:, 0], pos[:, 1])
    before = TF.held_out_mse(texels0, face, bary, want)
    fitted, ref_losses = TF.fit(texels0, QUAD_F, QUAD_VT, [d[:2] for d in draws], [TF.wave(d[2][:, 0], d[2][:, 1]) for d in draws], 1e-2)
    ref_after = TF.held_out_mse(TF.quantize(fitted).astype(np.float64) / 255.0, face, bary, want)
    on_device = [(dev(d[0]), dev(d[1])) for d in draws]
    tex = TextureBRDF(quad_scene(), QUAD_F, QUAD_VT, albedo, rm)
    report = fit_textures(net, tex, QUAD_V, QUAD_F, 200, 1024, 1e-2, draw=lambda step: on_device[step])
    a, r = tex.to_images()
    got = np.concatenate([a.cpu().numpy(), r.cpu().numpy()[..., :2]], -1)
    after = TF.held_out_mse(got.astype(np.float64) / 255.0, face, bary, want)
    bound = float(np.sqrt(before * ref_after))
    print(f"held-out MSE: baked {before:.4g}, the restatement's fit {ref_after:.4g}, the device's fit {after:.4g} (bound {bound:.4g}); last loss: device "
          f"{report['last_loss']:.6g}, restatement {ref_losses[-1]:.6g} (relative difference {abs(report['last_loss'] / ref_losses[-1] - 1):.3g}); first loss: device "
          f"{report['first_loss']:.6g}, restatement {ref_losses[0]:.6g}; bytes that differ from the restatement's: {int((got != TF.quantize(fitted)).sum())} of {got.size}")
    assert ref_after < before and after < bound
    assert abs(report["last_loss"] - ref_losses[-1]) <= 0.05 * ref_losses[-1]
    assert report["steps"] == 200 and abs(report["first_loss"] - ref_losses[0]) <= 0.05 * ref_losses[0]
    # the default draw: area-proportional faces, barycentrics inside the triangle, a function of (seed, step) alone
    from iris_amd.utils.texture import surface_draw
    v3 = np.float32([[0, 0, 0], [3, 0, 0], [0, 2, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [5, 5, 5], [5, 5, 5]])
    f3 = np.arange(9, dtype=np.int32).reshape(3, 3)                                  # areas 3, 0.5 and 0
    draw = surface_draw(v3, f3, 20000, 7, torch.device(DEV))
    f_a, b_a = draw(3)
    f_b, b_b = draw(3)
    assert torch.equal(f_a, f_b) and torch.equal(b_a, b_b) and not torch.equal(f_a, draw(4)[0]) and f_a.dtype == torch.int64 and b_a.dtype == torch.float32
    share = float((f_a == 0).float().mean())
    assert abs(share - 6 / 7) < 5 * np.sqrt(6 / 7 * 1 / 7 / 20000) and int(f_a.max()) == 1           # five standard deviations; the face without area is never drawn
    assert float(b_a.min()) >= 0 and float(b_a.sum(1).max()) <= 1 and 0.3 < float(b_a.mean()) < 0.37


# ------------------------------------------------------------------------------------------------------------------------------ 6. the command line
def test_export_command_line_with_the_fit(tmp_path):
    """python -m iris_amd.utils.export on the quad with the wave material at 16 x 16, as subprocesses: --fit_steps 0 writes the bytes of the command without the
    option; --fit_steps 50 --verify 2000 exits 0, prints the PSNR line twice with albedo not lower after the fit, and writes files that from_export loads
    and that are a fixed point of to_images().  Against the same fit run here the files differ by at most one 8-bit code (the gradient's float atomics make
    a fit reproducible to rounding, not bit for bit)."""
    from PIL import Image
    from iris_amd.model.texture import BakedTextureBRDF, TextureBRDF
    from iris_amd.utils.texture import bake_textures, fit_textures
    with open(tmp_path / "quad.obj", "w") as fh:
        fh.writelines("v {:.9g} {:.9g} {:.9g}\n".format(*p) for p in QUAD_V.tolist())
        fh.writelines("f {} {} {}\n".format(*(i + 1 for i in t)) for t in QUAD_F.tolist())
    torch.save({"voxel_min": -1.0, "voxel_max": 2.0}, tmp_path / "vslf.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, "tests")]))

    def run(name, *extra):
        out = tmp_path / name
        out.mkdir()
        np.save(out / "ft.npy", QUAD_F)
        np.save(out / "vt.npy", QUAD_VT)
        p = subprocess.run([sys.executable, "-m", "iris_amd.utils.export", "--mesh", str(tmp_path / "quad.obj"), "--emitter_path", str(tmp_path), "--dir_save", str(out),
                            "--tex_res", "16", "--atlas", "files", "--material", "test_texture_fit:wave_material", "--device", DEV] + list(extra), env=env,
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        print(p.stdout, p.stderr)
        assert p.returncode == 0, name
        return out, p.stdout
    plain, _ = run("plain")
    zero, text = run("zero", "--fit_steps", "0")
    for name in ("albedo.png", "rm.png", "ft.npy", "vt.npy"):
        assert (plain / name).read_bytes() == (zero / name).read_bytes(), name
    assert "[INFO] fit" not in text
    fit, text = run("fit", "--fit_steps", "50", "--fit_points", "4096", "--fit_lr", "1e-2", "--verify", "2000")
    lines = [l for l in text.splitlines() if l.startswith("[INFO] verify:")]
    assert len(lines) == 2 and len([l for l in text.splitlines() if l.startswith("[INFO] fit: 50 steps")]) == 1
    psnr = [float(l.split("PSNR albedo ")[1].split(" dB")[0]) for l in lines]
    assert psnr[1] >= psnr[0], psnr
    assert (fit / "albedo.png").read_bytes() != (plain / "albedo.png").read_bytes()
    images = [np.array(Image.open(fit / n)) for n in ("albedo.png", "rm.png")]
    baked = BakedTextureBRDF.from_export(str(fit), QUAD_V, QUAD_F, torch.device(DEV))
    assert np.array_equal(baked.tex.albedo.cpu().numpy(), images[0]) and np.array_equal(baked.tex.rm.cpu().numpy(), images[1])
    again = TextureBRDF.from_export(str(fit), QUAD_V, QUAD_F, torch.device(DEV)).to_images()
    assert np.array_equal(again[0].cpu().numpy(), images[0]) and np.array_equal(again[1].cpu().numpy(), images[1]) and int(images[1][..., 2].max()) == 0
    net = WaveMaterial()
    albedo, rm = bake_textures(net, QUAD_VT, QUAD_F, QUAD_V, QUAD_F, 16, device=torch.device(DEV))
    assert np.array_equal(albedo.cpu().numpy(), np.array(Image.open(plain / "albedo.png")))
    tex = TextureBRDF(quad_scene(), QUAD_F, QUAD_VT, albedo, rm)
    fit_textures(net, tex, QUAD_V, QUAD_F, 50, 4096, 1e-2, seed=0)
    here = tex.to_images()
    for mine, theirs in zip(here, images):
        d = np.abs(mine.cpu().numpy().astype(np.int32) - theirs.astype(np.int32))
        print(f"bytes that differ from the fit run here: {int((d > 0).sum())} of {d.size}")
        assert d.max() <= 1
