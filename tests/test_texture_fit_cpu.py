"""The trainable texture on the CPU: the restatement tests/texfit_ref.py against central differences and on the fit it has to win,
to_images' rounding rule on hand values, the export command line's three option tables, and what is refused before a device is touched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import texfit_ref as TF


def test_restated_gradient_against_central_differences():
    """3 x 4 texels in float64, 40 points on the identity quad with its UVs stretched to [-1, 2] (clamped taps, merged border taps), rows without a triangle
    mixed in, roughness taps well above and well below the floor: d sum(out * g) / d texel by central differences, h = 1e-4, against gradient(gate='float64').
    The fetch is linear in the texels away from the floor, so the difference quotient is exact up to the rounding of the two values: each is a float64 sum of
    N = 5 B products, off by at most N 2^-53 sum |out g|, and the two errors are divided by 2 h (about 2e-8 here; a wrong weight or tap is off by 0.01 and more)."""
    rng = np.random.default_rng(3)
    H, W, B = 3, 4, 40
    texels = rng.uniform(-0.5, 1.5, (H, W, 5))
    texels[:, :2, 3] = rng.uniform(-0.4, -0.1, (H, 2))              # roughness below the floor on the left half, above it on the right
    texels[:, 2:, 3] = rng.uniform(0.3, 0.9, (H, 2))
    vt = TF.QUAD_VT * 3 - 1
    tri = rng.integers(0, 2, B)
    tri[[5, 17]] = -1
    tri[9] = 2
    bary = rng.random((B, 2)).astype(np.float32)
    bary = np.where(bary.sum(1, keepdims=True) > 1, np.float32(1) - bary, bary).astype(np.float32)
    g = rng.normal(size=(B, 5))

    def value(t):
        out, _ = TF.fetch64(tri, bary, TF.QUAD_F, vt, t)
        return float((out * g).sum())
    grad, n, S = TF.gradient(tri, bary, TF.QUAD_F, vt, texels, g[:, :3], g[:, 3], g[:, 4], gate="float64")
    out, _ = TF.fetch64(tri, bary, TF.QUAD_F, vt, texels)
    h, worst = 1e-4, 0.0
    bound = 2 * (5 * B) * 2.0 ** -53 * float(np.abs(out * g).sum() + 5 * B * h * np.abs(g).max()) / (2 * h)
    for idx in np.ndindex(H, W, 5):
        up, down = texels.copy(), texels.copy()
        up[idx] += h
        down[idx] -= h
        worst = max(worst, abs((value(up) - value(down)) / (2 * h) - grad[idx]))
    print(f"largest difference from central differences {worst:.3g} (allowed {bound:.3g})")
    assert worst <= bound
    assert n[..., 0].sum() == 4 * (B - 3) and (n[..., 3] < n[..., 0]).any() and n[..., 3].sum() > 0          # some roughness rows are blocked, some pass
    assert (S >= np.abs(grad) - 1e-12).all() and ((n == 0) == (S == 0)).all()
    # the float32 gate agrees with the float64 one away from the floor, and the float32 fetch with the float64 fetch
    grad32, _, _ = TF.gradient(tri, bary, TF.QUAD_F, vt, texels.astype(np.float32), g[:, :3], g[:, 3], g[:, 4])
    assert np.abs(grad32 - grad).max() <= 1e-12
    f32, (f64, _) = TF.fetch(tri, bary, TF.QUAD_F, vt, texels.astype(np.float32)), TF.fetch64(tri, bary, TF.QUAD_F, vt, texels.astype(np.float32))
    got = np.concatenate([f32["albedo"], f32["roughness"], f32["metallic"]], 1)
    assert got.dtype == np.float32 and np.abs(got - f64).max() <= 16 * 2.0 ** -24 * 2.0          # nine roundings at magnitudes below 2, and slack
    assert (got[[5, 9, 17]] == np.float32([0, 0, 0, 0.02, 0])).all()


def test_to_images_rounds_to_nearest():
    """floor(clamp(x, 0, 1) * 255 + 0.5) in float32 on values either side of k + 0.5 codes, and NaN, -1, 2, +-inf"""
    from iris_amd.model.texture import quantize_texels
    f = np.float32
    cases = [(0.0, 0), (1.0, 255), (-1.0, 0), (2.0, 255), (float("nan"), 0), (float("inf"), 255), (float("-inf"), 0), (0.5 / 255, 1), (0.49 / 255, 0), (0.51 / 255, 1),
             (100.49 / 255, 100), (100.51 / 255, 101), (254.49 / 255, 254), (254.51 / 255, 255), (0.4567, 116), (0.8, 204), (0.02, 5)]
    assert int(np.float32(0.4567) * 255) == 116 and int(np.float32(0.02) * 255) == 5
    vals = np.array([c[0] for c in cases], f)
    texels = np.zeros((1, len(cases), 5), f)
    for ch in range(5):
        texels[0, :, ch] = np.roll(vals, ch)
    albedo, rm = quantize_texels(torch.from_numpy(texels))
    assert albedo.dtype == torch.uint8 and rm.dtype == torch.uint8 and tuple(albedo.shape) == (1, len(cases), 3) and tuple(rm.shape) == (1, len(cases), 3)
    want = np.array([c[1] for c in cases], np.uint8)
    for ch in range(3):
        assert albedo[0, :, ch].tolist() == np.roll(want, ch).tolist(), ch
    assert rm[0, :, 0].tolist() == np.roll(want, 3).tolist() and rm[0, :, 1].tolist() == np.roll(want, 4).tolist() and int(rm[..., 2].max()) == 0
    assert np.array_equal(TF.quantize(texels)[..., :3], albedo.numpy()) and np.array_equal(TF.quantize(texels)[..., 3:], rm.numpy()[..., :2])
    # a byte / 255 comes back as the byte: the round trip of an unfitted texture is the identity
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(TF.quantize(b.astype(f) / f(255)), b)


def test_the_three_export_parsers():
    """build_parser() and build_parser(area_atlas=True) keep the tables that tests/test_stage_setup_cpu.py and tests/test_atlas_cpu.py pin; the parser main() runs
    is the second plus --verify and the four options of the fit"""
    from iris_amd.utils import export as E
    from test_stage_setup_cpu import PARSERS, _table
    area = dict(PARSERS["export"], atlas=(("--atlas",), str, "auto", ("auto", "files", "grid", "area"), False, None), dilate=(("--dilate",), int, 0, None, False, None))
    full = dict(area, verify=(("--verify",), int, 0, None, False, None), fit_steps=(("--fit_steps",), int, 0, None, False, None),
                fit_points=(("--fit_points",), int, 262144, None, False, None), fit_lr=(("--fit_lr",), float, 5e-3, None, False, None),
                fit_seed=(("--fit_seed",), int, 0, None, False, None))
    assert _table(E.build_parser()) == PARSERS["export"]
    assert _table(E.build_parser(area_atlas=True)) == area
    assert _table(E.build_parser(area_atlas=True, verify=True)) == dict(area, verify=full["verify"])
    assert _table(E.build_parser(area_atlas=True, verify=True, fit=True)) == full
    with pytest.raises(SystemExit):
        E.build_parser(area_atlas=True, verify=True).parse_args(["--fit_steps", "5"])


def test_refusals_come_before_the_device(tmp_path):
    """(no device here: an IrisError that is not 'needs a GPU' came from the host checks)"""
    from iris_amd._lib import IrisError
    from iris_amd.model.texture import TextureBRDF
    from iris_amd.utils import export as E, texture as T
    assert T.check_fit_options(0, 1, 1e-9) == (0, 1, 1e-9) and T.check_fit_options(np.int64(3), 7, 1) == (3, 7, 1.0)
    for bad in ((-1, 10, 1e-2), (1.5, 10, 1e-2), (True, 10, 1e-2), (5, 0, 1e-2), (5, -3, 1e-2), (5, 2.0, 1e-2), (5, 10, 0.0), (5, 10, -1e-3), (5, 10, float("nan")),
                (5, 10, float("inf")), (5, 10, "1e-2")):
        with pytest.raises(IrisError, match="fit_textures"):
            T.check_fit_options(*bad)
    missing = str(tmp_path / "nothing_here.obj")                    # main() would fail on this file next: the options are refused first
    base = ["--mesh", missing, "--emitter_path", str(tmp_path), "--dir_save", str(tmp_path / "out")]
    for extra, word in ((["--fit_steps", "-1"], "steps"), (["--fit_steps", "3", "--fit_points", "0"], "points"), (["--fit_steps", "3", "--fit_lr", "0"], "lr"),
                        (["--fit_lr", "-1"], "lr")):
        with pytest.raises(IrisError, match=word):
            E.main(base + extra)
    assert not (tmp_path / "out").exists()
    # the material's host checks are BakedTextureBRDF's, and run before the scene's device is asked for anything
    scene = SimpleNamespace(device="cuda", n_triangles=2)
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(IrisError, match="differ in size"):
        TextureBRDF(scene, TF.QUAD_F, TF.QUAD_VT, img, np.zeros((4, 5, 3), np.uint8))
    with pytest.raises(IrisError, match="8-bit RGB"):
        TextureBRDF(scene, TF.QUAD_F, TF.QUAD_VT, img.astype(np.float32), img)
    with pytest.raises(IrisError, match="the mesh has 2 faces"):
        TextureBRDF(scene, TF.QUAD_F[:1], TF.QUAD_VT, img, img)
    with pytest.raises(IrisError, match="outside the 3 UV vertices"):
        TextureBRDF(scene, TF.QUAD_F, TF.QUAD_VT[:3], img, img)
    with pytest.raises(IrisError, match="requires grad"):
        TextureBRDF(scene, TF.QUAD_F, torch.from_numpy(TF.QUAD_VT).requires_grad_(True), img, img)
    with pytest.raises(IrisError, match="not found"):
        TextureBRDF.from_export(str(tmp_path), TF.QUAD_V, TF.QUAD_F)


def test_restated_fit_wins_back_what_the_bake_loses():
    """The issue's case: 16 x 16 texels on the identity quad, the material 0.5 + 0.35 sin(2 pi 4 x + phase) cos(2 pi 4 y) (wavelength 4 texels), initial texels =
    the material at texel centres truncated to 8 bits, Adam at lr 1e-2 on 1024 uniform points per step for 200 steps, the result rounded to 8 bits, scored on
    20 000 held-out points: the restatement's own fit must bring the mean squared error below the geometric mean of the initial one and 1.5e-3 (the figure of
    a float64 run of the same case)."""
    H = W = 16
    cx, cy = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
    baked = np.floor(TF.wave(cx.ravel(), cy.ravel()).astype(np.float32) * np.float32(255)).astype(np.uint8).reshape(H, W, 5)
    texels0 = baked.astype(np.float32) / np.float32(255)
    rng = np.random.default_rng(0)
    draws, targets = [], []
    for _ in range(200):
        face, bary, pos = TF.quad_draw(rng, 1024)
        draws.append((face, bary))
        targets.append(TF.wave(pos[:, 0], pos[:, 1]))
    face, bary, pos = TF.quad_draw(np.random.default_rng(1), 20000)
    want = TF.wave(pos[:, 0], pos[:, 1])
    before = TF.held_out_mse(texels0, face, bary, want)
    fitted, losses = TF.fit(texels0, TF.QUAD_F, TF.QUAD_VT, draws, targets, 1e-2)
    after = TF.held_out_mse(TF.quantize(fitted).astype(np.float64) / 255.0, face, bary, want)
    print(f"held-out MSE {before:.4g} -> {after:.4g} ({-10 * np.log10(before):.1f} -> {-10 * np.log10(after):.1f} dB), loss {losses[0]:.4g} -> {losses[-1]:.4g}")
    assert after < np.sqrt(before * 1.5e-3)
    assert losses[-1] < losses[0]
