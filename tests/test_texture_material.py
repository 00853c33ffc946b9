"""The exported textures read back on the GPU (iris_amd/csrc/iris_texmat.h, iris_amd/model/texture.py): the fetch against its numpy restatement
(tests/texmat_ref.py) and against analytic values on a hand-made atlas, the one-launch material against the two-call composition, and the whole way round --
export a constant material, read it back exactly, render with it bit for bit as with the constants, run the command line."""
import functools
import json

import numpy as np
import pytest
import torch

import texmat_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FETCH_BOUND = 8 * 2.0 ** -24          # the values are at most 1 and the lerps three deep: derived, not measured

QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
QUAD_VT = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_fetch_on_a_hand_made_atlas():
    """one quad of two faces over the whole UV square, a 5-row x 7-column texture with the column in one channel and the row in another: at interior points the
    bilinear value is the linear function of the position, so a flipped v, a half-texel shift, swapped channels or a swapped H / W all show"""
    from iris_amd.model.texture import BakedTextureBRDF, sample_textures
    from iris_amd.utils.closest import closest_point
    from iris_amd.utils.path_tracing import Scene
    H, W = 5, 7
    albedo = np.zeros((H, W, 3), np.uint8)
    albedo[..., 0] = np.arange(W)[None, :] * 30
    albedo[..., 1] = np.arange(H)[:, None] * 50
    albedo[..., 2] = 200
    rm = np.zeros((H, W, 3), np.uint8)
    rm[..., 0] = np.arange(W)[None, :] * 20 + 30
    rm[..., 1] = np.arange(H)[:, None] * 40
    rm[..., 2] = 255                                                   # never read
    scene = Scene(QUAD_V, QUAD_F, device=torch.device(DEV))
    net = BakedTextureBRDF(scene, QUAD_F, QUAD_VT, albedo, rm)
    rng = np.random.default_rng(1)
    uv = np.stack([rng.uniform(0.5 / W, 1 - 0.5 / W, 4097), rng.uniform(0.5 / H, 1 - 0.5 / H, 4097)], 1)
    x = dev(np.concatenate([uv, rng.uniform(-0.5, 0.5, (4097, 1))], 1).astype(np.float32))              # above and below the quad
    out = net(x)
    xs, ys = x[:, 0].double().cpu().numpy() * W - 0.5, x[:, 1].double().cpu().numpy() * H - 0.5
    want = {"albedo": np.stack([xs * 30, ys * 50, np.full_like(xs, 200)], 1) / 255, "roughness": (xs * 20 + 30)[:, None] / 255, "metallic": (ys * 40)[:, None] / 255}
    for k, w in want.items():
        assert out[k].shape == w.shape and out[k].dtype == torch.float32
        assert np.abs(out[k].double().cpu().numpy() - w).max() <= 2e-6, k           # (x = u W - 0.5 in float32: 7 x 2^-24 x the slope of 30 / 255)
    # the same through the two calls, and through the restatement
    tri, bary, _, _ = closest_point(scene, x)
    two = sample_textures(tri, bary, QUAD_F, QUAD_VT, albedo, rm)
    ref = TR.fetch(tri.cpu().numpy(), bary.cpu().numpy(), QUAD_F, QUAD_VT, albedo, rm)
    for k in want:
        assert torch.equal(out[k].view(torch.int32), two[k].view(torch.int32)), k
        assert np.abs(two[k].double().cpu().numpy() - ref[k]).max() <= FETCH_BOUND, k
    # beyond the border texels' centres the value is the border's: u = 0 and u = 1, v = 0 and v = 1 (the quad's corners)
    corners = net(dev(QUAD_V))
    assert np.allclose(corners["albedo"].cpu().numpy() * 255, [[0, 0, 200], [180, 0, 200], [180, 200, 200], [0, 200, 200]], atol=1e-4)
    # a batch shape is kept; tri = -1 gives zeros and the floor
    assert net(x[:12].reshape(3, 4, 3))["roughness"].shape == (3, 4, 1)
    none = net.sample(torch.tensor([-1, 0, 5], device=DEV), torch.zeros(3, 2, device=DEV))
    assert none["albedo"][[0, 2]].abs().max() == 0 and none["metallic"][[0, 2]].abs().max() == 0 and bool((none["roughness"][[0, 2]] == np.float32(0.02)).all())
    assert none["albedo"][1].abs().max() > 0
    nan = net(torch.full((3, 3), float("nan"), device=DEV))
    assert nan["albedo"].abs().max() == 0 and bool((nan["roughness"] == np.float32(0.02)).all())
    assert net(torch.zeros(0, 3, device=DEV))["albedo"].shape == (0, 3)


@functools.lru_cache(maxsize=None)
def ico():
    from iris_amd.utils.lights import icosphere
    from iris_amd.utils.path_tracing import Scene
    v, f = icosphere(3)
    v, f = v.astype(np.float32), np.asarray(f, np.int32)
    return v, f, Scene(v, f, device=torch.device(DEV))


def surface_points(v, f, n, seed):
    rng = np.random.default_rng(seed)
    face = rng.integers(0, len(f), n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    p0, p1, p2 = (v[f[face, k]].astype(np.float64) for k in range(3))
    return ((1 - b.sum(1, keepdims=True)) * p0 + b[:, :1] * p1 + b[:, 1:] * p2).astype(np.float32)


def test_fetch_against_the_restatement_and_the_composition():
    """random 48 x 64 images on the icosphere's grid atlas, 4097 points inside the box and 4097 on the surface: sample_textures at the device's own (tri, bary)
    within 8 * 2^-24 of tests/texmat_ref.py, BakedTextureBRDF.forward bit-equal to the two calls; a zero roughness image returns exactly 0.02"""
    from iris_amd import _lib as L
    from iris_amd.model.texture import BakedTextureBRDF, sample_textures
    from iris_amd.utils.closest import closest_point
    from iris_amd.utils.texture import grid_atlas
    v, f, scene = ico()
    H, W = 48, 64
    vt, ft = grid_atlas(len(f), (H, W))
    rng = np.random.default_rng(2)
    albedo, rm = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    net = BakedTextureBRDF(scene, ft, vt, albedo, rm)
    x = dev(np.concatenate([rng.uniform(-1, 1, (4097, 3)).astype(np.float32), surface_points(v, f, 4097, 3)]))
    tri, bary, _, _ = closest_point(scene, x)
    two = sample_textures(tri, bary, ft, vt, albedo, rm)
    one = net(x)
    ref = TR.fetch(tri.cpu().numpy(), bary.cpu().numpy(), ft, vt, albedo, rm)
    for k in ("albedo", "roughness", "metallic"):
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k
        err = np.abs(two[k].double().cpu().numpy() - ref[k]).max()
        print(f"{k}: largest deviation from the restatement {err / 2.0 ** -24:.3g} x 2^-24 (allowed 8)")
        assert err <= FETCH_BOUND, k
    assert float(one["roughness"].min()) >= float(np.float32(0.02)) and float(one["albedo"].std()) > 0.05
    floor = BakedTextureBRDF(scene, ft, vt, albedo, np.zeros_like(rm))(x)
    assert bool((floor["roughness"] == np.float32(0.02)).all()) and float(floor["metallic"].abs().max()) == 0
    with pytest.raises(L.IrisError, match="requires grad"):
        net(torch.rand(4, 3, device=DEV, requires_grad=True))
    with pytest.raises(L.IrisError, match="requires grad"):
        sample_textures(tri[:4], bary[:4].clone().requires_grad_(True), ft, vt, albedo, rm)
    with pytest.raises(L.IrisError):
        net(torch.rand(4, 3))
    with pytest.raises(L.IrisError, match="the mesh has 1280 faces"):
        BakedTextureBRDF(scene, ft[:5], vt, albedo, rm)


# ---- the whole way round: a constant material, exported and read back
CONST = {"albedo": (0.8, 0.35, 0.123), "roughness": 0.4567, "metallic": 0.77}


class ConstMaterial(torch.nn.Module):
    def __init__(self, albedo, roughness, metallic):
        super().__init__()
        self.values = (torch.tensor(albedo, dtype=torch.float32), torch.tensor([roughness], dtype=torch.float32), torch.tensor([metallic], dtype=torch.float32))

    def forward(self, x):
        n = x.reshape(-1, 3).shape[0]
        a, r, m = (t.to(x.device) for t in self.values)
        return {"albedo": a.expand(n, 3).contiguous(), "roughness": r.expand(n, 1).contiguous(), "metallic": m.expand(n, 1).contiguous()}


def const_material(voxel_min=None, voxel_max=None, ckpt=None):
    """--material test_texture_material:const_material"""
    return ConstMaterial(CONST["albedo"], CONST["roughness"], CONST["metallic"])


def dequantised():
    q = lambda c: float(np.float32(int(np.float32(c) * np.float32(255.0))) / np.float32(255.0))           # trunc(c * 255) / 255 in float32, as the export and the fetch
    return ConstMaterial([q(c) for c in CONST["albedo"]], q(CONST["roughness"]), q(CONST["metallic"]))


def write_room(folder):
    """the icosphere as a scene on disk, seen from inside: scene.obj, the emitter files (eight of its faces shine), a checkpoint with a response model, one
    32 x 24 camera.  (The scene-on-disk pattern of tests/test_render.py, for a mesh made here.)"""
    from iris_amd.model.crf import EmorCRF
    from iris_amd.model.slf import VoxelSLF
    v, f, _ = ico()
    data, bake, ckpt_dir = folder / "data", folder / "bake", folder / "ckpt" / "exp"
    for d in (data, bake, ckpt_dir):
        d.mkdir(parents=True)
    with open(data / "scene.obj", "w") as fh:
        fh.writelines("v {:.9g} {:.9g} {:.9g}\n".format(*p) for p in v.tolist())
        fh.writelines("f {} {} {}\n".format(*(i + 1 for i in t)) for t in f.tolist())
    is_emitter = torch.zeros(len(f), dtype=torch.bool)
    is_emitter[:8] = True
    ev = torch.from_numpy(v[f[:8]])
    area = 0.5 * torch.linalg.cross(ev[:, 1] - ev[:, 0], ev[:, 2] - ev[:, 0]).norm(dim=-1)
    torch.save({"is_emitter": is_emitter, "emitter_vertices": ev, "emitter_area": area, "emitter_normal": torch.zeros(8, 3),
                "emitter_radiance": torch.full((8, 3), 6.0)}, bake / "emitter.pth")
    mask = torch.ones(4, 4, 4, dtype=torch.bool)
    slf = VoxelSLF(mask, -1.05, 1.05)
    slf.radiance[:] = torch.rand(64, 3, generator=torch.Generator().manual_seed(4)) * 0.5
    for name in ("vslf.npz", "vslf_0.npz"):
        torch.save({"mask": mask, "voxel_min": -1.05, "voxel_max": 1.05, "weight": slf.state_dict()}, bake / name)
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (k + 1)) * 0.05 for k in range(3)]))
    torch.save({"state_dict": {"model_crf." + k: t for k, t in crf.state_dict().items()}}, ckpt_dir / "last.ckpt")
    K = [[30.0, 0.0, 16.0], [0.0, 30.0, 12.0], [0.0, 0.0, 1.0]]
    c2w = [[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, 0.05], [0.0, 0.0, 1.0, -0.1]]
    with open(data / "cameras.json", "w") as fh:
        json.dump({"img_hw": [24, 32], "views": [{"K": K, "c2w": c2w}]}, fh)
    return data, bake, crf, np.float32(K), np.float32(c2w)


def test_constant_material_round_trip(tmp_path, capsys):
    """python -m iris_amd.utils.export --atlas area --tex_res 256 --dilate 2 --verify 4097 of a constant material on the icosphere; then BakedTextureBRDF returns
    exactly trunc(c * 255) / 255 per channel at 4097 random surface points (one black tap would break this), render_view with it equals render_view with a
    module that returns those constants bit for bit under the same seeds, and python -m iris_amd.render --textures writes its files"""
    from iris_amd import render as R
    from iris_amd.model.emitter import SLFEmitter
    from iris_amd.model.texture import BakedTextureBRDF
    from iris_amd.utils import export as E
    from iris_amd.utils.cameras import view_rays
    v, f, scene = ico()
    data, bake, crf, K, c2w = write_room(tmp_path)
    tex = tmp_path / "texture"
    E.main(["--mesh", str(data / "scene.obj"), "--emitter_path", str(bake), "--dir_save", str(tex), "--tex_res", "256", "--atlas", "area", "--dilate", "2",
            "--material", "test_texture_material:const_material", "--device", DEV, "--verify", "4097"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[INFO] verify:")]
    assert len(line) == 1, line
    psnr = [float(t.split(" dB")[0]) for t in line[0].split("PSNR ")[1].replace("albedo ", "").replace("roughness ", "").replace("metallic ", "").split(", ")]
    print(line[0])
    assert len(psnr) == 3 and all(p > 20 * np.log10(255.0) for p in psnr)                    # truncation to 8 bits costs less than 1 / 255 per value
    net = BakedTextureBRDF.from_export(str(tex), v, f, torch.device(DEV))
    want = dequantised()
    x = dev(surface_points(v, f, 4097, 5))
    got, exact = net(x), want(x)
    for k in ("albedo", "roughness", "metallic"):
        assert torch.equal(got[k], exact[k]), (k, got[k][:2], exact[k][:2])
    # the same image through both materials
    em = SLFEmitter(str(bake / "emitter.pth"), str(bake / "vslf_0.npz")).to(DEV)
    rays = view_rays({"kind": "real", "K": K, "c2w": c2w}, (24, 32), torch.device(DEV), ray_diff=True)
    outs = []
    for material in (net, want):
        torch.manual_seed(11); torch.cuda.manual_seed(11)
        outs.append(R.render_view(scene, em, material, crf.to(DEV), rays, (24, 32), 4, 4, 2))
    for k in ("rgb_full", "rgb_ldr", "kd", "a_prime", "roughness", "metallic", "emission", "slf"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert float(outs[0]["rgb_full"].max()) > 0 and float(outs[0]["roughness"].min()) > 0.4
    # the command line
    outp = tmp_path / "out"
    R.main(["--experiment_name", "exp", "--checkpoint_path", str(tmp_path / "ckpt"), "--ckpt", "last.ckpt", "--dataset", "generic", str(data), "--cameras",
            str(data / "cameras.json"), "--emitter_path", str(bake), "--output_path", str(outp), "--split", "val", "--SPP", "4", "--spp", "4", "--indir_depth", "2",
            "--crf_basis", "3", "--textures", str(tex), "--seed", "3", "--device", "0"])
    for folder, name in (("rgb", "rgb_full"), ("diffuse", "kd"), ("a_prime", "a_prime"), ("roughness", "roughness"), ("metallic", "metallic"), ("emission", "emission")):
        assert (outp / "val" / folder / f"00000_{name}.exr").exists(), folder
    from iris_amd.utils.exr import read_exr
    rough = read_exr(str(outp / "val" / "roughness" / "00000_roughness.exr"))[..., 0]
    assert np.abs(rough - want.values[1].item()).max() <= 1e-6                                # every pixel sees the sphere from inside
