"""The render stage on the GPU (iris_amd/csrc/iris_render.h, iris_amd/utils/render.py, iris_amd/render.py) against tests/golden/render_intrinsics.npz -- the
reference's render.py:178-220 through its own functions, in float32 and float64 (tools/make_render_golden.py) -- and against the documented per-sample formula
in plain torch (tests/render_formula.py, which tests/test_render_cpu.py ties to the reference's float64 run to 1e-15).

Sums are compared elementwise under
    deviation <= max(8 d32, spp 2^-24 max |x|)           per map, max norm
with d32 the map's largest deviation between a float32 and a float64 evaluation of the same lines and x the map's per-sample terms (tests/test_propagation.py's
and tests/test_crf.py's rule).  No figures from an MI355X are recorded in this file; the tests print them."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from render_formula import MAPS, bound, fixture, pixel_means, sample_terms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN_KEYS = ("pos", "nrm", "wo", "e0", "valid_next", "albedo", "roughness", "metallic", "u2")


@functools.lru_cache(maxsize=None)
def setup():
    """(fixture, scene, emitter) on the GPU, built once"""
    import tempfile
    from iris_amd.model.emitter import SLFEmitter
    from iris_amd.model.slf import VoxelSLF
    from iris_amd.utils.path_tracing import Scene
    f = fixture()
    tmp = tempfile.mkdtemp()
    ep, sp = write_emitter_files(f, tmp)
    return f, Scene(f["verts"], f["faces"], device=torch.device(DEV)), SLFEmitter(ep, sp).to(DEV)


def write_emitter_files(f, folder, slf_name="vslf.npz"):
    from iris_amd.model.slf import VoxelSLF
    slf = VoxelSLF(torch.from_numpy(f["slf_mask"]), float(f["voxel_min"]), float(f["voxel_max"]))
    slf.radiance[:] = torch.from_numpy(f["slf_radiance"])
    ep, sp = os.path.join(folder, "emitter.pth"), os.path.join(folder, slf_name)
    torch.save({"is_emitter": torch.from_numpy(f["is_emitter"]), "emitter_vertices": torch.from_numpy(f["emitter_vertices"]), "emitter_area": torch.from_numpy(f["emitter_area"]),
                "emitter_normal": torch.zeros(4, 3), "emitter_radiance": torch.from_numpy(f["emitter_radiance"])}, ep)
    torch.save({"mask": torch.from_numpy(f["slf_mask"]), "voxel_min": float(f["voxel_min"]), "voxel_max": float(f["voxel_max"]), "weight": slf.state_dict()}, sp)
    return ep, sp


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def launch(em, inputs, B, spp, out=None):
    """iris_render_intrinsics on per-sample arrays (numpy, in IN_KEYS order); returns the dict of (B, c) maps"""
    from iris_amd import _lib as L
    from iris_amd.utils.render import new_maps
    pos, nrm, wo, e0, vn, alb, rough, metal, u2 = (T(a) for a in inputs)
    out = new_maps(B, DEV) if out is None else out
    rad = em.radiance_on(DEV)
    L.check(L.lib().iris_render_intrinsics(em.handle(DEV), em.slf.handle(DEV), L.ptr(rad), L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(e0.to(torch.int32)), L.ptr(vn.to(torch.bool)),
                                           L.ptr(alb), L.ptr(rough.reshape(-1).contiguous()), L.ptr(metal.reshape(-1).contiguous()), L.ptr(u2), B, spp,
                                           *(L.ptr(out[k]) for k, _ in MAPS), L.stream()))
    torch.cuda.synchronize()
    return out


def terms(f, dtype, inputs):
    return sample_terms(dtype, *inputs, f["emitter_radiance"], f["slf_inds"], f["slf_radiance"], float(f["voxel_min"]), float(f["voxel_max"]))


def test_kernel_on_the_recorded_inputs():
    """both rounds accumulated into one set of maps, no intersector and no material network involved: every map within max(8 d32, spp 2^-24 max|x|) of the
    reference's float32 result, d32 = the reference's own float32 / float64 deviation"""
    f, _, em = setup()
    B, spp = int(f["H"]) * int(f["W"]), int(f["spp"])
    out, xmax = None, {k: 0.0 for k, _ in MAPS}
    for r in range(int(f["rounds"])):
        inputs = [f[f"{k}_{r}"] for k in IN_KEYS]
        out = launch(em, inputs, B, spp, out)
        x, _ = terms(f, torch.float64, inputs)
        for k, _ in MAPS:
            xmax[k] = max(xmax[k], float(x[k].abs().max()))
    for k, _ in MAPS:
        got = out[k].cpu().numpy().astype(np.float64)
        d32 = float(np.abs(f[f"map32_{k}"].astype(np.float64) - f[f"map64_{k}"]).max())
        bnd = bound(d32, spp, xmax[k])
        dev32, dev64 = float(np.abs(got - f[f"map32_{k}"]).max()), float(np.abs(got - f[f"map64_{k}"]).max())
        print(f"{k}: against the reference's float32 maps {dev32:.3g}, against its float64 maps {dev64:.3g} (bound {bnd:.3g}, d32 {d32:.3g}, max|x| {xmax[k]:.3g})")
        assert np.isfinite(got).all() and dev32 <= bnd, k


def test_exact_cases():
    """a pixel whose samples all miss: kd = a_prime = roughness = 1, metallic = emission = 0 exactly, everything finite; zero-sum emitter samples keep their
    material values: a pixel made of them alone equals the formula's kept values, not the defaults"""
    f, _, em = setup()
    spp = int(f["spp"])
    inputs = [f[f"{k}_0"] for k in IN_KEYS]
    e0, vn = inputs[3], inputs[4]
    miss = np.nonzero(~vn & (e0 < 0))[0][:2 * spp]
    zs = np.concatenate([np.nonzero(e0 == 2)[0][:spp], np.nonzero(e0 == 3)[0][:spp]])
    assert len(miss) == 2 * spp and len(zs) == 2 * spp
    sel = np.concatenate([miss, zs])                       # pixels 0, 1: misses; pixel 2: radiance row (0,0,0); pixel 3: row (1,-1,0)
    sub = [a[sel] for a in inputs]
    out = launch(em, sub, 4, spp)
    for k, _ in MAPS:
        assert bool(torch.isfinite(out[k]).all()), k
    for k, v in (("kd", 1.0), ("a_prime", 1.0), ("roughness", 1.0), ("metallic", 0.0), ("emission", 0.0)):
        assert bool((out[k][:2] == v).all()), (k, out[k][:2])
    x, keep = terms(f, torch.float64, sub)
    assert bool(keep[2 * spp:].all()) and not bool(keep[:2 * spp].any())
    d = {k: float((out[k][2:].cpu().double() - pixel_means(x[k], spp)[2:]).abs().max()) for k, _ in MAPS}
    print("zero-sum emitter pixels against the formula:", d)
    assert d["roughness"] <= 4 * spp * 2.0 ** -24 and d["metallic"] <= 4 * spp * 2.0 ** -24 and d["kd"] <= 4 * spp * 2.0 ** -24
    assert float((out["roughness"][2:] - 1).abs().max()) > 1e-3                # not the default
    assert bool((out["emission"][2] == 0).all()) and out["emission"][3].cpu().tolist() == [1.0, -1.0, 0.0]


@functools.lru_cache(maxsize=None)
def synthetic(spp, B=37):
    """B pixels x spp samples of every class: random frames, roughness in [0.2, 1] (the GGX terms stay well conditioned: d32 is rounding-sized), radiance rows 0..3 of
    the fixture's table (two of them sum to zero), misses with the zero normal and position an intersector returns, positions across the SLF's box and beyond"""
    f = fixture()
    g = torch.Generator().manual_seed(100 + spp)
    N = B * spp
    nrm = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    wo = torch.nn.functional.normalize(nrm + 0.7 * torch.randn(N, 3, generator=g), dim=-1)
    below = (wo * nrm).sum(-1, keepdim=True).clamp_max(0)
    wo = torch.nn.functional.normalize(wo - 2 * below * nrm, dim=-1)          # mirrored above the surface, as ray_intersect's face-forwarded normals guarantee
    pos = torch.rand(N, 3, generator=g) * 5.0 - 0.5
    cls = torch.randint(0, 10, (N,), generator=g)          # 0: miss, 1: emitter, else surface
    e0 = torch.where(cls == 1, torch.randint(0, 4, (N,), generator=g), torch.full((N,), -1)).to(torch.int32)
    vn = cls >= 2
    nrm[cls == 0] = 0; pos[cls == 0] = 0
    alb, rough, metal = torch.rand(N, 3, generator=g), torch.rand(N, 1, generator=g) * 0.8 + 0.2, torch.rand(N, 1, generator=g)
    metal[::7] = 0; metal[3::7] = 1; rough[5::11] = 1
    u2 = torch.rand(N, 2, generator=g)
    inputs = [a.numpy() for a in (pos, nrm, wo, e0, vn, alb, rough, metal, u2)]
    x64, _ = terms(f, torch.float64, inputs)
    x32, _ = terms(f, torch.float32, inputs)
    return inputs, {k: pixel_means(x64[k], spp) for k, _ in MAPS}, {k: pixel_means(x32[k], spp) for k, _ in MAPS}, {k: float(x64[k].abs().max()) for k, _ in MAPS}


@pytest.mark.parametrize("spp", [1, 3, 5, 64, 70])
def test_spp_against_the_formula(spp):
    """one lane group per pixel at 1, 3 (4 lanes), 5 (8 lanes), 64 (a whole wave) and 70 (two rounds of a wave); 37 pixels: more than one wave, the last one partly
    filled.  Against the float64 formula under the bound; two launches give the same bits; a second launch into the first result doubles it exactly."""
    _, _, em = setup()
    B = 37
    inputs, m64, m32, xmax = synthetic(spp)
    a = launch(em, inputs, B, spp)
    b = launch(em, inputs, B, spp)
    twice = launch(em, inputs, B, spp, {k: v.clone() for k, v in a.items()})
    for k, _ in MAPS:
        d32 = float((m32[k].double() - m64[k]).abs().max())
        bnd = bound(d32, spp, xmax[k])
        dev = float((a[k].cpu().double() - m64[k]).abs().max())
        print(f"spp {spp} {k}: deviation {dev:.3g} (bound {bnd:.3g}, d32 {d32:.3g}, max|x| {xmax[k]:.3g})")
        assert dev <= bnd, k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        assert torch.equal(twice[k], a[k] + a[k]), k


def test_render_primary():
    """wi = normalize(rays_d + dxdu u + dydv v) with u, v in [0,1) within 2e-6 (tests/test_pt_single.py's bound for sampled directions); e0, valid_next, pos, nrm
    bit for bit those of iris_intersect + iris_pt_primary_emit on the same directions; wo = -wi"""
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import ray_intersect
    f, scene, em = setup()
    B, spp = int(f["H"]) * int(f["W"]), int(f["spp"])
    ro, rd, dx, dy, dudv = T(f["rays_o"]), T(f["rays_d"]), T(f["dx_du"]), T(f["dy_dv"]), T(f["dudv_0"]).reshape(2, B, spp).contiguous()
    N = B * spp
    wi, wo, pos, nrm = (torch.empty(N, 3, device=DEV) for _ in range(4))
    e0, vn = torch.empty(N, device=DEV, dtype=torch.int32), torch.empty(N, device=DEV, dtype=torch.bool)
    L.check(L.lib().iris_render_primary(scene.handle, em.handle(DEV), L.ptr(ro), L.ptr(rd), L.ptr(dx), L.ptr(dy), L.ptr(dudv), B, spp, L.ptr(wi), L.ptr(wo), L.ptr(pos), L.ptr(nrm),
                                        L.ptr(e0), L.ptr(vn), L.stream()))
    want = torch.nn.functional.normalize(rd[:, None] + dx[:, None] * dudv[0][..., None] + dy[:, None] * dudv[1][..., None], dim=-1).reshape(N, 3)
    np.testing.assert_allclose(wi.cpu().numpy(), want.cpu().numpy(), atol=2e-6, rtol=0)
    np.testing.assert_allclose(wi.cpu().numpy(), f["wi_0"], atol=2e-6, rtol=0)                 # the reference's own jittered directions
    assert torch.equal(wo, -wi)
    p2, n2, _, tri, _ = ray_intersect(scene, ro.repeat_interleave(spp, 0), wi)
    e2, v2 = torch.empty_like(e0), torch.empty_like(vn)
    L.check(L.lib().iris_pt_primary_emit(em.handle(DEV), L.ptr(tri), N, L.ptr(e2), L.ptr(v2), L.stream()))
    assert torch.equal(e0, e2) and torch.equal(vn, v2)
    assert torch.equal(pos.view(torch.int32), p2.view(torch.int32)) and torch.equal(nrm.view(torch.int32), n2.view(torch.int32))
    assert 0 < int(vn.sum()) < N and int((e0 >= 0).sum()) > 0 and int((~vn & (e0 < 0)).sum()) > 0


class Replay:
    """material_net that returns the recorded rows of the round in call order (chunks arrive in pixel order)"""

    def __init__(self, f, r):
        self.rows, self.off = [T(f[f"{k}_{r}"]) for k in ("albedo", "roughness", "metallic")], 0

    def __call__(self, position):
        n, o = position.shape[0], self.off
        self.off += n
        return {"albedo": self.rows[0][o:o + n], "roughness": self.rows[1][o:o + n], "metallic": self.rows[2][o:o + n]}


def run_rounds(f, scene, em, chunk):
    from iris_amd.utils.render import render_intrinsics
    rays = [T(f[k]) for k in ("rays_o", "rays_d", "dx_du", "dy_dv")]
    out, dbg = None, []
    for r in range(int(f["rounds"])):
        d = {}
        out = render_intrinsics(scene, em, Replay(f, r), *rays, int(f["spp"]), out=out, uniforms=[T(f[f"dudv_{r}"]), T(f[f"u2_{r}"])], chunk=chunk, debug=d)
        dbg.append(d)
    return out, dbg


def test_render_intrinsics_end_to_end():
    """head + replayed material rows + kernel on the fixture's rays with the recorded draws: each map within relative L2 1e-5 of the reference's (the bar of the
    integrators in tests/test_pt_single.py), per-sample e0 / valid_next equal to the reference's, chunk = 7 pixels the same bits as one pass; CPU tensors refused"""
    from iris_amd import _lib as L
    from iris_amd.utils.render import render_intrinsics
    f, scene, em = setup()
    out, dbg = run_rounds(f, scene, em, None)
    for r, d in enumerate(dbg):
        assert np.array_equal(d["e0"].cpu().numpy(), f[f"e0_{r}"]) and np.array_equal(d["valid_next"].cpu().numpy(), f[f"valid_next_{r}"]), r
    for k, _ in MAPS:
        e = rel_l2(out[k].cpu().numpy(), f[f"map32_{k}"])
        print(f"{k}: relative L2 against the reference {e:.3g}")
        assert e <= 1e-5, k
    chunked, _ = run_rounds(f, scene, em, 7)
    for k, _ in MAPS:
        assert torch.equal(out[k].view(torch.int32), chunked[k].view(torch.int32)), k
    own = render_intrinsics(scene, em, Replay(f, 0), *[T(f[k]) for k in ("rays_o", "rays_d", "dx_du", "dy_dv")], int(f["spp"]))       # its own draws
    assert all(bool(torch.isfinite(own[k]).all()) for k, _ in MAPS) and float(own["emission"].max()) > 1.0
    with pytest.raises(L.IrisError):
        render_intrinsics(scene, em, Replay(f, 0), *[torch.from_numpy(f[k]) for k in ("rays_o", "rays_d", "dx_du", "dy_dv")], int(f["spp"]))


def test_render_view_and_cli(tmp_path, monkeypatch):
    """python -m iris_amd.render on the fixture's room at 24 x 16, SPP 4, spp 2, indir_depth 2, with a checkpoint written here: the reference's file names exist, the
    EXR files read back equal what render_view returns for the same seed, metrics.txt parses; a round count of 2 halves what two single rounds sum to"""
    from iris_amd import render as R
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.cameras import view_rays
    from iris_amd.utils.exr import read_exr
    from stub_material import StubMaterial
    f, scene, em = setup()
    H, W = int(f["H"]), int(f["W"])
    data, bake, ckpt_dir, outp = tmp_path / "data", tmp_path / "bake", tmp_path / "ckpt" / "exp", tmp_path / "out"
    for d in (data, bake, ckpt_dir):
        d.mkdir(parents=True)
    with open(data / "scene.obj", "w") as fh:
        fh.writelines("v {:.9g} {:.9g} {:.9g}\n".format(*v) for v in f["verts"].tolist())
        fh.writelines("f {} {} {}\n".format(*(i + 1 for i in t)) for t in f["faces"].tolist())
    write_emitter_files(f, str(bake), "vslf_0.npz")
    write_emitter_files(f, str(bake), "vslf.npz")
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (k + 1)) * 0.05 for k in range(3)]))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    torch.save({"state_dict": {"model_crf." + k: v for k, v in crf.state_dict().items()}}, ckpt_dir / "last.ckpt")
    gt = np.full((H, W, 3), 0.5, np.float32)
    from iris_amd.utils.exr import write_exr
    write_exr(str(data / "gt.exr"), gt)
    with open(data / "cameras.json", "w") as fh:
        json.dump({"img_hw": [H, W], "views": [{"K": f["K"].tolist(), "c2w": f["c2w"].tolist(), "image": "gt.exr", "exposure": 1.2}]}, fh)
    argv = ["--experiment_name", "exp", "--checkpoint_path", str(tmp_path / "ckpt"), "--ckpt", "last.ckpt", "--dataset", "generic", str(data), "--cameras", str(data / "cameras.json"),
            "--emitter_path", str(bake), "--output_path", str(outp), "--split", "val", "--SPP", "4", "--spp", "2", "--indir_depth", "2", "--crf_basis", "3",
            "--material", "stub_material:material", "--seed", "3"]
    R.main(argv)
    root = outp / "val"
    names = {"rgb": "rgb_full", "diffuse": "kd", "a_prime": "a_prime", "roughness": "roughness", "metallic": "metallic", "emission": "emission"}
    for folder, name in names.items():
        assert (root / folder / f"00000_{name}.exr").exists(), folder
    assert (root / "merge").is_dir() and (root / "slf" / "00000_slf.exr").exists()
    try:
        import PIL      # noqa
        assert (root / "rgb" / "00000_rgb_full.png").exists() and (root / "diffuse" / "00000_kd.png").exists()
    except ImportError:
        assert not (root / "rgb" / "00000_rgb_full.png").exists()
    lines = open(root / "rgb" / "metrics.txt").read().splitlines()
    assert lines[0] == "Name, PSNR" and lines[1].startswith("00000, ") and lines[2].startswith("mean ")
    assert float(lines[1].split(", ")[1]) == float(lines[2].split(", ")[1]) > 0
    # the same view through render_view with the CLI's seed: the files hold the returned maps
    rays = view_rays({"kind": "real", "K": f["K"], "c2w": f["c2w"]}, (H, W), torch.device(DEV), ray_diff=True)
    torch.manual_seed(3 * 1000003); torch.cuda.manual_seed(3 * 1000003)
    out = R.render_view(scene, em, StubMaterial(), crf.to(DEV), rays, (H, W), 4, 2, 2, exposure=1.2, gt=gt)
    assert out["rounds"] == 2 and abs(out["psnr"] - float(lines[1].split(", ")[1])) < 1e-4
    for folder, key in (("rgb", "rgb_full"), ("diffuse", "kd"), ("a_prime", "a_prime"), ("emission", "emission"), ("slf", "slf")):
        np.testing.assert_array_equal(read_exr(str(root / folder / f"00000_{names.get(folder, 'slf')}.exr")), out[key].cpu().numpy(), err_msg=folder)
    for key in ("roughness", "metallic"):
        np.testing.assert_array_equal(read_exr(str(root / key / f"00000_{key}.exr"))[..., 1], out[key].cpu().numpy(), err_msg=key)
    assert out["rgb_ldr"].shape == (H, W, 3) and float(out["rgb_ldr"].min()) >= 0 and float(out["rgb_full"].max()) > 1
    # SPP // spp = 2 divides the sum of the two rounds by 2: the same draws as two one-round calls
    from iris_amd.utils.render import new_maps, render_intrinsics
    torch.manual_seed(9); torch.cuda.manual_seed(9)
    one = new_maps(H * W, DEV)
    render_intrinsics(scene, em, StubMaterial(), *rays, 2, out=one)
    first = {k: v.clone() for k, v in one.items()}
    render_intrinsics(scene, em, StubMaterial(), *rays, 2, out=one)
    assert float((one["kd"] - first["kd"]).abs().max()) > 0
    torch.manual_seed(9); torch.cuda.manual_seed(9)
    monkeypatch.setattr(R, "path_tracing", lambda *a, **k: torch.zeros(H * W, 3, device=DEV))      # (the integrator draws too: taken out, the intrinsics' draws are the two calls')
    both = R.render_view(scene, em, StubMaterial(), None, rays, (H, W), 4, 2, 0, denoise=False)
    for k, c in MAPS:
        assert torch.equal(both[k].reshape(-1), (one[k] / 2).reshape(-1)), k
