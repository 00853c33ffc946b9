"""The 8-bit resize kernel (iris_amd/csrc/iris_resize.h, iris_amd/utils/resize.py) on the GPU, byte for byte against tests/resize_ref.py (linear) and PIL
(nearest), and the scannetpp layout at --res_scale 0.5 through the stages that open photographs.

Stage fixture: the closed cube [-1, 1]^3 as data/<scene>/scans/scene.ply, 3 train views (and one test view) of 12 x 16 pixels from inside it, random 8-bit
photographs, albedo priors and segment-id images under psdf/; --res_scale 0.5 makes the views 6 x 8."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resize_ref
from conftest import REPO
from test_prebake_cli import write_emor
from test_resize_cpu import CONTENTS, FULL, SIZES, SIZE_IDS, content, linear_ref, nearest_pil

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCH = 17                                    # more than one launch's 16 images


def up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ---- the kernel
@pytest.mark.parametrize("sizes", SIZES, ids=SIZE_IDS)
def test_linear_equals_the_restatement(sizes):
    from iris_amd.utils.resize import resize_u8
    src, dst = sizes
    for channels in (3, 1):
        for name in CONTENTS:
            got = resize_u8(up(content(name, src, channels)), dst, "linear")
            want = linear_ref(name, src, dst, channels)
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (channels, name)
        images = [content("random", src, channels, seed) for seed in range(BATCH)]
        want = np.stack([linear_ref("random", src, dst, channels, seed) for seed in range(BATCH)])
        given = [up(a) for a in images]
        got = resize_u8(given, dst, "linear")                                                    # a list in, a list out
        assert isinstance(got, list) and len(got) == BATCH
        if src == dst:
            assert got is given
        assert np.array_equal(torch.stack(got).cpu().numpy(), want), channels
        if channels == 3:
            for n in (1, BATCH):                                                                 # (N, H, W, 3) in, (N, Ht, Wt, 3) out
                got = resize_u8(up(np.stack(images[:n])), dst, "linear")
                assert tuple(got.shape) == (n, *dst, 3) and np.array_equal(got.cpu().numpy(), want[:n]), n


@pytest.mark.parametrize("sizes", SIZES, ids=SIZE_IDS)
def test_nearest_equals_pil(sizes):
    from iris_amd.utils.resize import resize_u8
    src, dst = sizes
    for channels in (1, 3):
        images = [content("random", src, channels, seed) for seed in range(BATCH)]
        want = np.stack([nearest_pil(np.array(a), dst) for a in images])
        got = resize_u8(up(images[0]), dst, "nearest")
        assert tuple(got.shape) == want[0].shape and np.array_equal(got.cpu().numpy(), want[0]), channels
        got = resize_u8([up(a) for a in images], dst, "nearest")
        assert np.array_equal(torch.stack(got).cpu().numpy(), want), channels


@pytest.mark.parametrize("sizes", FULL, ids=["exact2", "general"])
def test_a_scannetpp_photograph_at_half_resolution(sizes):
    from iris_amd.utils.resize import resize_u8
    src, dst = sizes
    image = content("random", src, 3)
    assert np.array_equal(resize_u8(up(image), dst, "linear").cpu().numpy(), linear_ref("random", src, dst, 3))
    ids = np.ascontiguousarray(image[..., 2])
    assert np.array_equal(resize_u8(up(ids), dst, "nearest").cpu().numpy(), nearest_pil(ids, dst))


def test_same_size_returns_the_input_and_two_calls_agree():
    from iris_amd.utils.resize import resize_u8
    t = up(content("random", (9, 9), 3))
    assert resize_u8(t, (9, 9)) is t and resize_u8(t, (9, 9), "nearest") is t
    for src, dst in (((24, 40), (9, 15)), ((12, 16), (6, 8)), ((20, 70), (9, 67))):
        batch = up(np.stack([content("random", src, 3, seed) for seed in range(BATCH)]))
        for mode in ("linear", "nearest"):
            a, b = resize_u8(batch, dst, mode), resize_u8(batch, dst, mode)
            assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_refusals_launch_nothing(monkeypatch):
    from iris_amd import _lib as L
    from iris_amd.utils.resize import resize_u8
    monkeypatch.setattr(L.lib(), "iris_resize_u8", lambda *a: pytest.fail("a refused call launched"))
    good = up(content("random", (12, 16), 3))
    for bad in (good.cpu(), good.float(), torch.zeros(12, 16, 4, dtype=torch.uint8, device=DEV), torch.zeros(2, 12, 16, 1, 1, dtype=torch.uint8, device=DEV),
                [good, good[:6].contiguous()], []):
        with pytest.raises(L.IrisError):
            resize_u8(bad, (6, 8))
    with pytest.raises(L.IrisError, match="mode"):
        resize_u8(good, (6, 8), "cubic")
    with pytest.raises(L.IrisError, match="65535"):
        resize_u8(good, (0, 8))


def test_the_library_refuses_bad_arguments():
    import ctypes as C
    from iris_amd import _lib as L
    lib, t, out = L.lib(), up(content("random", (12, 16), 3)), torch.empty(6 * 8 * 3, dtype=torch.uint8, device=DEV)
    ptrs = (C.c_void_p * 1)(t.data_ptr())
    for args in ((ptrs, 1, 12, 16, 4, 0, None, None, None, None, L.ptr(out), 6, 8), (ptrs, 1, 12, 16, 3, 2, None, None, None, None, L.ptr(out), 6, 8),
                 (ptrs, 1, 12, 16, 3, 0, None, None, None, None, L.ptr(out), 5, 8), (ptrs, 0, 12, 16, 3, 0, None, None, None, None, L.ptr(out), 6, 8),
                 (ptrs, 1, 12, 16, 3, 0, None, None, None, None, L.ptr(out), 6, 0), ((C.c_void_p * 1)(None), 1, 12, 16, 3, 0, None, None, None, None, L.ptr(out), 6, 8)):
        assert lib.iris_resize_u8(*args, L.stream()) != 0 and b"iris_resize_u8" in lib.iris_last_error()


# ---- the stages on a tiny scannetpp scene
H, W, SCALE = 12, 16, 0.5
HW2 = (6, 8)
SCENE = "45b0dac5e3"
NAMES = ["b.png", "a.png", "c.png"]
CUBE_V = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
CUBE_F = np.array([t for a, b, c, d in [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)] for t in ((a, b, c), (a, c, d))], np.int32)


def write_scannetpp_scene(root, hw=(H, W), shrink=None, seed=3):
    """-> {name: (photograph, albedo prior, segment-id image)} as written.  shrink: write every image through resize_ref at that size (the tree a run at
    --res_scale 1 reads), the intrinsics scaled to match."""
    from iris_amd.utils.texture import write_png
    from test_train_brdf_crf import look_at
    g = np.random.default_rng(seed)
    psdf = root / "data" / SCENE / "psdf"
    for d in ("images", "albedo", "seg"):
        os.makedirs(psdf / d)
    os.makedirs(root / "data" / SCENE / "scans")
    with open(root / "data" / SCENE / "scans" / "scene.ply", "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
                 "property list uchar int vertex_indices\nend_header\n" % (len(CUBE_V), len(CUBE_F)))
        fh.write("".join("%g %g %g\n" % tuple(v) for v in CUBE_V) + "".join("3 %d %d %d\n" % tuple(f) for f in CUBE_F))
    poses = [look_at((0.1, -0.05, 0.0), (0.2, 0.1, 1.0)), look_at((-0.3, 0.2, 0.1), (0.4, -0.1, -1.0)), look_at((0.2, 0.1, -0.4), (1.0, 0.3, 0.5)), look_at((0, 0, 0), (0, 1, 0.2))]
    frames = []
    for name, c2w in zip(["a.png", "b.png", "c.png", "t.png"], poses):                          # (the file's order is not the split's)
        m = np.eye(4)
        m[:3] = c2w
        m[:3, 1:3] *= -1                                                                          # OpenCV -> OpenGL: the loader negates them back
        frames.append({"file_path": "images/" + name, "transform_matrix": m.tolist()})
    s = 1.0 if shrink is None else shrink[0] / hw[0]
    with open(psdf / "transforms_all.json", "w") as fh:
        json.dump({"h": int(hw[0] * s), "w": int(hw[1] * s), "fl_x": 10.0 * s, "fl_y": 10.0 * s, "cx": 8.0 * s, "cy": 6.0 * s, "frames": frames}, fh)
    with open(psdf / "train_test_lists.json", "w") as fh:
        json.dump({"train": NAMES, "test": ["t.png"]}, fh)
    written = {}
    for name in NAMES:
        rgb, albedo = (g.integers(0, 256, (*hw, 3)).astype(np.uint8) for _ in range(2))
        seg = np.stack([g.integers(0, 256, hw), g.integers(0, 256, hw), g.integers(0, 5, hw) * 3 + 7], -1).astype(np.uint8)       # the ids are channel B
        written[name] = (rgb, albedo, seg)
        for folder, a in zip(("images", "albedo", "seg"), written[name]):
            write_png(psdf / folder / name, a if shrink is None or folder == "seg" else resize_ref.resize_linear_u8(a, shrink))
    return written


def test_photograph_batches_resize_on_the_device(tmp_path):
    from iris_amd.utils import stage
    written = write_scannetpp_scene(tmp_path)
    img_hw, views, photos = stage.load_photographs("scannetpp", str(tmp_path), SCENE, SCALE)
    assert img_hw == HW2 and [v["name"] for v in views] == NAMES
    batches = list(stage.photograph_batches(views, img_hw, photos, torch.device(DEV), resize=stage.layout_resizes("scannetpp")))
    assert len(batches) == 3
    for b, name in zip(batches, NAMES):
        assert b["image"].is_cuda and b["image"].dtype == torch.uint8 and b["img_hw"] == HW2 and b["exposure"] == 1.0
        assert np.array_equal(b["image"].cpu().numpy(), resize_ref.resize_linear_u8(written[name][0], HW2)), name


def test_slf_bake_runs_the_scannetpp_command_line_at_half_resolution(tmp_path, monkeypatch):
    """scripts/scannetpp/bathroom2/train.sh:23-25's argument list, unchanged, on full-size photographs; the file equals the one a run at scale 1 writes
    from photographs shrunk beforehand by the restatement (and the intrinsics halved), as closely as tests/test_prebake_cli.py compares a command's file
    with the function's result: the float sums are atomics, everything else is exact."""
    from iris_amd import slf_bake
    full, half = tmp_path / "full", tmp_path / "half"
    os.makedirs(full)
    os.makedirs(half)
    write_scannetpp_scene(full)
    write_scannetpp_scene(half, shrink=HW2)
    write_emor(str(tmp_path / "crf" / "emor.txt"))
    cmd = [sys.executable, "-m", "iris_amd.slf_bake", "--dataset_root", str(full), "--scene", SCENE, "--output", str(tmp_path / "out_full"), "--res_scale", str(SCALE),
           "--dataset", "scannetpp"]
    p = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=REPO), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "3 views of 6 x 8" in p.stdout
    monkeypatch.chdir(tmp_path)                                                                   # crf/emor.txt is here
    assert slf_bake.cli(["--dataset_root", str(half), "--scene", SCENE, "--output", str(tmp_path / "out_half"), "--dataset", "scannetpp"]) == 0
    got, want = torch.load(tmp_path / "out_full" / "vslf.npz"), torch.load(tmp_path / "out_half" / "vslf.npz")
    assert got["voxel_min"] == want["voxel_min"] and got["voxel_max"] == want["voxel_max"]
    assert torch.equal(got["mask"], want["mask"]) and tuple(got["mask"].shape) == (256, 256, 256)
    assert torch.equal(got["weight"]["inds"], want["weight"]["inds"]) and torch.equal(got["weight"]["count"], want["weight"]["count"])
    assert int(got["weight"]["count"].sum()) == 3 * HW2[0] * HW2[1]
    np.testing.assert_allclose(got["weight"]["radiance"].numpy(), want["weight"]["radiance"].numpy(), rtol=2e-5, atol=1e-6)
    assert float(got["weight"]["radiance"].abs().max()) > 0


def test_training_files_of_a_scannetpp_scene_at_half_resolution(tmp_path):
    from iris_amd.utils.dataset import PixelSet
    from iris_amd.utils.dataset.files import load_training_files
    written = write_scannetpp_scene(tmp_path)
    files = load_training_files("scannetpp", str(tmp_path), None, res_scale=SCALE, device=DEV, scene=SCENE)
    assert files["img_hw"] == HW2 and [v["name"] for v in files["views"]] == NAMES and files["synthetic"] is False and files["cache"] is None
    assert files["exposure"].dtype == np.float32 and files["exposure"].tolist() == [1.0, 1.0, 1.0]
    for k, name in enumerate(NAMES):
        rgb, albedo, seg = written[name]
        assert all(files[key][k].is_cuda and files[key][k].dtype == torch.uint8 for key in ("rgb", "int_albedo", "segmentation"))
        assert np.array_equal(files["rgb"][k].cpu().numpy(), resize_ref.resize_linear_u8(rgb, HW2)), name
        assert np.array_equal(files["int_albedo"][k].cpu().numpy(), resize_ref.resize_linear_u8(albedo, HW2)), name
        assert np.array_equal(files["segmentation"][k].cpu().numpy(), nearest_pil(np.ascontiguousarray(seg[..., 2]), HW2).reshape(-1)), name
    ps = PixelSet(files["views"], files["img_hw"], files["rgb"], segmentation=files["segmentation"], int_albedo=files["int_albedo"], exposure=files["exposure"],
                  synthetic=False, batch_size=64, device=DEV)
    n = HW2[0] * HW2[1]
    assert ps.n_pixels == 3 * n
    batch = ps[0]
    idx = batch["idx"].cpu().numpy()
    flat = {key: np.concatenate([files[key][k].cpu().numpy().reshape(n, -1) for k in range(3)]) for key in ("rgb", "int_albedo", "segmentation")}
    assert np.array_equal(batch["rgbs"].cpu().numpy(), (flat["rgb"][idx] / 255.0).astype(np.float32))
    assert np.array_equal(batch["int_albedo"].cpu().numpy(), (flat["int_albedo"][idx] / 255.0).astype(np.float32))
    assert np.array_equal(batch["segmentation"].cpu().numpy(), flat["segmentation"][idx, 0].astype(np.int64))
    assert (batch["exposure"].cpu().numpy() == 1.0).all()
    # a file of the views' size is taken as it is
    same = load_training_files("scannetpp", str(tmp_path), None, res_scale=1.0, device=DEV, scene=SCENE)
    assert same["img_hw"] == (H, W) and np.array_equal(same["rgb"][1].cpu().numpy(), written[NAMES[1]][0])
    assert np.array_equal(same["segmentation"][1].cpu().numpy(), written[NAMES[1]][2][..., 2].reshape(-1))


def test_train_brdf_crf_runs_the_scannetpp_command_line_at_half_resolution(tmp_path):
    """modelled on tests/test_train_brdf_crf.py::test_cli_trains_a_real_layout_scene: the shading cache by position in the split, at the views' 6 x 8"""
    from iris_amd.utils.exr import write_exr
    from test_train_brdf_crf import VMAX, VMIN
    write_scannetpp_scene(tmp_path)
    g = np.random.default_rng(5)
    for d in ("diffuse", "specular"):
        os.makedirs(tmp_path / "shading" / d)
    for position in range(3):
        write_exr(tmp_path / "shading" / "diffuse" / ("%03d.exr" % position), g.random((*HW2, 3)).astype(np.float32))
        for k in range(2):
            for level in range(6):
                write_exr(tmp_path / "shading" / "specular" / ("%03d_%d_%d.exr" % (position, k, level)), g.random((*HW2, 3)).astype(np.float32))
    torch.save(dict(voxel_min=VMIN, voxel_max=VMAX), tmp_path / "vslf.npz")
    write_emor(str(tmp_path / "crf" / "emor.txt"))
    cmd = [sys.executable, "-m", "iris_amd.train_brdf_crf", "--experiment_name", "cli", "--dataset", "scannetpp", str(tmp_path), "--scene", SCENE, "--res_scale", str(SCALE),
           "--has_part", "0", "--val_frame", "0", "--voxel_path", str(tmp_path / "vslf.npz"), "--cache_dir", str(tmp_path / "shading"), "--batch_size", "64",
           "--max_epochs", "1", "--la", "0.01", "--checkpoint_path", str(tmp_path / "checkpoints"), "--log_path", str(tmp_path / "logs"), "--log_every", "1"]
    p = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=REPO), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "3 views of 6 x 8" in p.stdout
    state = torch.load(tmp_path / "checkpoints" / "cli" / "last.ckpt", map_location="cpu", weights_only=False)
    assert state["epoch"] == 1 and state["global_step"] >= 2 and "material.mlp.params" in state["state_dict"] and "model_crf.weight" in state["state_dict"]
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "cli" / "metrics.jsonl")]
    assert len(lines) == state["global_step"] and all(np.isfinite(e["train/loss"]) for e in lines)
