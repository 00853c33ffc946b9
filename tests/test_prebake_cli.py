"""The three pre-bake commands (python -m iris_amd.slf_bake / extract_emitter_ldr / slf_refine) and their setup in iris_amd/utils/stage.py.

On the CPU: extract_emitter_ldr --mode update, the photograph-path helper on the four layouts, and every refusal (non-zero status, one line on stderr, before any
device is opened).  On the GPU: the three commands as subprocesses on a real-layout scene written into tmp_path -- the cube [-1, 1]^3 with a light quad under its
+y face, four cameras of 12 x 16 pixels (view 0 validates), 8-bit photographs that are bright exactly where the light quad projects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

H, W = 12, 16
BOX_V = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)] + [[-0.5, 0.9, -0.5], [0.5, 0.9, -0.5], [0.5, 0.9, 0.5], [-0.5, 0.9, 0.5]], np.float32)
BOX_F = np.array([t for a, b, c, d in [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5), (8, 9, 10, 11)] for t in ((a, b, c), (a, c, d))],
                 np.int32)                                                    # -z, +z, -y, +y, -x, +x, the light quad (triangles 12, 13)
CAMS = [((0, 0, 0), (0, 0, 1), (0, 1, 0)), ((0.1, 0.0, 0.2), (0.1, 0.0, -0.8), (0, 1, 0)), ((0.1, 0.1, 0.0), (1.1, 0.1, 0.0), (0, 1, 0)), ((0.0, 0.2, -0.1), (0.0, 1.2, -0.1), (0, 0, 1))]
EXPOSURES = np.array([9.0, 0.6, 0.9, 1.2], np.float32)


def write_emor(path, n=32, n_basis=11):
    s = torch.linspace(0, 1, n)
    blocks = [("E", s), ("f0", s ** 0.45)] + [("h(%d)" % (j + 1), torch.sin(3.14159 * s * (j + 1)) * 0.05) for j in range(n_basis)]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for name, values in blocks:
            fh.write(name + " =\n" + "\n".join(" ".join("%.9g" % float(x) for x in values[r:r + 4]) for r in range(0, n, 4)) + "\n")


def write_real_scene(root, images=None, n_views=len(CAMS), hw=(H, W)):
    """cam.txt / K_list.txt, scene.obj, ldr/{:03d}_0001.png by CAPTURE id for the train split, ldr/cam/exposure.npy; crf/emor.txt under root.
    images: {capture id: (H, W, 3) uint8}; by default random ones."""
    from iris_amd.utils.cameras import real_split_ids
    from iris_amd.utils.texture import write_png
    g = np.random.default_rng(3)
    scene = root / "scene"
    os.makedirs(scene / "ldr" / "cam")
    cams = [CAMS[i % len(CAMS)] for i in range(n_views)]
    with open(scene / "cam.txt", "w") as fh:
        fh.write("%d\n" % len(cams) + "".join("%g %g %g\n" % tuple(row) for cam in cams for row in cam))
    with open(scene / "K_list.txt", "w") as fh:
        fh.write("%d\n" % len(cams) + "".join("10 0 8\n0 10 6\n0 0 1\n" for _ in cams))
    with open(scene / "scene.obj", "w") as fh:
        fh.write("".join("v %g %g %g\n" % tuple(v) for v in BOX_V) + "".join("f %d %d %d\n" % tuple(f + 1) for f in BOX_F))
    np.save(scene / "ldr" / "cam" / "exposure.npy", np.resize(EXPOSURES, n_views))
    for i in real_split_ids(n_views, "train"):
        write_png(scene / "ldr" / ("%03d_0001.png" % i), images[i] if images else g.integers(0, 256, (*hw, 3)).astype(np.uint8))
    write_emor(str(root / "crf" / "emor.txt"))
    return scene


# ---- CPU
def test_update_mode_replaces_the_emitter_radiance_only(tmp_path, capsys):
    from iris_amd.extract_emitter_ldr import cli
    emitter = {"is_emitter": torch.tensor([False, True, True]), "emitter_vertices": torch.rand(2, 3, 3), "emitter_area": torch.rand(2), "emitter_normal": torch.rand(2, 3),
               "emitter_radiance": torch.zeros(3, 3)}
    torch.save(emitter, tmp_path / "emitter.pth")
    learned = torch.rand(3, 3)
    torch.save({"state_dict": {"emitter.radiance": learned, "material.x": torch.zeros(1)}}, tmp_path / "with.ckpt")
    torch.save({"state_dict": {"material.x": torch.zeros(1)}}, tmp_path / "without.ckpt")
    common = ["--scene", str(tmp_path), "--output", str(tmp_path), "--dataset", "real", "--mode", "update"]
    assert cli(common + ["--ckpt", str(tmp_path / "with.ckpt")]) == 0
    after = torch.load(tmp_path / "emitter.pth")
    assert set(after) == set(emitter) and torch.equal(after["emitter_radiance"], learned)
    for k in emitter:
        if k != "emitter_radiance":
            assert torch.equal(after[k], emitter[k]), k
    capsys.readouterr()
    assert cli(common + ["--ckpt", str(tmp_path / "without.ckpt")]) != 0
    assert "emitter.radiance" in capsys.readouterr().err
    assert torch.equal(torch.load(tmp_path / "emitter.pth")["emitter_radiance"], learned)       # the refused call wrote nothing
    assert cli(["--scene", str(tmp_path), "--output", str(tmp_path), "--dataset", "real", "--mode", "test"]) == 0


def test_photographs_of_a_real_layout_go_by_capture_id(tmp_path):
    from iris_amd.utils import stage
    scene = write_real_scene(tmp_path, n_views=12)                               # views 0 and 10 validate
    img_hw, views, photos = stage.load_photographs("real", str(scene), str(scene), 1.0, ldr_img_dir="ldr")
    ids = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
    assert img_hw == (H, W) and len(views) == len(ids)
    assert [p for p, _ in photos] == [str(scene / "ldr" / ("%03d_0001.png" % i)) for i in ids]
    assert [e for _, e in photos] == [float(np.resize(EXPOSURES, 12)[i]) for i in ids]
    _, _, photos = stage.load_photographs("real", str(scene), str(scene), 1.0, ldr_img_dir="ldr", max_views=2)
    assert len(photos) == 2
    from iris_amd.utils.exr import write_exr
    os.makedirs(scene / "Image")
    write_exr(scene / "Image" / "000_0001.exr", np.zeros((H, W, 3), np.float32))  # where the reference takes the image size from
    _, _, photos = stage.load_photographs("real", str(scene), str(scene), 1.0)    # no --ldr_img_dir: Image/, no exposures
    assert photos[0] == (str(scene / "Image" / "001_0001.png"), None)
    a = stage.read_photograph(str(scene / "ldr" / "001_0001.png"), (H, W))
    assert a.dtype == np.uint8 and a.shape == (H, W, 3)


def test_photographs_of_a_synthetic_layout(tmp_path):
    from iris_amd.utils import stage
    from iris_amd.utils.texture import write_png
    root = tmp_path / "scene"
    os.makedirs(root / "train" / "ldr" / "cam")
    frames = [{"transform_matrix": np.eye(4).tolist()} for _ in range(3)]
    with open(root / "train" / "transforms.json", "w") as fh:
        json.dump({"camera_angle_x": 0.9, "frames": frames}, fh)
    write_png(root / "train" / "ldr" / "000_0001.png", np.zeros((H, W, 3), np.uint8))
    np.save(root / "train" / "ldr" / "cam" / "exposure.npy", np.array([0.5, 1.5, 2.5], np.float32))
    img_hw, views, photos = stage.load_photographs("synthetic", str(root), str(root), 1.0, ldr_img_dir="ldr")
    assert img_hw == (H, W) and [v["kind"] for v in views] == ["synthetic"] * 3
    assert photos == [(str(root / "train" / "ldr" / ("%03d_0001.png" % i)), e) for i, e in enumerate((0.5, 1.5, 2.5))]


def test_photographs_of_a_scannetpp_layout(tmp_path):
    from iris_amd.utils import stage
    psdf = tmp_path / "data" / "room" / "psdf"
    os.makedirs(psdf)
    with open(psdf / "train_test_lists.json", "w") as fh:
        json.dump({"train": ["b.JPG", "a.JPG"], "test": ["c.JPG"]}, fh)
    frames = [{"file_path": "images/" + n, "transform_matrix": np.eye(4).tolist()} for n in ("a.JPG", "b.JPG", "c.JPG")]
    with open(psdf / "transforms_all.json", "w") as fh:
        json.dump({"h": H, "w": W, "fl_x": 10.0, "fl_y": 10.0, "cx": 8.0, "cy": 6.0, "frames": frames}, fh)
    img_hw, views, photos = stage.load_photographs("scannetpp", str(tmp_path), "room", 1.0)
    assert img_hw == (H, W) and [v["name"] for v in views] == ["b.JPG", "a.JPG"]          # the split list's order
    assert photos == [(str(psdf / "images" / n), 1.0) for n in ("b.JPG", "a.JPG")]


def test_photographs_of_a_cameras_json(tmp_path):
    from iris_amd.utils import stage
    K, c2w = [[10, 0, 8], [0, 10, 6], [0, 0, 1]], np.eye(4)[:3].tolist()
    with open(tmp_path / "cameras.json", "w") as fh:
        json.dump({"img_hw": [H, W], "views": [{"K": K, "c2w": c2w, "image": "shots/a.png", "exposure": 2.5}, {"K": K, "c2w": c2w, "image": "/abs/b.png"}]}, fh)
    img_hw, views, photos = stage.load_photographs("real", "unused", "unused", 1.0, cameras_json=str(tmp_path / "cameras.json"))
    assert img_hw == (H, W) and len(views) == 2
    assert photos == [(str(tmp_path / "shots" / "a.png"), 2.5), ("/abs/b.png", 1.0)]
    with open(tmp_path / "bare.json", "w") as fh:
        json.dump({"img_hw": [H, W], "views": [{"K": K, "c2w": c2w}]}, fh)
    from iris_amd._lib import IrisError
    with pytest.raises(IrisError, match="image"):
        stage.load_photographs("real", "unused", "unused", 1.0, cameras_json=str(tmp_path / "bare.json"))


def test_refusals_come_before_the_device(tmp_path, capsys, monkeypatch):
    from iris_amd import extract_emitter_ldr, slf_bake, slf_refine
    scene = write_real_scene(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a refused command opened the device"))
    common = ["--scene", str(scene), "--output", str(tmp_path / "out"), "--dataset", "real"]
    monkeypatch.chdir(tmp_path)                                                  # crf/emor.txt is here
    # a photograph whose size is not the view's: --res_scale 0.5 against full-size files (the view's size comes from the first photograph, halved)
    for mod in (slf_bake, extract_emitter_ldr, slf_refine):
        assert mod.cli(common + ["--ldr_img_dir", "ldr", "--res_scale", "0.5"] + (["--crf_basis", "3"] if mod is slf_refine else [])) != 0
        err = capsys.readouterr().err
        assert "resizing" in err and "001_0001.png" in err
    # the real and synthetic layouts have no exposures without --ldr_img_dir
    for mod in (slf_bake, slf_refine):
        assert mod.cli(common) != 0
        assert "ldr_img_dir" in capsys.readouterr().err
        assert mod.cli(["--scene", str(scene), "--output", str(tmp_path / "out"), "--dataset", "synthetic"]) != 0
        assert "ldr_img_dir" in capsys.readouterr().err
    # no EMoR file under the working directory and no --emor_path
    monkeypatch.chdir(scene)
    assert slf_bake.cli(common + ["--ldr_img_dir", "ldr"]) != 0
    assert "EMoR" in capsys.readouterr().err
    assert slf_refine.cli(common + ["--ldr_img_dir", "ldr", "--crf_basis", "3"]) != 0
    assert "EMoR" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


# ---- GPU
@pytest.mark.gpu
def test_the_three_commands_on_a_real_layout_scene(tmp_path):
    from iris_amd import slf_bake as sb
    from iris_amd.model.crf import EmorCRF
    from iris_amd.model.emitter import SLFEmitter
    from iris_amd.utils import cameras, stage
    from iris_amd.utils.path_tracing import Scene, ray_intersect
    dev = torch.device("cuda:0")
    scene = Scene(BOX_V, BOX_F, device=dev)
    # the photographs: dim noise, bright exactly where a light triangle is the primary hit
    os.makedirs(tmp_path / "probe")
    probe = write_real_scene(tmp_path / "probe")                                 # (camera files only: its photographs are not used)
    _, views = cameras.load_real(str(probe), img_hw=(H, W), split="train")
    ids, g, images, batches = [1, 2, 3], np.random.default_rng(7), {}, []
    for i, view in zip(ids, views):
        rays = torch.cat(cameras.view_rays(view, (H, W), dev), -1)
        idx = ray_intersect(scene, rays[:, :3].contiguous(), rays[:, 3:].contiguous())[3].cpu().numpy()
        assert (idx >= 0).all()
        img = g.integers(0, 100, (H * W, 3)).astype(np.uint8)
        img[idx >= 12] = 250
        images[i] = img.reshape(H, W, 3)
        batches.append({"rays": rays, "rgbs": torch.from_numpy(img), "exposure": float(EXPOSURES[i])})
    assert any((im == 250).all(-1).any() for im in images.values())
    root = tmp_path / "run"
    os.makedirs(root)
    data = write_real_scene(root, images=images)
    out = root / "out"
    env = dict(os.environ, PYTHONPATH=REPO)
    common = ["--scene", str(data), "--output", str(out), "--dataset", "real", "--ldr_img_dir", "ldr"]

    def run(module, *extra):
        p = subprocess.run([sys.executable, "-m", "iris_amd." + module] + common + list(extra), env=env, cwd=str(root), capture_output=True, text=True, timeout=300)
        print(p.stdout, p.stderr)
        assert p.returncode == 0, module

    run("slf_bake", "--voxel_num", "16")
    run("extract_emitter_ldr", "--threshold", "0.9")
    crf = EmorCRF(3, emor_path=str(root / "crf" / "emor.txt"))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    stage.write_checkpoint(str(root / "last.ckpt"), {}, crf.state_dict(), {}, epoch=1, global_step=1, hyper_parameters={})
    run("slf_refine", "--ckpt", str(root / "last.ckpt"), "--crf_basis", "3", "--load", "vslf.npz", "--save", "vslf_0.npz")
    for name in ("vslf.npz", "emitter.pth", "vslf_0.npz"):
        assert (out / name).exists(), name

    baked = torch.load(out / "vslf.npz")
    want = sb.bake_slf(scene, batches, res_spatial=16, dataset="real", device=dev, crf=EmorCRF(emor_path=str(root / "crf" / "emor.txt")).to(dev))
    assert baked["voxel_min"] == want["voxel_min"] and baked["voxel_max"] == want["voxel_max"]
    assert torch.equal(baked["mask"], want["mask"]) and tuple(baked["mask"].shape) == (16, 16, 16)
    assert torch.equal(baked["weight"]["inds"], want["weight"]["inds"]) and torch.equal(baked["weight"]["count"], want["weight"]["count"])
    assert int(baked["weight"]["count"].sum()) == len(ids) * H * W
    np.testing.assert_allclose(baked["weight"]["radiance"].numpy(), want["weight"]["radiance"].numpy(), rtol=2e-5, atol=1e-6)

    emitter = torch.load(out / "emitter.pth")
    assert emitter["is_emitter"].tolist() == [False] * 12 + [True, True]
    assert emitter["emitter_vertices"].shape == (2, 3, 3) and emitter["emitter_radiance"].shape == (14, 3)

    refined = torch.load(out / "vslf_0.npz")
    assert torch.equal(refined["mask"], baked["mask"]) and torch.equal(refined["weight"]["inds"], baked["weight"]["inds"])
    assert torch.equal(refined["weight"]["count"], baked["weight"]["count"])     # counted anew from zero: the same hits, not twice as many
    again = sb.refine_slf(baked, scene, batches, dev, crf=crf.to(dev))
    np.testing.assert_allclose(refined["weight"]["radiance"].numpy(), again["weight"]["radiance"].numpy(), rtol=2e-5, atol=1e-6)
    assert not np.allclose(refined["weight"]["radiance"].numpy(), baked["weight"]["radiance"].numpy())       # another response model
    assert SLFEmitter(str(out / "emitter.pth"), str(out / "vslf_0.npz")) is not None
