"""The BRDF-CRF training stage on the GPU (iris_amd/train_brdf_crf.py): BRDFCRFTrainer over a PixelSet of the open-box scene, its checkpoint, schedule,
resume, and the command line on a real-layout scene written into tmp_path.

Fixture: the cube [-1, 1]^3 without its +z face, 3 views of 12 x 16 pixels from inside it, random 8-bit images and albedo priors, 4 segment ids, a random
ShadingCache, an EmorCRF from arrays, NGPBRDF(...).init_parameters(), batches of 64 pixels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

H, W, V, BATCH = 12, 16, 3, 64
HW, N = H * W, H * W * V
VMIN, VMAX = -1.5, 1.5


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    return np.concatenate([np.stack([r, u, f], 1), np.asarray(eye, np.float64).reshape(3, 1)], 1).astype(np.float32)


def cameras():
    """inside the open box: view 0 looks out of the missing +z face (its outer columns still see the walls), 1 and 2 at walls"""
    poses = [look_at((0.1, -0.05, 0.0), (0.2, 0.1, 1.0)), look_at((-0.3, 0.2, 0.1), (0.4, -0.1, -1.0)), look_at((0.2, 0.1, -0.4), (1.0, 0.3, 0.5))]
    Ks = [np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32) for fx, fy, cx, cy in ((6.0, 6.5, 7.9, 6.1), (7.0, 7.5, 8.0, 6.0), (9.0, 8.5, 8.2, 5.7))]
    return [dict(kind="real", K=K, c2w=p) for K, p in zip(Ks, poses)]


BOX_V = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
BOX_F = np.array([t for a, b, c, d in [(0, 1, 3, 2), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)] for t in ((a, b, c), (a, c, d))], np.int32)     # -z, -y, +y, -x, +x


def stores(seed=0):
    g = np.random.default_rng(seed)
    return dict(rgb=g.integers(0, 256, (N, 3)).astype(np.uint8), int_albedo=g.integers(0, 256, (N, 3)).astype(np.uint8),
                segmentation=(g.integers(0, 4, N) * 3 + 7).astype(np.int32), exposure=(0.5 + g.random(V)).astype(np.float32))


def emor_arrays(n=64):
    s = torch.linspace(0, 1, n)
    return s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)])


def make_trainer(tmp_path, **hp):
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.model.crf import EmorCRF
    from iris_amd.train_brdf_crf import BRDFCRFTrainer, default_hparams
    from iris_amd.utils.dataset import PixelSet
    from iris_amd.utils.path_tracing import Scene
    from iris_amd.utils.shading_cache import ShadingCache
    dev = torch.device("cuda:0")
    torch.manual_seed(0)                                      # the epochs' orders (PixelSet.resample draws from torch's generator on the device)
    st = stores()
    ps = PixelSet(cameras(), (H, W), st["rgb"], segmentation=st["segmentation"], int_albedo=st["int_albedo"], exposure=st["exposure"], batch_size=BATCH, device=dev)
    cache = ShadingCache(N, 6, dev)
    g = torch.Generator().manual_seed(8)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=g).to(dev))
    ps.attach_cache(cache)
    n = ps.restrict_to_hits(Scene(BOX_V, BOX_F, device=dev), store_positions=True)
    assert BATCH < n < N, n                                   # more than one batch; the rays through the opening are gone
    material = NGPBRDF(VMIN, VMAX).init_parameters(seed=5).to(dev)
    crf = EmorCRF.from_arrays(*emor_arrays()).to(dev)
    hparams = default_hparams(batch_size=BATCH, experiment_name="exp", checkpoint_path=str(tmp_path / "checkpoints"), log_path=str(tmp_path / "logs"),
                              has_part=0, la=0.01, learning_rate=1e-2, log_every=1, **hp)
    return BRDFCRFTrainer(material, crf, ps, hparams)


def optimizer_state(trainer):
    p = trainer.material.mlp.params
    st = trainer.optimizer.state[p]
    return p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])


def test_two_epochs_then_the_checkpoint_loads_where_the_stages_load_it(tmp_path):
    from iris_amd.model.brdf import load_ngpbrdf
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.optim import FusedAdam
    tr = make_trainer(tmp_path)
    assert isinstance(tr.optimizer, FusedAdam) and len(tr.optimizer.param_groups[0]["params"]) == 2
    steps = len(tr.ps)
    tr.fit(2)
    assert tr.epoch == 2 and tr.global_step == 2 * steps and len(tr.history) == 2 * steps
    losses = [e["train/loss"] for e in tr.history]
    print("losses", np.round(losses, 5).tolist())
    assert all(np.isfinite(e[k]) for e in tr.history for k in e)
    assert np.mean(losses[steps:]) < losses[0], (np.mean(losses[steps:]), losses[0])
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "exp" / "metrics.jsonl")]
    assert lines == tr.history and [e["step"] for e in lines] == list(range(2 * steps))
    assert {"train/loss", "train/loss_c", "train/loss_d", "train/loss_seg", "train/loss_a", "train/psnr"} <= set(lines[0])
    assert tr.material._native.keys[0].fresh(tr.material.mlp.params)                  # the last step left the handle current

    ckpt = tmp_path / "checkpoints" / "exp" / "last.ckpt"
    assert ckpt.exists()
    pos = tr.ps[0]["positions"][:64].contiguous()
    with torch.no_grad():
        mine = tr.material(pos)
    loaded = load_ngpbrdf(VMIN, VMAX, str(ckpt))(pos)
    for k in mine:
        assert torch.equal(mine[k], loaded[k]), k
    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert state["epoch"] == 2 and state["global_step"] == 2 * steps and state["hyper_parameters"]["learning_rate"] == 1e-2
    crf = EmorCRF.from_arrays(*emor_arrays())
    crf.load_state_dict({k.replace("model_crf.", ""): v for k, v in state["state_dict"].items() if "model_crf." in k})
    assert torch.equal(crf.weight.detach(), tr.model_crf.weight.detach().cpu()) and float(crf.weight.detach().abs().max()) > 0


def test_schedule_and_frozen_crf(tmp_path):
    tr = make_trainer(tmp_path, milestones=[1], scheduler_rate=0.5, freeze_crf=1)
    with torch.no_grad():
        tr.model_crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    before = tr.model_crf.weight.detach().clone()
    assert len(tr.optimizer.param_groups[0]["params"]) == 1 and not tr.model_crf.weight.requires_grad
    tr.fit(1)
    assert tr.optimizer.param_groups[0]["lr"] == 1e-2 and all(e["lr"] == 1e-2 for e in tr.history)
    tr.fit(2)
    assert tr.optimizer.param_groups[0]["lr"] == 1e-2 * 0.5 and tr.history[-1]["lr"] == 5e-3 and tr.history[-1]["epoch"] == 1
    assert torch.equal(tr.model_crf.weight.detach().view(torch.int32), before.view(torch.int32))


def test_resume(tmp_path):
    first = make_trainer(tmp_path)
    first.fit(1)
    steps = first.global_step
    want = optimizer_state(first)
    crf_state = first.optimizer.state[first.model_crf.weight]
    second = make_trainer(tmp_path, resume=True)
    assert second.epoch == 1 and second.global_step == steps
    got = optimizer_state(second)
    for a, b in zip(want[:3], got[:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert got[3] == want[3] == float(steps)
    assert torch.equal(second.model_crf.weight.detach(), first.model_crf.weight.detach())
    assert torch.equal(second.optimizer.state[second.model_crf.weight]["exp_avg"], crf_state["exp_avg"])
    second.fit(2)
    assert second.epoch == 2 and second.global_step == 2 * steps and second.history[0]["step"] == steps and second.history[0]["epoch"] == 1
    assert float(second.optimizer.state[second.material.mlp.params]["step"]) == 2 * steps
    fresh = make_trainer(tmp_path / "elsewhere", resume=True)              # nothing to resume from: starts at zero
    assert fresh.epoch == 0 and fresh.global_step == 0


def test_sgd_and_ranger(tmp_path):
    from iris_amd import _lib as L
    tr = make_trainer(tmp_path, optimizer="SGD")
    assert isinstance(tr.optimizer, torch.optim.SGD)
    tr.fit(1)
    assert tr.global_step == len(tr.ps) and all(np.isfinite(e["train/loss"]) for e in tr.history)
    with pytest.raises(L.IrisError, match="Ranger"):
        make_trainer(tmp_path, optimizer="Ranger")


# ---- the command line on a real-layout scene
def write_real_scene(root):
    """cam.txt / K_list.txt (4 views: view 0 is in the validation split, 1..3 train), scene.obj, ldr/{:03d}_0001.png, ldr/albedo, ldr/cam/exposure.npy,
    segmentation/{:03d}.exr by capture id; the shading cache by position in the split; vslf.npz; crf/emor.txt under the working directory"""
    from iris_amd.utils.exr import write_exr
    from iris_amd.utils.texture import write_png
    g = np.random.default_rng(3)
    scene = root / "scene"
    for d in (scene / "ldr" / "albedo", scene / "ldr" / "cam", scene / "segmentation", root / "shading" / "diffuse", root / "shading" / "specular", root / "crf"):
        os.makedirs(d)
    cams = [((0, 0, 0), (0, 0, 1), (0, 1, 0)), ((0.1, 0.0, 0.2), (0.1, 0.0, -0.8), (0, 1, 0)), ((0.1, 0.1, 0.0), (1.1, 0.1, 0.0), (0, 1, 0)), ((0.0, 0.2, -0.1), (0.0, 1.2, -0.1), (0, 0, 1))]
    with open(scene / "cam.txt", "w") as fh:
        fh.write("%d\n" % len(cams) + "".join("%g %g %g\n" % tuple(row) for cam in cams for row in cam))
    with open(scene / "K_list.txt", "w") as fh:
        fh.write("%d\n" % len(cams) + "".join("10 0 8\n0 10 6\n0 0 1\n" for _ in cams))
    with open(scene / "scene.obj", "w") as fh:
        fh.write("".join("v %g %g %g\n" % tuple(v) for v in BOX_V) + "".join("f %d %d %d\n" % tuple(f + 1) for f in BOX_F))
    np.save(scene / "ldr" / "cam" / "exposure.npy", np.array([9.0, 0.6, 0.9, 1.2], np.float32))
    for position, i in enumerate((1, 2, 3)):
        write_png(scene / "ldr" / ("%03d_0001.png" % i), g.integers(0, 256, (H, W, 3)).astype(np.uint8))
        write_png(scene / "ldr" / "albedo" / ("%03d_0001.png" % i), g.integers(0, 256, (H, W, 3)).astype(np.uint8))
        write_exr(scene / "segmentation" / ("%03d.exr" % i), np.repeat(g.integers(0, 4, (H, W, 1)).astype(np.float32), 3, axis=2))
        write_exr(root / "shading" / "diffuse" / ("%03d.exr" % position), g.random((H, W, 3)).astype(np.float32))
        for k in range(2):
            for level in range(6):
                write_exr(root / "shading" / "specular" / ("%03d_%d_%d.exr" % (position, k, level)), g.random((H, W, 3)).astype(np.float32))
    torch.save(dict(voxel_min=VMIN, voxel_max=VMAX), root / "vslf.npz")
    f0, basis = emor_arrays(32)
    blocks = [("E", torch.linspace(0, 1, 32)), ("f0", f0)] + [("h(%d)" % (j + 1), b) for j, b in enumerate(basis)]
    with open(root / "crf" / "emor.txt", "w") as fh:
        for name, values in blocks:
            fh.write(name + " =\n" + "\n".join(" ".join("%.9g" % float(x) for x in values[r:r + 4]) for r in range(0, 32, 4)) + "\n")
    return scene


def test_cli_trains_a_real_layout_scene(tmp_path):
    pytest.importorskip("PIL")
    scene = write_real_scene(tmp_path)
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, "-m", "iris_amd.train_brdf_crf", "--experiment_name", "cli", "--dataset", "real", str(scene), "--ldr_img_dir", "ldr", "--voxel_path",
           str(tmp_path / "vslf.npz"), "--cache_dir", str(tmp_path / "shading"), "--batch_size", str(BATCH), "--max_epochs", "1", "--has_part", "0", "--la", "0.01",
           "--checkpoint_path", str(tmp_path / "checkpoints"), "--log_path", str(tmp_path / "logs"), "--log_every", "2"]
    p = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0
    assert "accepted and ignored" in p.stdout
    state = torch.load(tmp_path / "checkpoints" / "cli" / "last.ckpt", map_location="cpu", weights_only=False)
    assert state["epoch"] == 1 and state["global_step"] >= 2 and "material.mlp.params" in state["state_dict"] and "model_crf.weight" in state["state_dict"]
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "cli" / "metrics.jsonl")]
    assert len(lines) == state["global_step"] // 2
    for e in lines:
        assert {"train/loss", "train/loss_c", "train/loss_d", "train/loss_seg", "train/loss_a", "train/psnr"} <= set(e) and np.isfinite(e["train/loss"])


def test_cli_refuses_what_is_not_built(tmp_path, capsys):
    from iris_amd.train_brdf_crf import cli
    common = ["--experiment_name", "x", "--ldr_img_dir", "ldr", "--cache_dir", str(tmp_path), "--checkpoint_path", str(tmp_path / "c"), "--log_path", str(tmp_path / "l")]
    assert cli(common + ["--dataset", "scannetpp", str(tmp_path), "--scene", "room"]) != 0
    assert "scannetpp" in capsys.readouterr().err
    assert cli(common + ["--dataset", "real", str(tmp_path), "--res_scale", "0.5"]) != 0
    assert "res_scale" in capsys.readouterr().err
    assert cli(common + ["--dataset", "real", str(tmp_path), "--optimizer", "Ranger"]) != 0
    assert "Ranger" in capsys.readouterr().err
    assert not (tmp_path / "c").exists() and not (tmp_path / "l").exists()
